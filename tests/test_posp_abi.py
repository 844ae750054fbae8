"""include/gsfm_posp.h: every declared entry point is exported, the ctypes mirror follows the header's summary struct, gsfm_pos.h and its
ABI version are untouched, the header is C99, and the argument checks of gsfm_posp_problem_create and the refusal of a host-callback loss
run before any device call (on a machine without a device a bad argument is reported as such, not as the missing device)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import have_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "gsfm_posp.h")).read()


def test_library_exports_every_declared_entry_point():
    from globalsfmpy_amd import _abi
    lib = _abi.load_library()
    txt = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    names = sorted(set(re.findall(r"\b(gsfm_posp_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["gsfm_posp_abi_version", "gsfm_posp_linearize", "gsfm_posp_problem_create", "gsfm_posp_problem_destroy", "gsfm_posp_residuals",
                     "gsfm_posp_schur_matvec", "gsfm_posp_set_loss", "gsfm_posp_set_loss_callback", "gsfm_posp_solve", "gsfm_posp_step_check",
                     "gsfm_posp_time_kernels"]
    for n in names:
        assert hasattr(lib, n), "libgsfm_rot.so does not export %s" % n
    assert lib.gsfm_posp_abi_version() == 1 and "#define GSFM_POSP_ABI_VERSION 1" in HDR
    assert lib.gsfm_pos_abi_version() == 2   # gsfm_pos.h stays as it is


def test_struct_mirror_and_signatures():
    from globalsfmpy_amd import _abi
    lib = _abi.load_library()
    body = HDR[HDR.index("typedef struct {\n  gsfm_pos_summary pos;"):HDR.index("} gsfm_posp_summary;")]
    assert re.findall(r"^\s+(?:gsfm_pos_summary|uint64_t)\s+(\w+);", body, flags=re.M) == [n for n, _ in _abi.PospSummary._fields_]
    assert C.sizeof(_abi.PospSummary) == C.sizeof(_abi.PosSummary) + 16 and C.sizeof(_abi.PosSummary) == 4 * 10 + 8 * 7
    assert _abi.PospSummary.num_observations_used.offset == C.sizeof(_abi.PosSummary)
    d = _abi.PospSummary().as_dict()
    assert d["num_observations_used"] == 0 and d["num_active_points"] == 0 and d["num_dense_solves"] == 0 and "termination_name" in d
    f = lib.gsfm_posp_step_check
    assert f.restype is C.c_int and len(f.argtypes) == 13 and f.argtypes[3] is C.c_int32 and f.argtypes[4] is C.c_double and f.argtypes[5] is C.POINTER(_abi.PosOptions)
    assert len(lib.gsfm_posp_problem_create.argtypes) == 14 and lib.gsfm_posp_problem_create.argtypes[12] is C.c_double
    assert len(lib.gsfm_posp_linearize.argtypes) == 8 and len(lib.gsfm_posp_residuals.argtypes) == 8 and len(lib.gsfm_posp_solve.argtypes) == 6


def test_header_is_pedantic_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use_posp.c"
    src.write_text('#include "gsfm_posp.h"\nint main(void) { gsfm_posp_summary s; s.num_active_points = 0; return gsfm_posp_abi_version() == GSFM_POSP_ABI_VERSION '
                   '&& s.num_active_points == 0 ? 0 : 1; }\n')
    exe = str(tmp_path / "use_posp")
    lib_dir = os.path.join(ROOT, "globalsfmpy_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir,
                        "-lgsfm_rot", "-Wl,-rpath," + lib_dir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0


def test_argument_checks_run_before_any_device_call():
    """With or without a device: a bad argument is GSFM_ERR_INVALID_ARG (status 1) -- no cameras or edges GSFM_ERR_EMPTY, as
    gsfm_pos_problem_create -- never the device's error."""
    from globalsfmpy_amd import _abi
    from globalsfmpy_amd.solver import PointPositionProblem, SolverError
    ei, ej = np.array([0, 1], np.uint32), np.array([1, 2], np.uint32)
    rel, rot, K = np.eye(3)[:2], np.zeros((3, 3)), np.tile([1000.0, 500.0, 400.0], (3, 1))
    xy = np.zeros((4, 2))
    good = (np.array([0, 2, 4], np.uint64), np.array([0, 1, 2, 0], np.uint32))
    cases = {"track_ptr[0]": (np.array([1, 2, 4], np.uint64), good[1], 0.5), "decreasing": (np.array([0, 3, 2, 4], np.uint64), good[1], 0.5),
             "camera index": (good[0], np.array([0, 1, 3, 0], np.uint32), 0.5), "zero weight": good + (0.0,), "negative weight": good + (-0.5,),
             "nan weight": good + (float("nan"),), "infinite weight": good + (float("inf"),)}
    for what, (tp, oc, w) in cases.items():
        with pytest.raises(SolverError, match="status 1"):
            PointPositionProblem(3, ei, ej, rel, rot, rot, K, tp, oc, xy, w)
    with pytest.raises(SolverError, match="status 1"):
        PointPositionProblem(3, np.array([0, 3], np.uint32), ej, rel, rot, rot, K, good[0], good[1], xy)   # an edge's camera index
    lib = _abi.load_library()
    h = C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    tp = good[0].ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.gsfm_posp_problem_create(3, 2, u(ei), u(ej), p(rel), p(rot), None, None, 2, tp, u(good[1]), p(xy), 0.5, C.byref(h)) == 1   # observations without rays' inputs
    assert lib.gsfm_posp_problem_create(3, 2, u(ei), u(ej), p(rel), p(rot), p(rot), p(K), 2, None, u(good[1]), p(xy), 0.5, C.byref(h)) == 1
    assert lib.gsfm_posp_problem_create(3, 2, u(ei), u(ej), p(rel), None, None, None, 0, None, None, None, 0.5, C.byref(h)) == 1
    assert lib.gsfm_posp_problem_create(3, 2, u(ei), u(ej), p(rel), p(rot), None, None, 0, None, None, None, 0.5, None) == 1
    assert lib.gsfm_posp_problem_create(0, 0, None, None, None, None, None, None, 0, None, None, None, 0.5, C.byref(h)) == _abi.ERR_EMPTY
    assert h.value is None
    assert lib.gsfm_posp_set_loss(None, None, 0) == 1 and lib.gsfm_posp_solve(None, None, None, -1, None, None) == 1
    assert lib.gsfm_posp_set_loss_callback(None, _abi.LOSS_CALLBACK_FN(), None) == 1
    assert "callback" in lib.gsfm_last_error().decode()


@pytest.mark.skipif(have_gpu(), reason="CPU-only behaviour")
def test_fails_loudly_without_a_gpu():
    from globalsfmpy_amd.solver import PointPositionProblem, SolverError
    with pytest.raises(SolverError, match="no HIP device"):
        PointPositionProblem(2, np.array([0], np.uint32), np.array([1], np.uint32), np.array([[1.0, 0.0, 0.0]]), np.zeros((2, 3)))
