"""include/gsfm_ba7.h: every declared entry point is exported with its ctypes prototype, the header is C99, and the argument checks run before
any device call (on a machine without a device a bad argument is reported as such, not as the missing device)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import have_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "gsfm_ba7.h")).read()


def test_library_exports_every_declared_entry_point():
    from globalsfmpy_amd import _abi
    lib = _abi.load_library()
    txt = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    names = sorted(set(re.findall(r"\b(gsfm_ba7_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["gsfm_ba7_abi_version", "gsfm_ba7_linearize", "gsfm_ba7_options_default", "gsfm_ba7_problem_create", "gsfm_ba7_problem_destroy", "gsfm_ba7_residuals",
                     "gsfm_ba7_schur_matvec", "gsfm_ba7_set_loss", "gsfm_ba7_solve", "gsfm_ba7_step_check", "gsfm_ba7_time_kernels"]
    for n in names:
        assert hasattr(lib, n), "libgsfm_rot.so does not export %s" % n
    assert lib.gsfm_ba7_abi_version() == 1 and "#define GSFM_BA7_ABI_VERSION 1" in HDR
    # the prototypes mirror the header's argument counts
    for n in names:
        if n in ("gsfm_ba7_abi_version",):
            continue
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % n, txt, flags=re.S).group(1)
        assert len(getattr(lib, n).argtypes) == decl.count(",") + 1, n
    # the defaults are gsfm_ba6.h's but for the stall rule, which looks over half of the iteration budget
    o6, o7 = _abi.BaOptions(), _abi.BaOptions()
    lib.gsfm_ba6_options_default(C.byref(o6))
    lib.gsfm_ba7_options_default(C.byref(o7))
    assert o7.cg_relative_tolerance == 1e-14 and (o6.cg_stall_iterations, o7.cg_stall_iterations, o7.max_cg_iterations) == (200, 1000, 2000)
    o7.cg_stall_iterations = o6.cg_stall_iterations
    assert bytes(o6) == bytes(o7)
    f = lib.gsfm_ba7_step_check
    assert f.restype is C.c_int and f.argtypes[5] is C.c_double and f.argtypes[6] is C.POINTER(_abi.BaOptions) and len(f.argtypes) == 17
    assert lib.gsfm_ba7_solve.argtypes[5] is C.POINTER(_abi.BaOptions) and lib.gsfm_ba7_solve.argtypes[6] is C.POINTER(_abi.BaSummary)
    assert lib.gsfm_ba7_problem_create.argtypes[3] is C.POINTER(C.c_uint8)   # focal_free


def test_pybind_module_reports_the_same_version():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "globalsfmpy_amd"))   # (the extension sits beside its shim)
    from globalsfmpy_amd import GlobalSfMpy
    assert GlobalSfMpy.ba7_abi_version() == 1


def test_header_is_pedantic_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use_ba7.c"
    src.write_text('#include "gsfm_ba7.h"\nint main(void) { gsfm_ba_options o; gsfm_ba7_options_default(&o); return gsfm_ba7_abi_version() == GSFM_BA7_ABI_VERSION && o.remove_gauge == 1 && o.cg_relative_tolerance < 1e-13 ? 0 : 1; }\n')
    exe = str(tmp_path / "use_ba7")
    lib_dir = os.path.join(ROOT, "globalsfmpy_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir,
                        "-lgsfm_rot", "-Wl,-rpath," + lib_dir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0


def test_argument_checks_run_before_any_device_call():
    """With or without a device: a bad argument is GSFM_ERR_INVALID_ARG (status 1), never the device's error."""
    from globalsfmpy_amd import _abi
    from globalsfmpy_amd.solver import FocalBundleProblem, SolverError
    K = np.tile([1000.0, 500.0, 400.0], (3, 1))
    xy = np.zeros((4, 2))
    cases = {"track_ptr[0]": (np.array([1, 2, 4], np.uint64), np.array([0, 1, 2, 0], np.uint32)),
             "decreasing": (np.array([0, 3, 2, 4], np.uint64), np.array([0, 1, 2, 0], np.uint32)),
             "camera index": (np.array([0, 2, 4], np.uint64), np.array([0, 1, 3, 0], np.uint32))}
    for what, (tp, oc) in cases.items():
        with pytest.raises(SolverError, match="status 1"):
            FocalBundleProblem(K, tp, oc, xy, focal_free=np.ones(3))
    with pytest.raises(ValueError, match="focal_free"):
        FocalBundleProblem(K, np.array([0, 2, 4], np.uint64), np.array([0, 1, 2, 0], np.uint32), xy, focal_free=np.ones(2))
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.gsfm_ba7_problem_create(3, None, None, None, 0, None, None, None, None, C.byref(h)) == 1
    assert lib.gsfm_ba7_problem_create(0, None, None, None, 0, None, None, None, None, None) == 1
    assert lib.gsfm_ba7_set_loss(None, None, 0) == 1 and lib.gsfm_ba7_solve(None, None, None, None, None, None, None) == 1
    assert lib.gsfm_ba7_residuals(None, None, None, None, None, None, None) == 1
    assert lib.gsfm_ba7_linearize(*([None] * 12)) == 1
    assert lib.gsfm_ba7_schur_matvec(None, None, 1e4, None, None) == 1
    assert lib.gsfm_ba7_step_check(None, None, None, None, None, 1e4, *([None] * 11)) == 1
    assert lib.gsfm_ba7_time_kernels(None, None, None, None, None, 1e4, 1, None) == 1
    lib.gsfm_ba7_problem_destroy(None)


def test_unsupported_loss_leaves_are_refused_before_the_handle_is_read():
    """tests/test_ba6_abi.py's test of the same name: the handle is a zeroed buffer, and a refusal returns before anything is read from it"""
    from globalsfmpy_amd import _abi
    lib = _abi.load_library()
    buf = C.create_string_buffer(1 << 16)
    h = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    refused = [(_abi.LOSS_CAUCHY, 10.0), (_abi.LOSS_ARCTAN, 10.0), (_abi.LOSS_TOLERANT, 10.0, 1.0), (_abi.LOSS_MAGSAC, 0.02, 3, 0), (99, 10.0), (_abi.LOSS_OP_SCALE, 2.0),
               (_abi.LOSS_TUKEY, 0.0), (_abi.LOSS_TUKEY, nan), (_abi.LOSS_GEMAN_MCCLURE, 10.0, inf), (_abi.LOSS_HUBER, 0.0), (_abi.LOSS_SOFT_L1, -1.0)]
    for node in refused:
        prog, n = _abi.make_program([node])
        assert lib.gsfm_ba7_set_loss(h, prog, n) == _abi.ERR_INVALID_ARG, node
    prog, _ = _abi.make_program([(_abi.LOSS_TUKEY, 10.0), (_abi.LOSS_TUKEY, 10.0)])
    assert lib.gsfm_ba7_set_loss(h, prog, 2) == _abi.ERR_INVALID_ARG and lib.gsfm_ba7_set_loss(h, None, 1) == _abi.ERR_INVALID_ARG
    assert not any(buf.raw)


@pytest.mark.skipif(have_gpu(), reason="CPU-only behaviour")
def test_fails_loudly_without_a_gpu():
    from globalsfmpy_amd.solver import FocalBundleProblem, SolverError
    with pytest.raises(SolverError, match="status 2: no HIP device: gsfm_ba7_problem_create"):
        FocalBundleProblem(np.ones((2, 3)), np.array([0, 2], np.uint64), np.array([0, 1], np.uint32), np.zeros((2, 2)))
