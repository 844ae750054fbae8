"""include/gsfm_ba6.h: every declared entry point is exported with its ctypes prototype, the header is C99, and the argument checks run before
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
HDR = open(os.path.join(ROOT, "include", "gsfm_ba6.h")).read()


def test_library_exports_every_declared_entry_point():
    from globalsfmpy_amd import _abi
    lib = _abi.load_library()
    txt = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    names = sorted(set(re.findall(r"\b(gsfm_ba6_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["gsfm_ba6_abi_version", "gsfm_ba6_linearize", "gsfm_ba6_options_default", "gsfm_ba6_problem_create", "gsfm_ba6_problem_destroy", "gsfm_ba6_residuals",
                     "gsfm_ba6_schur_matvec", "gsfm_ba6_set_loss", "gsfm_ba6_solve", "gsfm_ba6_step_check", "gsfm_ba6_time_kernels"]
    for n in names:
        assert hasattr(lib, n), "libgsfm_rot.so does not export %s" % n
    assert lib.gsfm_ba6_abi_version() == 1 and "#define GSFM_BA6_ABI_VERSION 1" in HDR
    # the prototypes mirror the header's argument counts
    for n in names:
        if n in ("gsfm_ba6_abi_version",):
            continue
        decl = re.search(r"\b%s\s*\(([^;]*)\);" % n, txt, flags=re.S).group(1)
        assert len(getattr(lib, n).argtypes) == decl.count(",") + 1, n
    # the defaults are gsfm_ba.h's but for the PCG tolerance
    o, o6 = _abi.BaOptions(), _abi.BaOptions()
    lib.gsfm_ba_options_default(C.byref(o))
    lib.gsfm_ba6_options_default(C.byref(o6))
    assert (o.cg_relative_tolerance, o6.cg_relative_tolerance) == (1e-12, 1e-14)
    o6.cg_relative_tolerance = o.cg_relative_tolerance
    assert bytes(o) == bytes(o6)
    f = lib.gsfm_ba6_step_check
    assert f.restype is C.c_int and f.argtypes[4] is C.c_double and f.argtypes[5] is C.POINTER(_abi.BaOptions)
    assert lib.gsfm_ba6_solve.argtypes[4] is C.POINTER(_abi.BaOptions) and lib.gsfm_ba6_solve.argtypes[5] is C.POINTER(_abi.BaSummary)


def test_header_is_pedantic_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use_ba6.c"
    src.write_text('#include "gsfm_ba6.h"\nint main(void) { gsfm_ba_options o; gsfm_ba6_options_default(&o); return gsfm_ba6_abi_version() == GSFM_BA6_ABI_VERSION && o.remove_gauge == 1 && o.cg_relative_tolerance < 1e-13 ? 0 : 1; }\n')
    exe = str(tmp_path / "use_ba6")
    lib_dir = os.path.join(ROOT, "globalsfmpy_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir,
                        "-lgsfm_rot", "-Wl,-rpath," + lib_dir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0


def test_argument_checks_run_before_any_device_call():
    """With or without a device: a bad argument is GSFM_ERR_INVALID_ARG (status 1), never the device's error."""
    from globalsfmpy_amd import _abi
    from globalsfmpy_amd.solver import FullBundleProblem, SolverError
    K = np.tile([1000.0, 500.0, 400.0], (3, 1))
    xy = np.zeros((4, 2))
    cases = {"track_ptr[0]": (np.array([1, 2, 4], np.uint64), np.array([0, 1, 2, 0], np.uint32)),
             "decreasing": (np.array([0, 3, 2, 4], np.uint64), np.array([0, 1, 2, 0], np.uint32)),
             "camera index": (np.array([0, 2, 4], np.uint64), np.array([0, 1, 3, 0], np.uint32))}
    for what, (tp, oc) in cases.items():
        with pytest.raises(SolverError, match="status 1"):
            FullBundleProblem(K, tp, oc, xy)
    lib = _abi.load_library()
    h = C.c_void_p()
    assert lib.gsfm_ba6_problem_create(3, None, None, 0, None, None, None, None, C.byref(h)) == 1
    assert lib.gsfm_ba6_problem_create(0, None, None, 0, None, None, None, None, None) == 1
    assert lib.gsfm_ba6_set_loss(None, None, 0) == 1 and lib.gsfm_ba6_solve(None, None, None, None, None, None) == 1
    assert lib.gsfm_ba6_residuals(None, None, None, None, None, None) == 1
    assert lib.gsfm_ba6_linearize(None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.gsfm_ba6_schur_matvec(None, None, 1e4, None, None) == 1
    assert lib.gsfm_ba6_step_check(None, None, None, None, 1e4, None, None, None, None, None, None, None, None, None, None) == 1
    assert lib.gsfm_ba6_time_kernels(None, None, None, None, 1e4, 1, None) == 1
    lib.gsfm_ba6_problem_destroy(None)


def test_unsupported_loss_leaves_are_refused_before_the_handle_is_read():
    """gsfm_ba6_set_loss answers status 1 for every leaf the kernels' loss_leaf_simple does not evaluate (it would fall through to `default:` -- no loss at
    all), for a width that is not positive and for a parameter that is not finite.  The handle here is not a problem at all (a zeroed
    buffer: no device is needed to have one): a refusal returns before anything is read from it.  Accepting Tukey and Geman-McClure writes
    into the handle, so tests/test_gpu_ba6.py asserts that on a real problem."""
    from globalsfmpy_amd import _abi
    lib = _abi.load_library()
    buf = C.create_string_buffer(1 << 16)
    h = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    refused = [(_abi.LOSS_CAUCHY, 10.0), (_abi.LOSS_ARCTAN, 10.0), (_abi.LOSS_TOLERANT, 10.0, 1.0), (_abi.LOSS_LONE_HALF, 10.0), (_abi.LOSS_LTWO, 10.0, 0.5),
               (_abi.LOSS_MAGSAC, 0.02, 3, 0), (_abi.LOSS_MAGSAC + 1, 10.0), (99, 10.0), (-1, 10.0), (_abi.LOSS_OP_SCALE, 2.0),
               (_abi.LOSS_TUKEY, 0.0), (_abi.LOSS_TUKEY, -10.0), (_abi.LOSS_TUKEY, nan), (_abi.LOSS_TUKEY, inf), (_abi.LOSS_TUKEY, 10.0, nan),
               (_abi.LOSS_GEMAN_MCCLURE, 0.0, 0.5), (_abi.LOSS_GEMAN_MCCLURE, -1.0, 0.5), (_abi.LOSS_GEMAN_MCCLURE, 10.0, nan), (_abi.LOSS_GEMAN_MCCLURE, 10.0, inf),
               (_abi.LOSS_GEMAN_MCCLURE, 10.0, 0.5, inf), (_abi.LOSS_HUBER, 0.0), (_abi.LOSS_SOFT_L1, -1.0)]
    for node in refused:
        prog, n = _abi.make_program([node])
        assert lib.gsfm_ba6_set_loss(h, prog, n) == _abi.ERR_INVALID_ARG, node
    prog, _ = _abi.make_program([(_abi.LOSS_TUKEY, 10.0), (_abi.LOSS_TUKEY, 10.0)])
    assert lib.gsfm_ba6_set_loss(h, prog, 2) == _abi.ERR_INVALID_ARG and lib.gsfm_ba6_set_loss(h, prog, -1) == _abi.ERR_INVALID_ARG and lib.gsfm_ba6_set_loss(h, None, 1) == _abi.ERR_INVALID_ARG
    assert not any(buf.raw)


@pytest.mark.skipif(have_gpu(), reason="CPU-only behaviour")
def test_fails_loudly_without_a_gpu():
    from globalsfmpy_amd.solver import FullBundleProblem, SolverError
    with pytest.raises(SolverError, match="status 2: no HIP device: gsfm_ba6_problem_create"):
        FullBundleProblem(np.ones((2, 3)), np.array([0, 2], np.uint64), np.array([0, 1], np.uint32), np.zeros((2, 2)))
