"""include/gsfm_rot_l1l2.h: every declared entry point is exported, the ctypes mirrors follow the header's structs field for field, the
defaults are those of Theia's RobustRotationEstimator::Options and L1Solver::Options, the header is C99 (the compiled program also checks
the mirrors' sizes against the C ones), and every refusal of the definition is returned with its message before any device call: on a
machine without a device a bad argument is reported as such, not as the missing device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import have_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "gsfm_rot_l1l2.h")).read()


def test_library_exports_every_declared_entry_point():
    from globalsfmpy_amd import _abi
    lib = _abi.load_library()
    txt = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    names = sorted(set(re.findall(r"\b(gsfm_rot_l1l2_[a-z0-9_]+)\s*\(", txt)))
    assert names == ["gsfm_rot_l1l2_abi_version", "gsfm_rot_l1l2_laplacian_solve", "gsfm_rot_l1l2_options_default", "gsfm_rot_l1l2_residuals",
                     "gsfm_rot_l1l2_solve"]
    for n in names:
        assert hasattr(lib, n), "libgsfm_rot.so does not export %s" % n
    assert lib.gsfm_rot_l1l2_abi_version() == 1 and "#define GSFM_ROT_L1L2_ABI_VERSION 1" in HDR


def _fields(struct_name, first):
    body = HDR[HDR.index("typedef struct {\n  int32_t %s;" % first):HDR.index("} %s;" % struct_name)]
    return re.findall(r"^\s+(?:int32_t|uint64_t|double)\s+(\w+)(?:\[\w+\])?;", body, flags=re.M)


def test_struct_mirrors_and_defaults():
    from globalsfmpy_amd import _abi
    lib = _abi.load_library()
    assert _fields("gsfm_rot_l1l2_options", "max_num_l1_iterations") == [n for n, _ in _abi.RotL1L2Options._fields_]
    assert _fields("gsfm_rot_l1l2_summary", "num_l1_iterations") == [n for n, _ in _abi.RotL1L2Summary._fields_]
    assert "#define GSFM_ROT_L1L2_MAX_L1 %d " % _abi.ROT_L1L2_MAX_L1 in HDR
    assert C.sizeof(_abi.RotL1L2Options) == 4 * 8 + 8 * 8 and C.sizeof(_abi.RotL1L2Summary) == 4 * 16 + 8 * 13
    o = _abi.RotL1L2Options()
    lib.gsfm_rot_l1l2_options_default(C.byref(o))
    # Theia: robust_rotation_estimator.h Options, l1_solver.h Options, SolveL1Regression's first max_num_iterations
    assert (o.max_num_l1_iterations, o.l1_step_convergence_threshold, o.max_num_irls_iterations, o.irls_step_convergence_threshold) == (5, 1e-3, 100, 1e-3)
    assert o.irls_loss_parameter_sigma == pytest.approx(np.radians(5.0), rel=1e-15)
    assert (o.admm_initial_iterations, o.admm_rho, o.admm_alpha, o.admm_absolute_tolerance, o.admm_relative_tolerance) == (5, 1.0, 1.0, 1e-4, 1e-2)
    assert (o.max_cg_iterations, o.cg_relative_tolerance, o.cg_check_interval, o.cg_stall_iterations, o.verbose) == (2000, 1e-14, 4, 200, 0)
    import robust_rotation_reference as ref
    for k, v in ref.DEFAULTS.items():
        assert getattr(o, k) == pytest.approx(v, rel=1e-15), k   # the restatement runs the library's defaults


def test_header_is_pedantic_c99_and_the_mirrors_have_the_c_sizes(tmp_path):
    from globalsfmpy_amd import _abi
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use_l1l2.c"
    src.write_text('#include <stddef.h>\n#include "gsfm_rot_l1l2.h"\nint main(void) { gsfm_rot_l1l2_options o; gsfm_rot_l1l2_options_default(&o);\n'
                   "  if (sizeof(gsfm_rot_l1l2_options) != %d || sizeof(gsfm_rot_l1l2_summary) != %d) return 2;\n"
                   "  if (offsetof(gsfm_rot_l1l2_summary, num_edges_used) != %d || offsetof(gsfm_rot_l1l2_options, cg_check_interval) != %d) return 3;\n"
                   "  return o.max_num_irls_iterations == 100 ? 0 : 1; }\n"
                   % (C.sizeof(_abi.RotL1L2Options), C.sizeof(_abi.RotL1L2Summary), _abi.RotL1L2Summary.num_edges_used.offset,
                      _abi.RotL1L2Options.cg_check_interval.offset))
    exe = str(tmp_path / "use_l1l2")
    lib_dir = os.path.join(ROOT, "globalsfmpy_amd")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + lib_dir,
                        "-lgsfm_rot", "-Wl,-rpath," + lib_dir, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([exe]).returncode == 0


def _solve(n, ei, ej, rel, rot, fixed=0):
    from globalsfmpy_amd import solver
    return solver.estimate_rotations_robust_l1l2(n, np.array(ei, np.uint32), np.array(ej, np.uint32), rel, rot, fixed)


def test_every_refusal_is_returned_before_any_device_call():
    from globalsfmpy_amd import solver
    rel, rot = np.zeros((2, 3)), np.zeros((5, 3))
    nan_rel = rel.copy(); nan_rel[1, 1] = np.nan
    inf_rot = rot.copy(); inf_rot[2, 0] = np.inf
    refusals = [
        ("joins camera 1 to itself", (5, [0, 1], [1, 1], rel, rot)),
        ("camera index >= n_cams", (2, [0, 1], [1, 2], rel, rot[:2])),
        ("edge 1 has a non-finite relative rotation", (5, [0, 1], [1, 2], nan_rel, rot)),
        ("camera 2 has an edge and a non-finite start rotation", (5, [0, 1], [1, 2], rel, inf_rot)),
        ("fixed_cam 3 appears in no edge", (5, [0, 1], [1, 2], rel, rot, 3)),
        ("fixed_cam must be a camera index", (5, [0, 1], [1, 2], rel, rot, 7)),
        ("camera 3 has an edge but is not connected to fixed_cam 0", (5, [0, 3], [1, 4], rel, rot)),
    ]
    for message, args in refusals:
        with pytest.raises(solver.SolverError, match="status 1: .*" + re.escape(message)):
            _solve(*args)
    # the Laplacian aid checks the graph the same way, and its weights
    with pytest.raises(solver.SolverError, match="status 1: .*not connected to fixed_cam"):
        solver.robust_l1l2_laplacian_solve(5, np.array([0, 3], np.uint32), np.array([1, 4], np.uint32), np.zeros((5, 3)))
    with pytest.raises(solver.SolverError, match="status 1: .*weight that is not positive"):
        solver.robust_l1l2_laplacian_solve(3, np.array([0, 1], np.uint32), np.array([1, 2], np.uint32), np.zeros((3, 3)), weights=[1.0, 0.0])
    with pytest.raises(solver.SolverError, match="status 1: .*joins camera"):
        solver.robust_l1l2_residuals(3, np.array([0, 1], np.uint32), np.array([1, 1], np.uint32), rel, rot[:3])
    with pytest.raises(TypeError, match="unknown option"):
        solver.estimate_rotations_robust_l1l2(3, [0, 1], [1, 2], rel, rot[:3], no_such_option=1)
    from globalsfmpy_amd import _abi
    lib = _abi.load_library()
    assert lib.gsfm_rot_l1l2_solve(3, 2, None, None, None, None, 0, None, None) == _abi.ERR_INVALID_ARG
    assert lib.gsfm_rot_l1l2_solve(3, 0, None, None, None, None, 0, None, None) == _abi.ERR_EMPTY


def test_a_start_rotation_that_is_not_finite_is_ignored_on_a_camera_without_an_edge():
    """... such a camera is not a parameter.  The call then gets as far as the device (or its absence)."""
    from globalsfmpy_amd import solver
    rot = np.zeros((4, 3)); rot[3] = np.nan
    if have_gpu():
        out, _ = _solve(4, [0, 1], [1, 2], np.zeros((2, 3)), rot)
        assert np.all(np.isnan(out[3])) and np.all(out[:3] == 0.0)
    else:
        with pytest.raises(solver.SolverError, match="no HIP device"):
            _solve(4, [0, 1], [1, 2], np.zeros((2, 3)), rot)


@pytest.mark.skipif(have_gpu(), reason="CPU-only behaviour")
def test_fails_loudly_without_a_gpu():
    from globalsfmpy_amd import solver
    with pytest.raises(solver.SolverError, match="no HIP device"):
        _solve(3, [0, 1], [1, 2], np.zeros((2, 3)), np.zeros((3, 3)))
