"""-m gpu: one Levenberg-Marquardt step of both full bundle adjustments (gsfm_ba6_step_check, gsfm_ba7_step_check) keeps the bytes of the
commit before the 6- and 7-coordinate solvers became one kernel family and one host template.

tests/golden/full_ba_step_parent_bytes.npz (tools/make_full_ba_parent_golden.py, recorded on an MI355X from a library built from that commit)
holds every output of step_check at the default options from the near starts of the step tests of test_gpu_ba6.py and test_gpu_ba7.py.  Scene
t under Tukey at radius 1e10 is the case that reaches the preconditioner's second tier (k_fba_cam_precond), which no solve golden does.  The
kernels use no atomics and are deterministic run to run, so the comparison is equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import make_full_ba_parent_golden as G  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "full_ba_step_parent_bytes.npz")


@pytest.mark.parametrize("case", sorted(G.STEP_CASES))
@pytest.mark.parametrize("solver", ["ba6", "ba7"])
def test_step_check_keeps_the_bytes_of_the_commit_before_the_shared_kernel_family(solver, case):
    gold = np.load(GOLD)
    got = G.step_case(solver, *G.STEP_CASES[case])
    print(solver, case, "PCG", list(got["info"]), "scalars", ["%.17g" % v for v in got["scal"]])
    assert sorted(got) == sorted(G.STEP_ARRAYS[solver] + ["scal", "info"])
    for key, value in got.items():
        want = gold["%s_%s_%s" % (solver, case, key)]
        assert value.shape == want.shape and value.tobytes() == want.tobytes(), key
