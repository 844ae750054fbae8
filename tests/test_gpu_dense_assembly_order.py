"""-m gpu: the exact step's dense assembly adds the entries of a repeated camera pair in CSR order, in one lane, and the step it
gives is the long-double solution of the damped system.

The last camera of a scene (its hub: the row of the lower-triangle cell) holds one pair measured four times, at row positions
10, 101, 200 and 231 -- three wavefronts of the row's workgroup, both orientations --, one of them weighted 1e4 (1e8 in the normal
matrix) and the others 1, so that the summation order changes the cell.  On the column-sorted layout filler edges among the
cameras below the pair's put the run at positions 510-513 of the row block: across the first sub-chunk boundary, i.e. into
another workgroup.  Two solves of one LM iteration must return the same bytes on the row-major, column-sorted and component paths
(all three take exact steps), and the step must meet a componentwise forward-error bound against the long-double solution.
"""
import numpy as np
import pytest

from globalsfmpy_amd import _abi
from globalsfmpy_amd.solver import RotationProblem

import hp_reference as H

pytestmark = pytest.mark.gpu

PAIR_POS = (10, 101, 200, 231)
PAIR_M = 7


def _scene(n, base, pad_to=None):
    """Hub = base + n - 1 with 240 entries; pair (hub, base + 7) at PAIR_POS of the hub's row; a chain through the rest.
    pad_to: add filler edges among cameras base + 1 .. base + 6 (and one to base + 8 for parity) until the sorted position of the
    pair's run in the row block is pad_to."""
    hub, m7 = base + n - 1, base + PAIR_M
    ei, ej = [], []
    for k in range(240):
        m = base + 1 + (k % (n - 2))
        if m == m7 and k not in PAIR_POS:
            m = base + 8
        if k in PAIR_POS:
            m = m7
        (ei.append(hub), ej.append(m)) if k % 2 else (ei.append(m), ej.append(hub))
    for c in range(base + 1, base + n - 2):
        ei.append(c); ej.append(c + 1)
    if pad_to is not None:
        def run_pos():   # entries of the block sorted by (camera, row): those with a camera below m7, then m7's with a row below the hub
            cams = [(j, i) for i, j in zip(ei, ej)] + [(i, j) for i, j in zip(ei, ej)]   # (camera, row)
            return sum(1 for cam, row in cams if cam < m7 or (cam == m7 and row < hub))
        p = run_pos()
        assert p <= pad_to, p
        if (pad_to - p) % 2:
            ei.append(base + 1); ej.append(base + 8)   # +1: (camera base+1, row base+8) precedes, (camera base+8, row base+1) follows
        k = 0
        while run_pos() < pad_to:
            a, b = 1 + k % 6, 1 + (k // 6 + k % 6 + 1) % 6
            if a != b:
                ei.append(base + a); ej.append(base + b)
            k += 1
        assert run_pos() == pad_to
    return ei, ej


def _problem(scenes, pad_to, rng):
    ei, ej, base = [], [], 0
    for n in scenes:
        a, b = _scene(n, base, pad_to if base == 0 else None)
        ei += a; ej += b; base += n
    N = base
    rot = rng.standard_normal((N, 3)) * 0.8
    rel = []
    for i, j in zip(ei, ej):   # consistent measurements plus 0.05 rad of noise: the first LM step is accepted
        q = H.q_mul(H.aa_to_q(rot[j]), H.q_conj(H.aa_to_q(rot[i])))
        rel.append([float(x) for x in H.q_log(q)] + rng.standard_normal(3) * 0.05)
    w = np.ones(len(ei))
    pair = [e for e in range(len(ei)) if {ei[e], ej[e]} == {scenes[0] - 1, PAIR_M}]
    assert len(pair) == 4
    w[pair[1]] = 1e4
    return N, np.array(ei), np.array(ej), np.array(rel), w, rot


def _step_reference(N, ei, ej, rel, w, rot, radius=1e4):
    """The first LM step in long double, as Ceres takes it: Jacobi scaling s = 1 / (1 + ||J_:k||), D = sqrt(clamp(diag(J_s^T J_s)) /
    radius), (J_s^T J_s + D^2) y = J_s^T r, delta = -s y.  Returns delta and its componentwise first-order error bound for a double
    evaluation: |d delta| <= s |A^-1| (E_A |y| + E_b), E_A = c u (|J_s|^T |J_s| + D^2) + (3n + 1) u sqrt(diag A) sqrt(diag A)^T
    (assembly, then the Cholesky factor's backward error, |L| |L^T| <= sqrt(a_ii a_jj)), E_b = c u |J_s|^T |r|."""
    ref = H.edge_set(_abi.ANGLE_AXIS_INLIERS, ei, ej, rel, rot, inlier_weight=w)
    lin = H.corrected(ref)
    J = H.normal_matrix(lin, N, ei, ej)
    Jabs = H.normal_matrix(lin, N, ei, ej, key="t_abs")
    n = 3 * N
    s = 1 / (1 + np.sqrt(np.diag(J)))
    As = J * s[:, None] * s[None, :]
    D2 = np.clip(np.diag(As), H.LD(1e-6), H.LD(1e32)) / H.LD(radius)
    A = As + np.diag(D2)
    A_g = H.assemble(lin, N, ei, ej)
    b = A_g["g"].reshape(-1) * s
    bm = (A_g["g_mag"].reshape(-1)) * s
    y = H.cholesky_solve(A, b)
    Ainv = H.cholesky_solve(A, np.eye(n, dtype=H.LD))
    deg = np.repeat(A_g["deg"], 3).astype(float)
    c = (16.0 + deg)
    d = np.sqrt(np.diag(A))
    E_A = c[:, None] * H.U * (Jabs * s[:, None] * s[None, :] + np.diag(D2)) + (3 * n + 1) * H.U * np.outer(d, d)
    E_b = c * H.U * bm
    dy = np.abs(Ainv) @ (E_A @ np.abs(y) + E_b)
    return -s * y, s * dy, float(np.linalg.cond(A.astype(float)))


@pytest.mark.parametrize("path", ["row_major", "colsort", "components"])
def test_repeated_pair_assembly_is_reproducible(monkeypatch, path):
    rng = np.random.default_rng(17)
    scenes = [120] if path != "components" else [120, 60, 40]
    if path == "colsort":
        monkeypatch.setenv("GSFM_K3_COLSORT", "1")
    N, ei, ej, rel, w, rot = _problem(scenes, 510 if path == "colsort" else None, rng)
    opts = dict(max_num_iterations=1, dense_cholesky_max_cams=120 if path == "components" else 512)
    outs = []
    for _ in range(2):
        dev = RotationProblem(N, ei, ej, rel, _abi.ANGLE_AXIS_INLIERS, inlier_weight=w)
        r, s = dev.solve(rot, **opts)
        assert s["num_dense_solves"] >= 1, s   # the exact step ran (on the component path: k_comp_assemble and the batch)
        outs.append(r.copy())
        dev.close()
    assert outs[0].tobytes() == outs[1].tobytes()
    delta, bound, kappa = _step_reference(N, ei, ej, rel, w, rot)
    delta_dev = outs[0].reshape(-1).astype(H.LD) - rot.reshape(-1).astype(H.LD)   # (exact in long double)
    bound = bound + H.U * np.abs(outs[0].reshape(-1))   # the rounding of x + delta
    q = H.ratio(delta_dev, delta, bound)
    print("%s: kappa(A) %.1e, step error / bound worst %.2e, allowed relative (median) %.1e"
          % (path, kappa, q, H.allowed_relative(bound, np.abs(delta))))
    assert q <= 1.0
