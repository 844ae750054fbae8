"""The exact step's dense tiled Cholesky (csrc/dense_kernels.hpp) against a high-precision reference, through gsfm_rot_dense_factor_check:
the launch sequence the LM step itself runs (solver_dense.hpp enqueue_chol_solve, solver_components.hpp enqueue_chol_batch) on a matrix of
the test's choosing.

The reference is plain numpy in long double (80-bit on x86) or exact small-integer arithmetic.  The assertions are the rigorous backward
error bounds of Cholesky (Higham, Accuracy and Stability of Numerical Algorithms, 10.1), not bit comparisons, so that a correct change of
summation order passes and a missing or misplaced update does not (u = 2^-53):
  * factor:  max |A - L L^T| <= 2 (n + 1) u max(|L| |L^T|)        (n <= 512: an O(n^3) long-double product)
  * solve:   ||b - A x||_inf <= 2 (3 n + 1) u || |L| |L^T| |x| ||_inf
  * forward: ||x - x*||_inf / ||x*||_inf <= 4 n u kappa_inf(A), x* by iterative refinement in long double.
Shapes: T = 1, 2, 3 block columns (the first launch, an even and an odd last launch), T = 9 (one backward group of 8 plus one), T = 48
(512 cameras), T = 64 / 65 (the fused schedule's limit), and one ~5 000-unknown matrix checked by its residual."""
import ctypes as C

import numpy as np
import pytest

from globalsfmpy_amd import _abi

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
GSFM_OK, GSFM_ERR_UNSUPPORTED = 0, 6
SINGLE, FUSED, BATCH = 0, 1, 2
SIZES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 96, 97, 255, 256, 257, 1023, 1536, 2047, 2048, 2049]
FUSED_MAX_N = 64 * 32


def factor(schedule, mats, rhs, active=None):
    """x, L (row-major lower factors), info per matrix; raises on any status but GSFM_OK."""
    lib = _abi.load_library()
    n = np.array([m.shape[0] for m in mats], dtype=np.uint32)
    A = np.ascontiguousarray(np.concatenate([np.ascontiguousarray(m, dtype=np.float64).ravel() for m in mats]))
    b = np.ascontiguousarray(np.concatenate([np.asarray(v, dtype=np.float64) for v in rhs]))
    x = np.full(b.size, 7.0)
    L = np.full(A.size, 7.0)
    info = np.full(len(mats), -7, dtype=np.int32)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    DP = C.POINTER(C.c_double)
    st = lib.gsfm_rot_dense_factor_check(schedule, len(mats), n.ctypes.data_as(C.POINTER(C.c_uint32)), A.ctypes.data_as(DP), b.ctypes.data_as(DP),
                                         None if act is None else act.ctypes.data_as(C.POINTER(C.c_int32)), x.ctypes.data_as(DP), L.ctypes.data_as(DP),
                                         info.ctypes.data_as(C.POINTER(C.c_int32)))
    if st != GSFM_OK:
        raise RuntimeError("gsfm_rot_dense_factor_check: %d %s" % (st, lib.gsfm_last_error().decode()))
    xs, Ls, o, oL = [], [], 0, 0
    for k in n.astype(np.int64):
        xs.append(x[o:o + k]); Ls.append(L[oL:oL + k * k].reshape(k, k)); o += k; oL += k * k
    return xs, Ls, info


def spd(n, kappa, rng):
    """Q diag(lambda) Q^T, eigenvalues geometric from 1 down to 1 / kappa, symmetric to the last bit."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, -np.log10(kappa), n) if n > 1 else np.ones(1)
    A = (Q * lam) @ Q.T
    return np.tril(A) + np.tril(A, -1).T


def block_laplacian(n_cams, kappa, rng):
    """A damped block Laplacian (x) I_3 in rotated camera frames -- the shape of the rotation problem's normal matrix: sum over edges of
    w [I, -R_ij; -R_ij^T, I] blocks -- with an absolute damping that sets kappa_2 ~ kappa."""
    edges = {(k - 1, k) for k in range(1, n_cams)}
    while len(edges) < min(4 * n_cams, n_cams * (n_cams - 1) // 2):
        i, j = sorted(rng.integers(0, n_cams, 2))
        if i != j:
            edges.add((int(i), int(j)))
    Lg = np.zeros((n_cams, n_cams))
    for i, j in edges:
        w = rng.uniform(0.5, 2.0)
        Lg[i, i] += w; Lg[j, j] += w; Lg[i, j] -= w; Lg[j, i] -= w
    R = np.linalg.qr(rng.standard_normal((n_cams, 3, 3)))[0]
    A = np.kron(Lg, np.eye(3))
    A = A.reshape(n_cams, 3, n_cams, 3)
    A = np.einsum("iab,ibjc,jdc->iajd", R, A, R, optimize=True).reshape(3 * n_cams, 3 * n_cams)
    A += np.eye(3 * n_cams) * (np.linalg.eigvalsh(Lg)[-1] / kappa)
    return np.tril(A) + np.tril(A, -1).T


def ld_matvec(A, x):
    return np.asarray(A, dtype=LD) @ np.asarray(x, dtype=LD)


def refined_solution(A, b, Ainv):
    """x* by iterative refinement: long-double residuals, float64 corrections, until the change stalls."""
    x = np.asarray(Ainv @ b, dtype=LD)
    bl = np.asarray(b, dtype=LD)
    for _ in range(30):
        r = bl - ld_matvec(A, x)
        d = Ainv @ np.asarray(r, dtype=np.float64)
        x = x + np.asarray(d, dtype=LD)
        if np.max(np.abs(d)) <= 1e-6 * U * float(np.max(np.abs(x))):
            break
    return x


def check_solution(A, b, x, L, kappa_inf=None, xstar=None, factor_error=True, tag=""):
    """The bounds above; returns the worst ratio of error to bound."""
    n = A.shape[0]
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(L)), tag
    absL = np.abs(L)
    ratios = {}
    if factor_error:
        LL = np.asarray(L, dtype=LD) @ np.asarray(L, dtype=LD).T
        err = float(np.max(np.abs(np.asarray(A, dtype=LD) - LL)))
        bound = 2 * (n + 1) * U * float(np.max(absL @ absL.T))
        ratios["factor"] = err / bound
    res = float(np.max(np.abs(np.asarray(b, dtype=LD) - ld_matvec(A, x))))
    bound = 2 * (3 * n + 1) * U * float(np.max(absL @ (absL.T @ np.abs(x))))
    ratios["solve"] = res / bound if bound > 0 else (0.0 if res == 0 else np.inf)
    if xstar is not None:
        fe = float(np.max(np.abs(np.asarray(x, dtype=LD) - xstar)) / np.max(np.abs(xstar)))
        ratios["forward"] = fe / (4 * n * U * kappa_inf)
    print("%s n=%d %s" % (tag, n, " ".join("%s %.2e" % kv for kv in ratios.items())))
    for k, v in ratios.items():
        assert v <= 1.0, "%s n=%d: %s error / bound = %.3e" % (tag, n, k, v)
    return ratios


@pytest.mark.parametrize("kappa", [1e1, 1e8, 1e13])
@pytest.mark.parametrize("n", SIZES)
def test_spd_factor_and_solve_within_the_backward_error_bounds(n, kappa):
    rng = np.random.default_rng(1000 * n + int(np.log10(kappa)))
    A = spd(n, kappa, rng)
    b = rng.standard_normal(n)
    Ainv = np.linalg.inv(A)
    kinf = np.max(np.abs(A).sum(1)) * np.max(np.abs(Ainv).sum(1))
    xstar = refined_solution(A, b, Ainv)
    for schedule in (SINGLE, FUSED):
        if schedule == FUSED and n > FUSED_MAX_N:
            continue
        (x,), (L,), info = factor(schedule, [A], [b])
        assert info[0] == 0, (schedule, info)
        check_solution(A, b, x, L, kinf, xstar, factor_error=n <= 512, tag="spd kappa=%.0e schedule=%d" % (kappa, schedule))


@pytest.mark.parametrize("n_cams", [2, 11, 21, 32, 85, 341, 512, 683])
def test_damped_block_laplacian_within_the_bounds(n_cams):
    """The normal matrix's own shape (3 x 3 blocks of rotated Laplacian weights) at kappa ~ 1e10."""
    rng = np.random.default_rng(77 + n_cams)
    A = block_laplacian(n_cams, 1e10, rng)
    n = A.shape[0]
    b = rng.standard_normal(n)
    Ainv = np.linalg.inv(A)
    kinf = np.max(np.abs(A).sum(1)) * np.max(np.abs(Ainv).sum(1))
    xstar = refined_solution(A, b, Ainv)
    for schedule in (SINGLE, FUSED):
        if schedule == FUSED and n > FUSED_MAX_N:
            continue
        (x,), (L,), info = factor(schedule, [A], [b])
        assert info[0] == 0
        check_solution(A, b, x, L, kinf, xstar, factor_error=n <= 512, tag="laplacian schedule=%d" % schedule)


def test_largest_supported_size_by_residual():
    """~5 000 unknowns (T = 157) on the default schedule, checked by the solve's backward error.  (One past each schedule's limit is refused
    before any device call: tests/test_comp_rest.py.)"""
    rng = np.random.default_rng(5)
    n_cams = 1666
    A = block_laplacian(n_cams, 1e8, rng)
    b = rng.standard_normal(A.shape[0])
    (x,), (L,), info = factor(SINGLE, [A], [b])
    assert info[0] == 0
    check_solution(A, b, x, L, factor_error=False, tag="large")


def indefinite(n, p, rng, band=3):
    """A = L D L^T, L unit lower banded with entries in {-1, 0, 1}, D = 4 except D_p = -4: small integers, exact in fp64, and every pivot of
    the factorisation up to p is exact (the factor's entries are 0, +-1, +-2), so pivot p is exactly -4: nothing but a wrong pivot index
    can give another status."""
    L = np.eye(n)
    for i in range(n):
        for j in range(max(0, i - band), i):
            L[i, j] = rng.integers(-1, 2)
    d = np.full(n, 4.0)
    d[p] = -4.0
    return (L * d) @ L.T


# (n, p): the first pivots, both sides of the tile boundaries 32 and 64, and the last pivot for an odd (T = 3) and an even (T = 4) count
INDEFINITE = [(97, 0), (97, 1), (97, 31), (97, 32), (97, 33), (97, 63), (97, 64), (65, 64), (97, 96), (128, 127)]


@pytest.mark.parametrize("n,p", INDEFINITE)
def test_exactly_indefinite_matrix_reports_its_pivot(n, p):
    rng = np.random.default_rng(n * 131 + p)
    A = indefinite(n, p, rng)
    b = rng.standard_normal(n)
    for schedule in (SINGLE, FUSED, BATCH):
        _, _, info = factor(schedule, [A], [b])
        assert info[0] == 1 + p, (schedule, n, p, info)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("n,p", [(97, 0), (97, 33), (97, 64), (65, 64), (96, 95), (128, 127)])
def test_non_finite_diagonal_reports_its_pivot(n, p, bad):
    """A NaN or an inf on the diagonal at p: the status names pivot p (an infinite pivot is no positive one either: its column turns to NaN,
    and where it is the last pivot of a full tile nothing after it would report)."""
    rng = np.random.default_rng(n + p)
    A = spd(n, 1e1, rng)
    A[p, p] = bad
    b = rng.standard_normal(n)
    for schedule in (SINGLE, FUSED, BATCH):
        _, _, info = factor(schedule, [A], [b])
        assert info[0] != 0 and info[0] == 1 + p, (schedule, n, p, bad, info)


def test_batch_matches_the_single_schedule_and_isolates_failures():
    """Items of 3, 96, 97, 700 and 1536 unknowns side by side (Tmax = 48: the short items sit out the late launches), one exactly indefinite
    item and one inactive one.  Every active SPD item gives the single schedule's x, L and status bit for bit (the same kernel body on the
    same tiles with the same arguments); the indefinite item reports its own pivot and leaves the others untouched; the inactive item is
    left alone (x = 0, status 0)."""
    rng = np.random.default_rng(2024)
    sizes = [3, 96, 97, 700, 1536]
    mats = [spd(k, 1e8, rng) for k in sizes]
    rhs = [rng.standard_normal(k) for k in sizes]
    p_bad = 40
    mats.insert(2, indefinite(99, p_bad, rng)); rhs.insert(2, rng.standard_normal(99))
    mats.append(spd(64, 1e1, rng)); rhs.append(rng.standard_normal(64))
    active = [1] * (len(mats) - 1) + [0]
    xs, Ls, info = factor(BATCH, mats, rhs, active)
    assert list(info) == [0, 0, 1 + p_bad, 0, 0, 0, 0], info
    assert np.all(xs[-1] == 0.0) and np.all(Ls[-1] == 0.0)
    for k, (A, b) in enumerate(zip(mats[:-1], rhs[:-1])):
        if k == 2:
            continue
        (x1,), (L1,), info1 = factor(SINGLE, [A], [b])
        assert info1[0] == 0
        assert np.array_equal(xs[k].view(np.uint64), x1.view(np.uint64)), "item %d: x differs from the single schedule" % k
        assert np.array_equal(Ls[k].view(np.uint64), L1.view(np.uint64)), "item %d: L differs from the single schedule" % k
        check_solution(A, b, xs[k], Ls[k], factor_error=A.shape[0] <= 512, tag="batch item %d" % k)
    # the same batch without the bad item: every other item's results are the same bits
    keep = [k for k in range(len(mats)) if k != 2]
    xs2, Ls2, info2 = factor(BATCH, [mats[k] for k in keep], [rhs[k] for k in keep], [active[k] for k in keep])
    assert not np.any(info2)
    for j, k in enumerate(keep):
        assert np.array_equal(xs2[j].view(np.uint64), xs[k].view(np.uint64))
        assert np.array_equal(Ls2[j].view(np.uint64), Ls[k].view(np.uint64))
