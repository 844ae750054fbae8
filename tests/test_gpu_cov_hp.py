"""-m gpu: the per-edge rotation covariance K7 (`k_cov_estimate`) against the high-precision reference (tests/cov_hp_reference.py),
with componentwise bounds in the style of test_gpu_positions_hp.py (u = 2^-53; each test asserts that its bounds bind: on its
well-conditioned cases, kappa_2(H_R) <= KAPPA_WELL, the median allowed relative error is at most 1e-11).  The reference is always
evaluated at the pose the device returned, so an error in the step is never blamed on the covariance.

  j (per match):  |dj| <= C_J u jscale,  jscale = |p1| |t| |p2| / sqrt(den) (1 + |t|^2 (|p1|^2 + |p2|^2) / (min f^2 den)) (2-norms):
                  the magnitude of num's terms (|R (t x p1)| <= |t| |p1|, Cauchy-Schwarz for the dot products) and of den's,
                  carried through the quotient (num's error reaches j through q = num / den times den's derivative terms).
                  C_J = 32: about 20 roundings from the pixel coordinates to a component of j (p = (x - u) / f, t x p1, R (.), the
                  dot products, 1 / sqrt(den), q, the J_l or chart product), each at most that scale, plus the few u of R and J_l,
                  rounded up to a power of two.
  H (5 x 5):      |dH| <= u (c_H M + C_J Mj),  M = sum |j||j|^T,  Mj = sum jscale (|j| 1^T + 1 |j|^T);  c_H = 4 + ceil(n / 64) + 6:
                  the product, the ceil(n / 64) serial additions of a lane and the 6 butterfly levels (Higham's recursive bound).
  C (3 x 3):      |C_dev - C*| <= |C*| dH_R |C*| / (1 - eta) + C_INV u kappa_2(H_R) max|C*|.  C_INV = 32: the cofactor inverse's
                  own rounding (a cofactor is two products and a difference, det three more terms) relative to max|C*| is at most
                  about 12 + 3 * 4 times kappa u, rounded up.
  LM step:        S, D^2, S H S, S g carry dH and dg = u (c_H G + C_J Gj) (G = sum |j||s|, Gj = sum jscale (|s| + |j|)) as in
                  test_gpu_positions_hp.py's dense step; y: 4 n u kappa_inf(K) |y*|_inf + |K^-1|_inf (|dK|_inf |y*|_inf + |db|_inf)
                  with n = 5; delta = S step: S |dy| + |delta| (sigma + u); the rotation adds u |rot|; the translation
                  0.6 |t| |d delta_t|_2 + C_PLUS u |t| (the chart's Lipschitz constant is |t| / 2 for |d| < 1, C_PLUS = 32 for
                  its Householder and sincos roundings).
The LM test's bounds bind only to ALLOW_MEDIAN_STEP = 1e-8 (measured: 2e-9 on the rotation, 2e-11 on the covariance at the returned
pose): the forward bound of the damped solve carries kappa_inf of the scaled 5 x 5 system.
Decisions are checked only where the reference's three have a margin: rel_dec >= 2e-3 or <= 0.5e-3, |cost change| >= 1e-5 cost,
the step >= 10 x the parameter tolerance.
"""
import math

import numpy as np
import pytest

from globalsfmpy_amd import covariance as cv

import cov_hp_reference as CR

pytestmark = pytest.mark.gpu

U = CR.U
LD = CR.LD
C_J = 32.0
C_INV = 32.0
C_PLUS = 32.0
ALLOW_MEDIAN = 1e-11
ALLOW_MEDIAN_STEP = 1e-8
KAPPA_WELL = 1e2
RANK_TOL = 1e-14


def c_h(n):
    return 4.0 + math.ceil(n / 64) + 6.0


def _device(edges, max_iterations):
    b = CR.batch(edges)
    return cv.estimate_rotation_covariances(b["match_ptr"], b["matches"], b["intrinsics"], b["rot"], b["trans"], max_iterations=max_iterations)


def _report(tag, worst, allow):
    print("%-34s %s | allowed rel. median %s" % (tag, " ".join("%s %.2e" % kv for kv in worst.items()),
                                                   " ".join("%s %.1e" % kv for kv in allow.items())))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, worst)
    loose = {k: a for k, a in allow.items() if not a <= ALLOW_MEDIAN}
    assert not loose, ("vacuous bound", tag, loose)


# ---- the cases of (a): one axis at a time around a generic edge --------------------------------------------------------------------
AXIS = np.array([0.48, -0.6, 0.64])
T_GEN = np.array([0.62, 0.3, -0.72])


def _fixed_pose_cases():
    cases = {}
    for n in (3, 5, 63, 64, 65, 127, 128, 129, 1000):
        cases["n%d" % n] = CR.make_edge(100 + n, n)
    m, K, r, t = CR.make_edge(5000, 331)   # 4096 matches: a cycle of 331 distinct ones (coprime with the 64 lanes)
    cases["n4096"] = (np.tile(m, (13, 1))[:4096], K, r, t)
    ang = {"rot0": 0.0, "rot1e-9": 1e-9, "rot3e-7": 3e-7, "rot9e-7": 9e-7, "rot0.99e-6": 0.99e-6, "rot2^-26-": 2.0 ** -26 * (1 - 2.0 ** -20),
           "rot2^-26+": 2.0 ** -26 * (1 + 2.0 ** -20), "rot0.1-": 0.1 * (1 - 1e-12), "rot0.1+": 0.1 * (1 + 1e-12), "rot1": 1.0,
           "rot_pi": math.pi - 1e-7}
    for k, th in ang.items():
        m, K, _, t = CR.make_edge(7, 40, rot=CR.aa(th, AXIS) if th else np.zeros(3), pose_noise=None)
        cases[k] = (m, K, CR.aa(th, AXIS) if th else np.zeros(3), t)
    for k, t in {"t+z": [0, 0, 1.0], "t-z": [0, 0, -1.0], "t1e-8+": [1e-8, 0, 1.0], "t1e-8-": [1e-8, 0, -1.0], "t2e-8+": [2e-8, 0, 1.0],
                 "t2e-8-": [2e-8, 0, -1.0]}.items():
        m, K, r, _ = CR.make_edge(8, 40, t=T_GEN, pose_noise=(0.01, 0.0))
        assert CR.branch_exact_agrees(t)
        cases[k] = (CR.make_edge(8, 40, t=t, pose_noise=None)[0], K, r, np.array(t))
    for k, tn in {"norm2^-30": 2.0 ** -30, "norm2^30": 2.0 ** 30}.items():
        cases[k] = CR.make_edge(9, 40, t=T_GEN / np.linalg.norm(T_GEN) * tn)
    cases["noise1e-6"] = CR.make_edge(10, 40, noise_px=1e-6)
    cases["noisefree_true"] = CR.make_edge(11, 40, rot=CR.aa(0.3, AXIS), t=T_GEN, noise_px=0.0, pose_noise=None)
    cases["f300"] = CR.make_edge(12, 40, f=(300.0, 300.0), pp=(800.0, 600.0, 780.0, 610.0))
    cases["f5000"] = CR.make_edge(13, 40, f=(5000.0, 5000.0), pp=(5000.0, 4000.0, 5100.0, 3900.0))
    # an exact zero residual: rot = 0, t = (1, 0, 0), a match with x1 = u1, y1 = v1, y2 = v2 (num == 0 exactly, den > 0)
    m, K, _, _ = CR.make_edge(14, 30, rot=np.zeros(3), t=np.array([1.0, 0, 0]), pose_noise=None)
    m[0] = [K[1], K[2], m[0, 2], K[5]]
    cases["zero_residual"] = (m, K, np.zeros(3), np.array([1.0, 0, 0]))
    return cases


@pytest.fixture(scope="module")
def fixed_pose():
    cases = _fixed_pose_cases()
    names = sorted(cases)
    edges = [cases[k] for k in names]
    dev = _device(edges, 0)
    ref = {k: CR.edge_data(*cases[k]) for k in names}
    return names, edges, dev, ref


def _check_cov(tag, names, dev, ref, idx, worst, allow_num, allow_den, kappa_well=KAPPA_WELL):
    for k, e in zip(names, idx):
        ed = ref[k]
        n = len(ed["s"])
        b = CR.cov_bound(ed, c_h(n), C_J, C_INV)
        if b is None:   # (only the rank test's ill-conditioned cases may get here: it checks their status and finiteness)
            assert tag.startswith("third_off"), tag
            assert np.all(np.isfinite(dev["cov"][e]))
            continue
        worst["C"] = max(worst.get("C", 0.0), CR.ratio(dev["cov"][e], ed["C"], b))
        if ed["kappa"] <= kappa_well:
            allow_num.append(np.asarray(b, float).ravel())
            allow_den.append(np.abs(np.asarray(ed["C"], float)).ravel())


def test_covariance_at_a_fixed_pose(fixed_pose):
    names, edges, dev, ref = fixed_pose
    for e, k in enumerate(names):
        assert dev["status"][e] == 0, (k, dev["status"][e], ref[k]["pivot_ratio"])
        assert dev["iterations"][e] == 0, k
        assert np.array_equal(dev["rotation"][e], edges[e][2]) and np.array_equal(dev["translation"][e], edges[e][3]), k
        assert ref[k]["pivot_ratio"] > 1e-13, k
    assert ref["zero_residual"]["s"][0] == 0 and np.all(np.isfinite(dev["cov"]))
    worst, num, den = {}, [], []
    per = {}
    for e, k in enumerate(names):
        w = {}
        _check_cov(k, [k], dev, ref, [e], w, num, den)
        per[k] = w["C"]
    for k in names:
        print("  %-16s kappa %.1e  ratio %.2e" % (k, ref[k]["kappa"], per[k]))
    worst["C"] = max(per.values())
    _report("fixed pose (%d edges)" % len(names), worst, {"C": CR.allowed_relative(np.concatenate(num), np.concatenate(den))})


# ---- (b) the rank rule --------------------------------------------------------------------------------------------------------------
def _rank_cases():
    m, K, r, t = CR.make_edge(21, 40)
    cases = {"generic": (m, K, r, t), "one_match": (m[:1], K, r, t), "two_matches": (m[:2], K, r, t),
             "identical": (np.tile(m[:1], (50, 1)), K, r, t)}
    d = np.array([0.6, -0.8, 0.3, 0.5])
    for eps in (1e-5, 1e-4, 1e-2, 3e-2, 0.1, 0.3):   # pivot ratio ~ 1.5e-10 eps^2 here
        cases["third_off_%.0e" % eps] = (np.vstack([m[:2], m[:1] + eps * d]), K, r, t)
    return cases


def test_rank_rule():
    cases = _rank_cases()
    names = sorted(cases)
    dev = _device([cases[k] for k in names], 0)
    worst, num, den = {}, [], []
    seen_ill = 0
    for e, k in enumerate(names):
        ed = CR.edge_data(*cases[k])
        pr = ed["pivot_ratio"]
        print("  %-16s pivot ratio %.3e  status %d" % (k, pr, dev["status"][e]))
        assert not (1e-15 <= pr <= 1e-13), (k, pr)   # either answer would do there
        assert dev["iterations"][e] == 0
        if pr < RANK_TOL:
            assert dev["status"][e] == 2, (k, pr)
            assert np.array_equal(dev["cov"][e], np.zeros((3, 3))), k
        else:
            assert dev["status"][e] == 0, (k, pr)
            _check_cov(k, [k], dev, {k: ed}, [e], worst, num, den, kappa_well=1e3 if k == "generic" else 0)
            seen_ill += 1e-12 <= pr <= 1e-6
    assert seen_ill >= 2
    for k in ("one_match", "two_matches", "identical"):
        assert dev["status"][names.index(k)] == 2, k
    _report("rank rule", worst, {"C": CR.allowed_relative(np.concatenate(num), np.concatenate(den))})


# ---- (c) one LM iteration -----------------------------------------------------------------------------------------------------------
def _lm_cases():
    t25 = T_GEN / np.linalg.norm(T_GEN) * 2.5
    return {
        "generic": CR.make_edge(31, 60, t=t25),
        "off0.3": (lambda e: (e[0], e[1], e[2] + CR.aa(0.3, [0.2, 1.0, -0.4]), e[3]))(CR.make_edge(32, 60, t=t25, pose_noise=None)),
        "pole+": CR.make_edge(33, 60, t=np.array([0, 0, 1.5]), pose_noise=(0.01, 0.0)),
        "pole-": CR.make_edge(34, 60, t=np.array([0, 0, -1.5]), pose_noise=(0.01, 0.0)),
        "pole1e-8+": CR.make_edge(35, 60, t=np.array([1e-8, 0, 1.5]), pose_noise=(0.01, 0.0)),
        "pole1e-8-": CR.make_edge(36, 60, t=np.array([1e-8, 0, -1.5]), pose_noise=(0.01, 0.0)),
        "rejected": (lambda e: (e[0], e[1], e[2] + CR.aa(1.5, [0, 0, 1.0]), e[3]))(CR.make_edge(37, 60, t=t25, pose_noise=None)),
    }


def _lm_bounds(ed, st, n, t):
    """bounds on delta (5) and on the candidate pose from the first-order perturbations of H and g"""
    ch = c_h(n)
    dH = CR.dH_bound(ed, ch, C_J)
    dg = U * (ch * ed["G"] + C_J * ed["Gj"])
    H = ed["H"]
    dgn = np.diagonal(H)
    sig = np.diagonal(dH) / (2 * dgn) + 3 * U
    S = st["S"]
    Hs = st["Hs"]
    dK = S[:, None] * dH * S[None, :] + np.abs(Hs) * (sig[:, None] + sig[None, :] + 3 * U)
    raw = np.diagonal(Hs)
    clamped = (raw <= 1e-6) | (raw >= 1e32)
    d2rel = np.where(clamped, 2 * U, 2 * sig + np.diagonal(dH) / dgn + 3 * U)
    dK = dK + np.diag(st["dd"] * d2rel)
    db = S * dg + np.abs(st["bs"]) * (sig + U)
    Kf = np.array(st["A"], float)
    Kinv = np.linalg.inv(Kf)
    kinv_inf = float(np.abs(Kinv).sum(axis=1).max()) * 1.01
    kappa = float(np.abs(Kf).sum(axis=1).max()) * kinv_inf
    yinf = float(np.abs(st["y"]).max())
    ey = 4 * 5 * U * kappa * yinf + kinv_inf * (float(np.asarray(dK, float).sum(axis=1).max()) * yinf + float(np.asarray(db, float).max()))
    dd = S * LD(ey) + np.abs(st["delta"]) * (sig + U)
    tn = float(np.linalg.norm(t))
    b_rot = dd[:3] + U * np.abs(st["crot"])
    b_t = np.full(3, 0.6 * tn * float(np.sqrt(np.sum(dd[3:] ** 2))) + C_PLUS * U * tn)
    return b_rot, b_t, dd


def test_one_lm_iteration():
    cases = _lm_cases()
    names = sorted(cases)
    edges = [cases[k] for k in names]
    dev = _device(edges, 1)
    worst, num, den, rn, rd = {}, [], [], [], []
    outcomes = {}
    for e, k in enumerate(names):
        m, K, r, t = edges[e]
        ed = CR.edge_data(m, K, r, t)
        st = CR.lm_step(m, K, r, t, ed)
        # the reference's decisions have a margin
        assert st["param_margin"] >= 10 and st["func_margin"] >= 10, (k, st["param_margin"], st["func_margin"])
        assert st["rel_dec_margin"] >= 2 or st["rel_dec_margin"] <= 0.5, (k, st["rel_dec_margin"])
        assert dev["iterations"][e] == 1, k
        outcomes[k] = st["accept"]
        if st["accept"]:
            b_rot, b_t, _ = _lm_bounds(ed, st, len(m), t)
            worst["rot"] = max(worst.get("rot", 0.0), CR.ratio(dev["rotation"][e], st["crot"], b_rot))
            worst["t"] = max(worst.get("t", 0.0), CR.ratio(dev["translation"][e], st["ct"], b_t))
            rn.append(np.asarray(b_rot, float))
            rd.append(np.abs(np.asarray(st["crot"], float)))
        else:
            assert np.array_equal(dev["rotation"][e], r) and np.array_equal(dev["translation"][e], t), k
        # the covariance at the pose the device returned
        ed2 = CR.edge_data(m, K, dev["rotation"][e], dev["translation"][e])
        assert dev["status"][e] == 0
        w = {}
        cn, cd = [], []
        _check_cov(k, [k], dev, {k: ed2}, [e], w, cn, cd)
        worst["C"] = max(worst.get("C", 0.0), w["C"])
        print("  %-12s accept %s  rel_dec %.3g  func %.3g  param %.3g  C %.2e" % (k, st["accept"], float(st["rel_dec"]), st["func_margin"],
                                                                             st["param_margin"], w["C"]))
        if cn:
            num += cn
            den += cd
    assert outcomes["rejected"] is False and all(v for k, v in outcomes.items() if k != "rejected"), outcomes
    allow = {"C": CR.allowed_relative(np.concatenate(num), np.concatenate(den)), "rot": CR.allowed_relative(np.concatenate(rn), np.concatenate(rd))}
    print("one LM iteration: allowed rel. median C %.1e rot %.1e" % (allow["C"], allow["rot"]))
    # the damped solve's forward bound carries kappa_inf(K) of the scaled 5 x 5 system: this test's bounds bind only to ALLOW_MEDIAN_STEP
    assert allow["C"] <= ALLOW_MEDIAN_STEP and allow["rot"] <= ALLOW_MEDIAN_STEP, allow
    _report("one LM iteration", worst, {})


# ---- (d) bit-exact properties -------------------------------------------------------------------------------------------------------
def _scaling_edges():
    out = [CR.make_edge(40 + s, 30 + 37 * s) for s in range(4)]
    for t in ([0, 0, 1.0], [0, 0, -1.0], [1e-8, 0, 1.0], [1e-8, 0, -1.0], [2e-8, 0, -1.0]):
        m, K, r, _ = CR.make_edge(50, 45, t=t)
        out.append((m, K, r, np.array(t)))
    return out


@pytest.mark.parametrize("k", [-40, -1, 1, 40])
def test_translation_scale_leaves_the_covariance_bit_identical(k):
    edges = _scaling_edges()
    base = _device(edges, 0)
    sc = _device([(m, K, r, np.ldexp(t, k)) for (m, K, r, t) in edges], 0)
    assert (base["status"] == 0).all()
    assert np.array_equal(sc["status"], base["status"])
    assert np.array_equal(sc["cov"], base["cov"])


@pytest.mark.parametrize("k", [-8, 8])
def test_pixel_scale_scales_the_covariance_exactly(k):
    edges = _scaling_edges()
    base = _device(edges, 0)
    sc = _device([(np.ldexp(m, k), np.ldexp(K, k), r, t) for (m, K, r, t) in edges], 0)
    assert (base["status"] == 0).all()
    assert np.array_equal(sc["status"], base["status"])
    assert np.array_equal(sc["cov"], np.ldexp(base["cov"], -2 * k))


def _isolation_edges(n):
    rng = np.random.default_rng(60)
    return [CR.make_edge(600 + e, int(rng.integers(5, 140))) for e in range(n)]


def _same(a, i, b, j):
    return all(np.array_equal(a[key][i], b[key][j]) for key in ("cov", "rotation", "translation", "status", "iterations"))


def test_batch_isolation():
    pool = _isolation_edges(257)
    alone = [_device([ed], 500) for ed in pool]
    m0, K0, r0, t0 = pool[0]
    nan_m = m0[:20].copy()
    nan_m[7, 2] = np.nan
    specials = [("zero_matches", (np.zeros((0, 4)), K0, r0, t0)), ("zero_t", (m0, K0, r0, np.zeros(3))), ("nan", (nan_m, K0, r0, t0))]
    for n in (1, 3, 4, 5, 257):
        edges = pool[:n]
        full = _device(edges, 500)
        rev = _device(edges[::-1], 500)
        mixed, where = [], []
        for e, ed in enumerate(edges):
            name, sp = specials[e % 3]
            mixed.append(sp)
            where.append(len(mixed))
            mixed.append(ed)
        mixed.append(specials[2][1])
        mix = _device(mixed, 500)
        for e in range(n):
            assert _same(full, e, alone[e], 0), (n, e)
            assert _same(rev, n - 1 - e, alone[e], 0), (n, e)
            assert _same(mix, where[e], alone[e], 0), (n, e)
        for s, ed in enumerate(mixed):
            if ed is specials[2][1]:
                assert mix["status"][s] == 2 and np.array_equal(mix["cov"][s], np.zeros((3, 3)))
                assert np.array_equal(mix["rotation"][s], r0) and np.array_equal(mix["translation"][s], t0)
            elif ed is specials[0][1] or ed is specials[1][1]:
                assert mix["status"][s] == 1 and np.array_equal(mix["cov"][s], np.zeros((3, 3)))
    assert all(a["status"][0] == 0 for a in alone)
