"""-m gpu: the position kernels and one position LM step against the high-precision reference (tests/position_hp_reference.py), at the
branch points of the residual and the rotation and at the row structures of the kernels, with componentwise bounds in the style of
test_gpu_hp_linearization.py (u = 2^-53, no maximum over an array in a componentwise bound; each test also asserts that its bounds bind:
the median allowed relative error is at most 1e-11).

  residual r:   |r_dev - r*| <= C0 u e_mag,  e_mag = 1 + |t| (position_hp_reference: w is one correctly rounded subtraction)
  rho, cost:    C0 u (scale(rho) + rho' sbound),  the cost with C0 + E (its sum)
  g, D_k, L v:  c_k u (first-order magnitude sums of hp_reference.assemble / matvec),  c_k = CA + deg(k)
  K entries:    c u S_r S_c |L|_rc (+ the relative error of S_r, S_c and of D^2),  c = C0 + deg(r) + deg(c); inactive rows exact
  b = S g:      c_k u S |g| + |b| (sigma + u)
  y (dense):    4 n u kappa_inf(K) |y*|_inf + |K^-1|_inf (|dK|_inf |y*|_inf + |db|_inf)   (test_gpu_dense_factor.py's forward bound plus
                the assembly's perturbation dK, db: the bounds above)
  delta:        the bound on y carried through S (the projection is orthogonal, so it does not grow an error)
  model change: |d delta|_2 (|g|_2 + |L|_2 |delta|_2) + c u (|delta|.|g| + |delta|^T |L| |delta|)
  PCG:          the true preconditioned relative residual of the device's y, in long double from K*, is at most cg_relative_tolerance plus
                the attainable-accuracy floor c u | |K||y| + |b| |_M^-1 / |b|_M^-1 plus the assembly's perturbation in the same norm.
At the rotation's small-angle switch the device's d must be within half an ULP plus u |t| / 10 of the exact R^T t (read from the n = 0
edges, where r = -d to the bit; t along y, the axis along x): cos and sin of theta ~ 1.5e-8 are exact to well below that, and Ceres'
first-order form, taken one ULP past the switch, is u |t| off in the y component.
"""
import numpy as np
import pytest

from globalsfmpy_amd import loss_functions as LF
from globalsfmpy_amd.solver import PositionProblem

import hp_reference as H
import position_hp_reference as PH

pytestmark = pytest.mark.gpu

U = H.U
LD = H.LD
C0 = 64.0
CA = 16.0
ALLOW_MEDIAN = 1e-11
EPS = np.finfo(np.float64).eps

LOSSES = {
    "none": (None, None, ()),
    "huber": (LF.HuberLoss(0.1), "huber", (0.1,)),
    "softl1": (LF.SoftLOneLoss(0.1), "softl1", (0.1,)),
    "cauchy": (LF.CauchyLoss(0.1), "cauchy", (0.1,)),
    "tukey": (LF.TukeyLoss(0.5), "tukey", (0.5,)),
    "geman_mcclure": (LF.GemanMcClureLoss(0.3, 0.5), "geman_mcclure", (0.3, 0.5)),
    "tolerant": (LF.TolerantLoss(0.05, 0.1), "tolerant", (0.05, 0.1)),
    "scaled_huber": (LF.ScaledLoss(LF.HuberLoss(0.1), 2.5), "scaled", (("huber", (0.1,)), 2.5)),
}
KNEES = {"huber": 0.01, "scaled_huber": 0.01, "tukey": 0.25}


class PyTolerant(object):
    """Tolerant through the host callback (no native_program): rho'' > 0, the Corrector's alpha branch on the POS_LM_EXT path"""

    def __init__(self, a, b):
        self.inner = LF.TolerantLoss(a, b)

    def Evaluate(self, s, out):
        self.inner.Evaluate(s, out)


def _aa(theta, axis):
    axis = np.asarray(axis, float)
    return theta * axis / np.linalg.norm(axis)


def _rot(v):
    from globalsfmpy_amd.synth import aa_to_matrix
    return aa_to_matrix(np.asarray(v, float)[None])[0]


# ---- graphs ---------------------------------------------------------------------------------------------------------------------
class Builder(object):
    def __init__(self, n, rng):
        self.n, self.rng = n, rng
        self.pos = rng.uniform(-1, 1, (n, 3))
        self.rot = np.array([_aa(rng.uniform(0.2, 2.8), rng.standard_normal(3)) for _ in range(n)])
        self.ei, self.ej, self.t = [], [], []

    def add(self, i, j, t=None, outlier=None, mag=1.0):
        if t is None:
            rng = self.rng
            if outlier is None:
                outlier = rng.uniform() < 0.3
            w = self.pos[j] - self.pos[i]
            d = rng.standard_normal(3) if outlier else w / np.linalg.norm(w) + rng.normal(scale=0.02, size=3)
            d = d / np.linalg.norm(d) * mag
            t = _rot(self.rot[i]) @ d   # R_i d, so that R_i^T t = d
        self.ei.append(i)
        self.ej.append(j)
        self.t.append(np.asarray(t, float))

    def graph(self, fixed):
        return {"n_cams": self.n, "edge_i": np.array(self.ei, np.uint32), "edge_j": np.array(self.ej, np.uint32), "rel_t": np.array(self.t),
                "rot_aa": self.rot.copy(), "pos": self.pos.copy(), "fixed": fixed}


def branch_graph(seed=21):
    """341 cameras (N = 1 mod 4): rotations at the small-angle switch, near pi and 2 pi and beyond; |t| in {0, 1e-8, 1, 1e3}; pairs at
    n = 0, 1e-13, 1e-12 (1 -+ 1e-6), 1e-11 and at |c| ~ 1e8 with n ~ 1e-3; an edge with r = 0 exactly; hub rows of degree 63, 64, 65, 128
    and 300; isolated cameras; repeated pairs in both orientations; the fixed camera in the middle, adjacent to a hub."""
    rng = np.random.default_rng(seed)
    n = 341
    b = Builder(n, rng)
    isolated = {n - 1, n - 6, n - 11}
    fixed = n // 2
    special = set(isolated) | {fixed}
    # rotations at the small-angle switch (axis x, t along y: R^T t's y component is cos(theta) |t|) and beyond
    th_eps = [(np.sqrt(EPS * (1 + 1e-6)), 0, 0), (np.sqrt(EPS * (1 - 1e-6)), 0, 0), (2.0 ** -26, 2.0 ** -52, 0), (2.0 ** -26, 0, 0),
              (1e-10, 0, 0), (0.0, 0.0, 0.0)]
    big = [_aa(np.pi - 1e-6, rng.standard_normal(3)), _aa(np.pi + 1e-6, rng.standard_normal(3)), _aa(2 * np.pi - 1e-3, rng.standard_normal(3)),
           _aa(10.0, rng.standard_normal(3))]
    sw_cams = list(range(10, 10 + len(th_eps) + len(big)))
    twins = [c + 20 for c in sw_cams]
    for c, w in zip(sw_cams, th_eps + big):
        b.rot[c] = w
    switch_edges = []
    for c, tw in zip(sw_cams, twins):
        b.pos[tw] = b.pos[c]   # n = 0: r = -d to the bit
        for mag in (1.0, 1e3, 1e-8, 0.0):
            if np.linalg.norm(b.rot[c]) < 1e-6:
                t = np.array([0.0, mag, 0.0])
                switch_edges.append(len(b.ei))
            else:
                t = rng.standard_normal(3)
                t *= mag / np.linalg.norm(t)
            b.add(c, tw, t)
        b.add(c, 200 + (c % 50), mag=1e3)
        b.add(c, 150 + (c % 50))
    special |= set(sw_cams) | set(twins)
    # pairs about the guard n < 1e-12 (near the origin, so that c_i + n u is exact to 1e-9 of n)
    base = 60
    for k, nn in enumerate((1e-13, 1e-12 * (1 - 1e-6), 1e-12 * (1 + 1e-6), 1e-11)):
        i, j = base + 2 * k, base + 2 * k + 1
        b.pos[i] = np.array([1.0, -2.0, 0.5]) * 1e-6 * (k + 1)
        u = rng.standard_normal(3)
        b.pos[j] = b.pos[i] + nn * u / np.linalg.norm(u)
        b.add(i, j)
        b.add(j, i, mag=0.0)
        b.add(i, 100 + k)
        special |= {i, j}
    # |c| ~ 1e8 and n ~ 1e-3
    far = rng.standard_normal(3)
    far *= 1e8 / np.linalg.norm(far)
    for k in range(3):
        b.pos[70 + k] = far + rng.uniform(-1e-3, 1e-3, 3)
    b.add(70, 71); b.add(71, 72); b.add(72, 70, outlier=True); b.add(70, 110)
    special |= {70, 71, 72}
    # r = 0 exactly: rot 0, c_j - c_i = (0, 2, 0), t = (0, 1, 0)
    b.rot[80] = 0.0
    b.pos[80] = [0.5, 0.25, 0.125]
    b.pos[81] = [0.5, 2.25, 0.125]
    b.add(80, 81, [0.0, 1.0, 0.0])
    special |= {80, 81}
    # repeated pairs in both orientations
    b.add(90, 91); b.add(91, 90); b.add(90, 91)
    hubs = {0: 300, 1: 63, 2: 64, 3: 65, 4: 128}   # (total degrees: hubs 1 and 2 also reach the fixed camera)
    live = [c for c in range(n) if c not in special and c not in hubs]
    for hub, deg in hubs.items():
        for k in range(deg - (1 if hub in (1, 2) else 0)):
            m = live[(k * 7 + hub) % len(live)]
            b.add(hub, m) if k % 2 else b.add(m, hub)
    b.add(fixed, 1)
    b.add(2, fixed)
    # a ring through the rest, with |t| in {1, 1e3, 1e-8, 0}
    ring = [c for c in range(n) if c not in isolated and c not in hubs]
    for k, c in enumerate(ring):
        b.add(c, ring[(k + 1) % len(ring)], mag=(1.0, 1e3, 1e-8, 0.0, 1.0, 1.0)[k % 6])
    g = b.graph(fixed)
    deg = np.bincount(g["edge_i"], minlength=n) + np.bincount(g["edge_j"], minlength=n)
    assert [deg[h] for h in sorted(hubs)] == [hubs[h] for h in sorted(hubs)] and deg[list(isolated)].sum() == 0
    g["switch_edges"] = np.array(switch_edges)
    g["isolated"] = sorted(isolated)
    g["guard_pairs"] = [(base + 2 * k, base + 2 * k + 1) for k in range(4)]
    return g


def small_graph(n, seed, hub_deg=20, tukey_outlier_cam=False):
    """n cameras: a chain plus random edges (about 4 n), a hub next to the fixed camera n // 2, a repeated pair (i, j), (j, i), (i, j), one
    isolated camera (n > 10); tukey_outlier_cam: camera 1's edges are all far beyond the Tukey cut (its diagonal is 0)."""
    rng = np.random.default_rng(seed)
    b = Builder(n, rng)
    iso = n - 2 if n > 10 else -1
    cams = [c for c in range(n) if c != iso]
    for k in range(len(cams) - 1):
        b.add(cams[k], cams[k + 1])
    for _ in range(3 * n):
        i, j = rng.choice(cams, 2, replace=False)
        b.add(int(i), int(j))
    fixed = n // 2
    hub = fixed + 1
    for k in range(min(hub_deg, len(cams) - 2)):
        m = cams[(k * 5 + 3) % len(cams)]
        if m != hub:
            b.add(hub, m)
    b.add(0, n - 1); b.add(n - 1, 0); b.add(0, n - 1)
    if tukey_outlier_cam:
        keep = [e for e in range(len(b.ei)) if 1 not in (b.ei[e], b.ej[e])]
        b.ei = [b.ei[e] for e in keep]; b.ej = [b.ej[e] for e in keep]; b.t = [b.t[e] for e in keep]
        for m in (0, 2, 3):
            b.add(1, m, t=-_rot(b.rot[1]) @ ((b.pos[m] - b.pos[1]) / np.linalg.norm(b.pos[m] - b.pos[1])))   # d = -u: s = 4
    return b.graph(fixed)


# ---- references (cached per graph) ------------------------------------------------------------------------------------------------
_T1 = {}


def tier1(key, g):
    if key not in _T1:
        _T1[key] = PH.edge_set(g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"], g["pos"])
    return _T1[key]


@pytest.fixture(scope="module")
def bgraph():
    return branch_graph()


def _device(g, lname, callback=False):
    dev = PositionProblem(g["n_cams"], g["edge_i"], g["edge_j"], g["rel_t"], g["rot_aa"])
    if callback:
        dev.set_loss_callback(PyTolerant(0.05, 0.1).Evaluate)
    else:
        dev.set_loss(LOSSES[lname][0])
    return dev


def _present(g):
    p = np.zeros(g["n_cams"], bool)
    p[g["edge_i"]] = True
    p[g["edge_j"]] = True
    return p


def _knee_clear(lin, lname):
    if lname in KNEES:
        a2 = KNEES[lname]
        s = lin["s"].astype(float)
        assert np.all(np.abs(s - a2) > 1e-9 * a2), lname


def _report(tag, worst, allow):
    print("%-34s %s | allowed rel. median %s" % (tag, " ".join("%s %.2e" % kv for kv in worst.items()),
                                                   " ".join("%s %.1e" % kv for kv in allow.items())))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (tag, worst)
    loose = {k: a for k, a in allow.items() if not a <= ALLOW_MEDIAN}
    assert not loose, ("vacuous bound", tag, loose)


# ---- 1. residuals, rho, cost, g, D, L v on the branch graph ------------------------------------------------------------------------
@pytest.mark.parametrize("lname", sorted(LOSSES) + ["tolerant_callback"])
def test_linearisation_against_hp_reference(bgraph, lname):
    g = bgraph
    callback = lname == "tolerant_callback"
    kind, params = LOSSES["tolerant" if callback else lname][1:]
    ref = tier1("branch", g)
    lin = PH.corrected(ref, kind, params)
    _knee_clear(lin, lname)
    n, ei, ej = g["n_cams"], g["edge_i"], g["edge_j"]
    if lname == "tolerant":
        assert np.sum(lin["rho"][2] > 0) > len(ei) // 4   # the Corrector's alpha branch runs on many edges
    dev = _device(g, lname, callback)
    r_dev, rho_dev = dev.residuals(g["pos"])
    emag = ref["e_mag"]
    worst = {"r": H.ratio(r_dev, ref["r"], C0 * U * emag)}
    sb = C0 * U * (lin["s"] + 2 * (np.abs(ref["r"]) * emag).sum(axis=1)) + ((C0 * U * emag) ** 2).sum(axis=1)
    rho0, rho1, rho2 = lin["rho"]
    worst["rho"] = H.ratio(rho_dev, rho0, C0 * U * lin["rho_scale"] + rho1 * sb)
    ld = dev.linearize(g["pos"])
    worst["cost"] = H.ratio(ld["cost"], LD(0.5) * rho0.sum(), 0.5 * ((C0 + len(ei)) * U * lin["rho_scale"] + rho1 * sb).sum())
    A = H.assemble(lin, n, ei, ej)
    ck = H.c_row(A["deg"], CA)
    bounds = {"g": (ck[:, None] * U * A["g_mag"], A["g_true"]), "D": (ck[:, None, None] * U * A["D_mag"], A["D_true"])}
    worst["g"] = H.ratio(ld["gradient"], A["g"], bounds["g"][0])
    worst["D"] = H.ratio(ld["diag_blocks"], A["D"], bounds["D"][0])
    iso = np.array(g["isolated"])
    assert np.all(ld["gradient"][iso] == 0) and np.all(ld["diag_blocks"][iso] == 0)
    rng = np.random.default_rng(3)
    for name, v in (("Lv_unit", np.eye(3)[np.arange(n) % 3]), ("Lv_rand", rng.standard_normal((n, 3)))):
        y, ym, yt = H.matvec(lin, n, ei, ej, v)
        bounds[name] = (ck[:, None] * U * ym, yt)
        yd = dev.normal_matvec(v)
        worst[name] = H.ratio(yd, y, bounds[name][0])
        assert np.all(yd[iso] == 0.0)
    # the fixed camera inactive (after a step check): its row is 0, its v still enters its neighbours' rows
    fixed = g["fixed"]
    dev.step_check(g["pos"], fixed_cam=fixed, radius=1e4, want_K=False, dense_max_cams=0, max_cg_iterations=1)
    v = rng.standard_normal((n, 3))
    v[fixed] = [1e3, -2e3, 5e2]
    y, ym, yt = H.matvec(lin, n, ei, ej, v)
    yd = dev.normal_matvec(v)
    assert np.all(yd[fixed] == 0.0) and np.all(yd[iso] == 0.0)
    act = _present(g)
    act[fixed] = False
    bounds["Lv_fixed"] = ((ck[:, None] * U * ym)[act], yt[act])
    worst["Lv_fixed"] = H.ratio(yd[act], y[act], bounds["Lv_fixed"][0])
    dev.close()
    allow = {k: H.allowed_relative(b, t) for k, (b, t) in bounds.items()}
    _report("linearisation " + lname, worst, allow)


def test_directions_at_the_small_angle_switch(bgraph):
    """r = -d to the bit on the n = 0 edges: the full rotation must be taken for theta^2 > DBL_EPSILON and be exact to half an ULP plus
    u |t| / 10 there (the first-order form is u |t| off one ULP past the switch); at or below the switch Ceres' first-order form is the rule: within
    theta^2 / 2 |t| + 4 u |t| of the exact d."""
    g = bgraph
    ref = tier1("branch", g)
    dev = _device(g, "none")
    r_dev, _ = dev.residuals(g["pos"])
    dev.close()
    worst = 0.0
    for e in g["switch_edges"]:
        i = g["edge_i"][e]
        th2 = float(np.sum(g["rot_aa"][i] ** 2))
        tn = float(np.linalg.norm(g["rel_t"][e]))
        assert not ref["unit"][e]
        err = np.abs(-r_dev[e].astype(LD) - ref["d"][e])
        if th2 > EPS:   # half an ULP of each component (the product with |t| rounds) plus u |t| / 10
            bound = 0.5 * np.spacing(np.abs(ref["d"][e].astype(float))) + 0.1 * U * tn
        else:
            bound = np.full(3, (th2 / 2 + 4 * U) * tn)
        if tn == 0:
            assert np.all(err == 0), e
            continue
        worst = max(worst, float((err / bound).max()))
    print("small-angle switch: worst ratio %.2e" % worst)
    assert worst <= 1.0


def test_guard_pairs_take_the_guard_on_the_exact_side(bgraph):
    g = bgraph
    ref = tier1("branch", g)
    for (i, j), unit in zip(g["guard_pairs"], (False, False, True, True)):
        e = [k for k in range(len(g["edge_i"])) if (g["edge_i"][k], g["edge_j"][k]) == (i, j)][0]
        n = float(ref["n"][e]) if ref["unit"][e] else float(np.linalg.norm(g["pos"][j] - g["pos"][i]))
        assert ref["unit"][e] == unit
        assert abs(n / 1e-12 - 1) >= 1e-9


# ---- 2. the dense step ------------------------------------------------------------------------------------------------------------
def _bounds_K(sysm, lin, A, g, act_cam, ck_cam, radius, min_diag, max_diag):
    """componentwise bounds of K, b and the relative error of S"""
    n = 3 * g["n_cams"]
    lin_m = dict(lin)
    lin_m["Jitm"] = lin["Jit_abs"] + lin["Jit_err"]
    lin_m["Jjtm"] = lin["Jjt_abs"] + lin["Jjt_err"]
    Lmag = H.normal_matrix(lin_m, g["n_cams"], g["edge_i"], g["edge_j"], key="tm")
    deg = np.repeat(A["deg"], 3).astype(float)
    Dmag = np.diagonal(Lmag)
    dg = sysm["diagL"]
    cr = np.repeat(ck_cam, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        sig = np.where(dg > 0, cr * U * Dmag / (2 * np.where(dg > 0, dg, 1)), 0) + 3 * U
    S = sysm["S"]
    cmat = C0 + deg[:, None] + deg[None, :]
    Kb = cmat * U * S[:, None] * Lmag * S[None, :] + np.abs(sysm["K"]) * (sig[:, None] + sig[None, :] + 3 * U)
    raw = S * S * dg
    clamped = (raw <= min_diag) | (raw >= max_diag)
    with np.errstate(divide="ignore", invalid="ignore"):
        d2rel = np.where(clamped, 2 * U, 2 * sig + np.where(dg > 0, cr * U * Dmag / np.where(dg > 0, dg, 1), 0) + 3 * U)
    Kb[np.arange(n), np.arange(n)] += sysm["D2"] * d2rel
    act = sysm["act"]
    Kb[~act, :] = 0
    Kb[:, ~act] = 0
    gmag = A["g_mag"].reshape(n)
    bb = np.where(act, cr * U * S * gmag + np.abs(sysm["b"]) * (sig + U), 0)
    Ktrue = S[:, None] * H.normal_matrix(lin, g["n_cams"], g["edge_i"], g["edge_j"], key="t_abs") * S[None, :]
    return Kb, bb, sig, Lmag, Ktrue, clamped


def _step_reference(g, key, lname, radius, min_diag=1e-6, max_diag=1e32):
    kind, params = LOSSES[lname][1:]
    lin = PH.corrected(tier1(key, g), kind, params)
    _knee_clear(lin, lname)
    act = _present(g)
    act[g["fixed"]] = False
    sysm = PH.step_system(lin, g["n_cams"], g["edge_i"], g["edge_j"], act, radius, min_diag, max_diag)
    return lin, sysm


def _delta_checks(g, sysm, lin, y_dev, res, ey_bound_2, worst, tag):
    """delta (after projection) and the model cost change against long double, given a 2-norm bound on y_dev - y*"""
    ystar = PH.solve_refined(sysm["K"], sysm["b"])
    delta, v, mcc, dg, dld = PH.project_step(ystar, sysm, g["pos"], g["fixed"])
    S = sysm["S"]
    # (the projection subtracts beta v with |beta| |v| <= |S y|: its own rounding is a few u |S y|)
    dd = float(np.max(np.where(sysm["act"], S, 0))) * ey_bound_2 + C0 * U * float(np.sqrt(delta @ delta) + np.sqrt((S * ystar) @ (S * ystar)))
    err = float(np.sqrt(np.sum((res["delta"].reshape(-1).astype(LD) - delta) ** 2)))
    worst["delta"] = err / dd if dd > 0 else (0.0 if err == 0 else np.inf)
    Lf = np.array(sysm["L"], float)
    normL = float(np.linalg.norm(Lf, 2))
    gn = float(np.sqrt(sysm["g"] @ sysm["g"]))
    dn = float(np.sqrt(delta @ delta))
    ad = np.abs(delta)
    cdim = C0 + 3 * g["n_cams"]
    Lmag = np.abs(sysm["L"])
    mb = dd * (gn + normL * (dn + dd)) + cdim * U * float(ad @ np.abs(sysm["g"]) + ad @ (Lmag @ ad))
    worst["model"] = abs(float(res["model_cost_change"] - mcc)) / mb
    assert mcc > 0
    return mcc


@pytest.mark.parametrize("n,radius", [(10, 1e4), (11, 1e12), (21, 1e4), (22, 1e12), (43, 1e4), (43, 1e12), (171, 1e4), (342, 1e12)])
def test_dense_step_against_hp_reference(n, radius):
    g = small_graph(n, seed=n, hub_deg=min(70, n))
    _dense_case(g, "small%d" % n, "huber", radius)


def test_dense_step_alpha_branch():
    g = small_graph(43, seed=143)
    _dense_case(g, "small43b", "tolerant", 1e4)


def test_dense_step_with_the_diagonal_clamps_binding():
    """camera 1's edges are all beyond the Tukey cut: rho' = 0, its diagonal is 0 and D^2 = min_lm_diagonal / radius; the large
    min_lm_diagonal also binds on other columns"""
    g = small_graph(22, seed=5, tukey_outlier_cam=True)
    _dense_case(g, "tukey22", "tukey", 1e4, min_diag=0.4)


def _dense_case(g, key, lname, radius, min_diag=1e-6):
    lin, sysm = _step_reference(g, key, lname, radius, min_diag)
    dev = _device(g, lname)
    res = dev.step_check(g["pos"], fixed_cam=g["fixed"], radius=radius, dense_max_cams=100000, min_lm_diagonal=min_diag)
    dev.close()
    assert res["path"] == 0 and res["chol_info"] == 0, res["chol_info"]
    A = sysm["A"]
    ck_cam = H.c_row(A["deg"], CA)
    Kb, bb, sig, Lmag, Ktrue, clamped = _bounds_K(sysm, lin, A, g, None, ck_cam, radius, min_diag, 1e32)
    if lname == "tukey":
        assert np.all(sysm["diagL"][3:6] == 0) and clamped[3:6].all()
        assert clamped.sum() > 6
    act = sysm["act"]
    Kd = res["K"]
    assert np.array_equal(Kd[~act][:, ~act], np.eye(int((~act).sum()))), "inactive block is not the identity"
    assert np.all(Kd[~act][:, act] == 0) and np.all(Kd[act][:, ~act] == 0)
    worst = {"K": H.ratio(Kd, sysm["K"], Kb), "b": H.ratio(res["b"].reshape(-1), sysm["b"], bb)}
    assert np.all(res["b"].reshape(-1)[~act] == 0) and np.all(res["y"].reshape(-1)[~act] == 0)
    nn = Kd.shape[0]
    Kf = np.array(sysm["K"], float)
    Kinv = np.linalg.inv(Kf)
    kinv_inf = float(np.abs(Kinv).sum(axis=1).max()) * 1.01
    kappa = float(np.abs(Kf).sum(axis=1).max()) * kinv_inf
    ystar = PH.solve_refined(sysm["K"], sysm["b"])
    yinf = float(np.abs(ystar).max())
    yb = 4 * nn * U * kappa * yinf + kinv_inf * (float(Kb.sum(axis=1).max()) * yinf + float(bb.max()))
    ey = np.abs(res["y"].reshape(-1).astype(LD) - ystar)
    worst["y"] = float(ey.max()) / yb
    _delta_checks(g, sysm, lin, res["y"], res, yb * np.sqrt(nn), worst, key)
    allow = {"K": H.allowed_relative(Kb[act][:, act], Ktrue[act][:, act]), "b": H.allowed_relative(bb, np.abs(sysm["S"]) * A["g_true"].reshape(-1))}
    _report("dense %s %s r=%.0e" % (key, lname, radius), worst, allow)


# ---- 3. the PCG step --------------------------------------------------------------------------------------------------------------
def _inv_norm2(K, iters=60):
    """|K^-1|_2 of a symmetric positive definite K by inverse iteration on its long-double Cholesky factor (at radius 1e16 the smallest
    eigenvalue lies below a float64 eigensolver's error)"""
    L = PH.cholesky_factor(K)
    x = np.random.default_rng(0).standard_normal(K.shape[0]).astype(LD)
    est = LD(0)
    for _ in range(iters):
        x = x / np.sqrt(x @ x)
        y = PH.cholesky_apply(L, x)
        est = np.sqrt(y @ y)
        x = y
    return float(est)


def _pcg_case(g, key, lname, radius, check_delta):
    lin, sysm = _step_reference(g, key, lname, radius)
    dev = _device(g, lname)
    o = dev.default_options()
    res = dev.step_check(g["pos"], fixed_cam=g["fixed"], radius=radius, want_K=False, dense_max_cams=0)
    dev.close()
    assert res["path"] == 1 and res["cg_iterations"] > 0
    n = g["n_cams"]
    ei, ej = g["edge_i"], g["edge_j"]
    act = sysm["act"]
    S, D2 = sysm["S"], sysm["D2"]
    y = res["y"].reshape(-1).astype(LD)
    # K y and |K| |y| by edges (long double), masked as the device masks them
    Ly, Lym, Lyt = H.matvec(lin, n, ei, ej, (S * y).reshape(n, 3))
    Ky = np.where(act, S * Ly.reshape(-1) + D2 * y, y)
    aKy = np.where(act, S * Lym.reshape(-1) + D2 * np.abs(y), np.abs(y))
    r = sysm["b"] - Ky
    A = sysm["A"]
    Dk = A["D"]
    Minv = np.zeros((n, 3, 3), LD)
    for k in range(n):
        sk = S[3 * k:3 * k + 3]
        if act[3 * k]:
            M = sk[:, None] * Dk[k] * sk[None, :] + np.diag(D2[3 * k:3 * k + 3])
            Minv[k] = np.linalg.inv(M.astype(float)).astype(LD)
        else:
            Minv[k] = np.eye(3)

    def mnorm(z):
        z3 = np.asarray(z, LD).reshape(n, 3)
        return np.sqrt(np.einsum("ka,kab,kb->", z3, Minv, z3))

    bn = mnorm(sysm["b"])
    ck_cam = H.c_row(A["deg"], CA)
    sig = 3 * U + np.repeat(ck_cam, 3) * U
    floor = mnorm(C0 * U * (aKy + np.abs(sysm["b"])) + np.repeat(ck_cam, 3) * U * aKy + np.abs(Ky) * 2 * sig
                  + np.repeat(ck_cam, 3) * U * S * A["g_mag"].reshape(-1)) / bn
    rel = mnorm(r) / bn
    tol = o.cg_relative_tolerance
    worst = {"pcg_true_residual": float(rel / (tol + floor))}
    print("pcg %s r=%.0e: true rel. residual %.3e, device's recursive %.3e, floor %.3e, iterations %d"
          % (key, radius, float(rel), res["cg_rel"], float(floor), res["cg_iterations"]))
    if check_delta:
        kinv2 = 1.05 * _inv_norm2(sysm["K"])
        r2 = float(np.sqrt(r @ r))
        pert = float(np.sqrt(np.sum((C0 * U * (aKy + np.abs(sysm["b"])) + np.repeat(ck_cam, 3) * U * aKy) ** 2)))
        _delta_checks(g, sysm, lin, res["y"], res, kinv2 * (r2 + pert), worst, key)
    _report("pcg %s %s r=%.0e" % (key, lname, radius), worst, {})


@pytest.mark.parametrize("n", [10, 43, 171])
@pytest.mark.parametrize("radius", [1e4, 1e12, 1e16])
def test_pcg_step_against_hp_reference(n, radius):
    g = small_graph(n, seed=n, hub_deg=min(70, n))
    _pcg_case(g, "small%d" % n, "huber", radius, check_delta=True)


@pytest.mark.parametrize("radius", [1e4, 1e16])
def test_pcg_step_beyond_1000_cameras(radius):
    g = small_graph(1203, seed=1203, hub_deg=300)
    _pcg_case(g, "small1203", "huber", radius, check_delta=False)


# ---- 4. a NaN gradient entry --------------------------------------------------------------------------------------------------------
def test_nan_gradient_entry_is_dropped_from_the_gradient_norm():
    """Every residual is zero at the start (t = 0, all positions 0: n = 0, r = -d = 0); the callback returns a finite rho and a NaN rho'
    on edge 5.  The gradient of its two cameras is NaN; final_gradient_max_norm drops it (fmax, as the oracle's std::fmax) and sees 0, so
    the solve stops at once on the gradient tolerance."""
    n = 12
    ei = np.arange(n - 1, dtype=np.uint32)
    ej = ei + 1
    E = len(ei)
    rel = np.zeros((E, 3))
    rot = np.zeros((n, 3))
    calls = [0]

    class NanAtEdge5(object):
        def Evaluate(self, s, out):
            e = calls[0] % E
            calls[0] += 1
            out[0], out[1], out[2] = s, (float("nan") if e == 5 else 1.0), 0.0

    dev = PositionProblem(n, ei, ej, rel, rot)
    dev.set_loss_callback(NanAtEdge5().Evaluate)
    calls[0] = 0
    ld = dev.linearize(np.zeros((n, 3)))
    bad = np.isnan(ld["gradient"]).any(axis=1)
    assert list(np.flatnonzero(bad)) == [5, 6], ld["gradient"]
    assert ld["cost"] == 0.0
    calls[0] = 0
    x, s = dev.solve(None, fixed_cam=0)
    dev.close()
    assert s["final_gradient_max_norm"] == 0.0, s
    assert s["termination_name"] == "GRADIENT_TOLERANCE", s
    assert s["num_iterations"] == 0 and np.all(x == 0.0)
