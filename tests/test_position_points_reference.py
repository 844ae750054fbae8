"""CPU: the two references of position estimation with point-to-camera constraints (tests/position_points_reference.py, float64;
tests/position_points_hp_reference.py, mpmath / long double) against each other and against finite differences, and the conditions the
GPU tests (tests/test_gpu_position_points.py) rely on."""
import numpy as np

from globalsfmpy_amd import loss_functions as LF

import hp_reference as H
import position_hp_reference as PH
import position_points_hp_reference as PPH
import position_points_reference as PR

LD, U = H.LD, H.U
W_P = 0.37


def _reference(sc, loss=None, weight=W_P):
    return PR.PointPositionReference(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["rel_t"], sc["rot_aa"], sc["ray_rot_aa"], sc["intrinsics"],
                                     sc["track_ptr"], sc["obs_cam"], sc["obs_xy"], weight, loss)


def _eval():
    sc = PR.make_scene(noise=0.01, outlier_frac=0.1)
    c0, p0 = PR.perturbed_start(sc, 0.3, 1)
    return sc, c0, p0


_T1 = {}


def _tier1():
    if "t" not in _T1:
        sc, c0, p0 = _eval()
        _T1["t"] = PPH.joint_edge_set(sc, c0, p0, W_P)
    return _T1["t"]


def test_scene_reaches_every_branch():
    sc, c0, p0 = _eval()
    st = PR.structure(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["track_ptr"], sc["obs_cam"])
    lengths = np.diff(sc["track_ptr"].astype(np.int64))
    assert sc["n_cams"] == 72 and len(sc["edge_i"]) == 300 and len(lengths) == 91
    assert set(PR.LONG_LENGTHS) <= set(lengths) and {8, 9, 64, 65} <= set(lengths)   # both sides of the lane classes' limits
    rows = np.bincount(sc["obs_cam"][st["used"]], minlength=72)
    assert rows[PR.HUB] > 64 and rows[PR.FIXED] >= 3 and rows[PR.NO_OBS_CAM] == 0 and st["present"][PR.NO_OBS_CAM]
    assert not st["present"][list(PR.EDGELESS)].any() and rows[list(PR.EDGELESS)].sum() == 0
    tp = sc["track_ptr"].astype(np.int64)
    single = slice(tp[PR.SINGLE_TRACK], tp[PR.SINGLE_TRACK + 1])
    assert st["present"][sc["obs_cam"][single]].sum() == 1 and not st["point_active"][PR.SINGLE_TRACK] and not st["used"][single].any()
    assert (~st["point_active"]).sum() == 1 and (~st["used"]).sum() >= 3
    for t in range(len(lengths)):   # a camera sees a track once among the used observations (the preconditioner's formula is the block diagonal then)
        cams = sc["obs_cam"][tp[t]:tp[t + 1]][st["used"][tp[t]:tp[t + 1]]]
        assert len(set(cams)) == len(cams)
    assert np.array_equal(c0[PR.COINCIDENT[0]], c0[PR.COINCIDENT[1]])
    first = int(sc["obs_cam"][tp[1]])
    assert st["used"][tp[1]] and np.array_equal(p0[1], c0[first])


def test_float64_and_hp_references_agree():
    sc, c0, p0 = _eval()
    ref = _tier1()
    E = ref["n_edges"]
    assert (~ref["unit"][:E]).sum() == 1 and (~ref["unit"][E:]).sum() == 1
    for loss, kind, params in ((None, None, ()), (LF.HuberLoss(0.1), "huber", (0.1,)), (LF.TolerantLoss(0.05, 0.1), "tolerant", (0.05, 0.1))):
        r64 = _reference(sc, loss)
        x = r64.joint(c0, p0)
        assert np.array_equal(r64.ei, ref["ei"]) and np.array_equal(r64.ej, ref["ej"])
        lin = PH.corrected(ref, kind, params)
        cost, g, A, rt, _ = r64.linearize(x)
        assert np.abs(r64.ray - ref["ray"].astype(float)).max() <= 8 * U
        assert np.abs(r64.residuals(x)[0] - ref["r"].astype(float)).max() <= 64 * U * float(ref["e_mag"].max())
        asm = H.assemble(lin, ref["n_nodes"], ref["ei"], ref["ej"])
        assert abs(cost - float(asm["cost"])) <= 1e-12 * float(asm["cost"])
        assert np.abs(g - asm["g"].astype(float)).max() <= 1e-11 * float(np.abs(asm["g"]).max())
        assert np.abs(A - lin["Jjt"].astype(float)).max() <= 1e-11 * float(np.abs(lin["Jjt"]).max())
        if kind == "tolerant":
            assert (lin["rho"][2][:E] > 0).sum() > E // 4 and (lin["rho"][2][E:] > 0).sum() > (len(ref["ei"]) - E) // 4
        if kind == "huber":
            s = lin["s"].astype(float)
            assert (s > 0.01).any() and (s < 0.01).any() and np.all(np.abs(s - 0.01) > 1e-11)


def test_gradient_against_finite_differences_of_the_cost():
    sc, c0, p0 = _eval()
    c0 = c0.copy()
    c0[PR.COINCIDENT[1]] += 0.1   # (away from the guard's kink)
    p0 = p0.copy()
    p0[1] += 0.1
    for loss in (None, LF.CauchyLoss(0.1)):
        r64 = _reference(sc, loss)
        x = r64.joint(c0, p0)
        _, g, _, _, _ = r64.linearize(x)
        rng = np.random.default_rng(0)
        for _ in range(5):
            d = np.where(r64.present[:, None], rng.standard_normal(x.shape), 0.0)
            h = 1e-6
            fd = (r64.cost(x + h * d) - r64.cost(x - h * d)) / (2 * h)
            assert abs(fd - (g * d).sum()) <= 1e-6 * max(1.0, abs(fd))
        assert np.all(g[~r64.present] == 0)


def test_schur_complement_solves_the_full_system():
    sc, c0, p0 = _eval()
    ref = _tier1()
    N, nn = sc["n_cams"], ref["n_nodes"]
    lin = PH.corrected(ref, "huber", (0.1,))
    Lm, g = PPH.normal_system(lin["Jjt"], lin["rt"], ref["ei"], ref["ej"], nn, LD)
    Ld = H.normal_matrix(lin, nn, ref["ei"], ref["ej"])
    assert np.abs(Lm - Ld).max() <= 1e-17 * float(np.abs(Ld).max())   # (the same matrix by hp_reference's own assembly)
    st = ref["structure"]
    act = np.concatenate([st["present"], st["point_active"]])
    act[sc["fixed"]] = False
    for radius in (1e4, 1e10):
        sysm = PPH.damped_system(Lm, g, act, radius, LD)
        chk = PH.step_system(lin, nn, ref["ei"], ref["ej"], act, radius)
        assert np.abs(sysm["K"] - chk["K"]).max() <= 1e-17 and np.abs(sysm["b"] - chk["b"]).max() <= 1e-17 * float(np.abs(chk["b"]).max())
        Sc, rhs, Mb = PPH.schur_system(sysm, N)
        y = PPH.solve_full(sysm)
        yc = PH.solve_refined(Sc, rhs)
        scale = float(np.abs(y).max())
        assert np.abs(yc - y[:3 * N]).max() <= 1e-9 * scale
        assert np.abs(PPH.back_substitute(sysm, N, yc).reshape(-1) - y[3 * N:]).max() <= 1e-9 * scale
        off = ~act[:N]
        assert np.array_equal(Sc[np.repeat(off, 3)][:, np.repeat(off, 3)], np.eye(3 * off.sum())) and np.all(rhs[np.repeat(off, 3)] == 0)
        delta, model = PPH.project_step(sysm, y, np.concatenate([c0, p0]), sc["fixed"])
        plain, model_plain = PPH.project_step(sysm, y, np.concatenate([c0, p0]), sc["fixed"], gauge=False)
        assert model > 0 and abs(float(model - model_plain)) <= 1e-9 * float(model)
        # the float64 tier runs the same steps
        r64 = _reference(sc, LF.HuberLoss(0.1))
        _, _, A, rt, _ = r64.linearize(r64.joint(c0, p0))
        L64, g64 = PPH.normal_system(A, rt, r64.ei, r64.ej, nn, np.float64)
        s64 = PPH.damped_system(L64, g64, act, radius, np.float64)
        assert s64["K"].dtype == np.float64 and np.abs(s64["K"] - sysm["K"].astype(float)).max() <= 1e-10
        y1 = PPH.first_pcg_iterate(Sc, rhs, Mb)
        assert np.all(np.isfinite(y1.astype(float))) and np.all(y1.reshape(N, 3)[off] == 0)


def test_reference_solves():
    sc = PR.make_scene()
    st = PR.structure(sc["n_cams"], sc["edge_i"], sc["edge_j"], sc["track_ptr"], sc["obs_cam"])
    c, p, s = _reference(sc, None, 0.5).solve_joint(fixed_cam=sc["fixed"])
    err = np.abs(PR.gauge_normalize(c, p, sc["fixed"], st["present"], st["point_active"])
                 - PR.gauge_normalize(sc["gt_pos"], sc["gt_points"], sc["fixed"], st["present"], st["point_active"])).max()
    assert s["termination"] in (0, 1, 2) and err <= 1e-8
    assert np.array_equal(c[list(PR.EDGELESS)], np.zeros((2, 3))) and np.array_equal(p[PR.SINGLE_TRACK], np.ones(3))   # inactive: as given
    # the noisy case of the GPU tests: the iteration count does not hang on the last digits of the weight
    sc = PR.make_scene(noise=0.01, outlier_frac=0.1, seed=5)
    runs = [_reference(sc, LF.HuberLoss(0.1), w).solve_joint(fixed_cam=sc["fixed"])[2] for w in (0.5, 0.5 * (1 + 1e-12))]
    assert runs[0]["num_iterations"] == runs[1]["num_iterations"] and runs[0]["termination"] == runs[1]["termination"]
    assert runs[0]["num_iterations"] >= 3 and runs[0]["termination"] in (0, 1, 2)
