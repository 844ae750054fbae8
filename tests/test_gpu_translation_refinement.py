"""The relative-translation refinement on the device (gsfm_pos_refine_relative_translations, include/gsfm_pos.h) against the 50-digit
restatement (tests/translation_refinement_reference.py).  The mpmath results of the parity batch and the arithmetic yardstick spread_max are
read from tests/golden/translation_refinement_spread.json, which tests/test_translation_refinement_reference.py recomputes and checks."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from globalsfmpy_amd import _abi
from globalsfmpy_amd import solver

import translation_refinement_reference as trr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "translation_refinement_spread.json")


def refine(b, **over):
    a = dict(b, **over)
    return solver.refine_relative_translations(a["n_cams"], a["edge_i"], a["edge_j"], a["match_ptr"], a["matches"], a["intrinsics"], a["rot_aa"], a["rel_t"])


@pytest.fixture(scope="module")
def batch():
    return trr.make_batch()


@pytest.fixture(scope="module")
def device(batch):
    return refine(batch)


def test_parity_with_the_high_precision_reference(batch, device):
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["batch_seed"] == trr.BATCH_SEED and len(gold["cases"]) == len(batch["pairs"])
    bound = 4.0 * gold["spread_max"]     # the device's butterfly and fma contraction are one more summation order of the same algorithm
    t, info = device
    n_clear, worst, worst_e, n_sign = 0, 0.0, -1, 0
    for e, (p, g) in enumerate(zip(batch["pairs"], gold["cases"])):
        n = p["matches"].shape[0]
        assert g["matches"] == n and g["seed"] == trr.BATCH_SEED + 1 + e
        assert info["status"][e] == 0, (e, info["status"][e])
        assert abs(np.linalg.norm(t[e]) - 1.0) <= 1e-12
        t_ref, in_front = np.array([float.fromhex(x) for x in g["t"]]), g["in_front"]
        if g["clear"]:
            n_clear += 1
            assert info["iterations"][e] == g["iterations"], (e, n, info["iterations"][e], g["iterations"])
        else:
            # the count may hinge on rounding, within the inner-iteration window; compare with the reference forced to the device's count
            assert abs(int(info["iterations"][e]) - g["iterations"]) <= trr.MAX_INNER, (e, info["iterations"][e], g["iterations"])
            hp = trr.refine_mp(p["matches"], p["intrinsics"], p["aa1"], p["aa2"], force_iterations=int(info["iterations"][e]))
            t_ref, in_front = hp.t, hp.in_front
        ang = trr.angle(t[e], t_ref)
        if ang > worst:
            worst, worst_e = ang, e
        assert ang <= bound, (e, n, ang, bound)
        # in_front is the count under the RETURNED sign.  Above n / 2 by more than 1 that sign has the majority whatever sign the
        # eigen-solver gave t, and the device must return it too.  At or below n / 2 neither sign had a majority (a pair whose fit
        # went wrong): the rule then returns the NEGATED eigenvector, so the sign is the eigen-solver's choice and is not compared.
        if in_front > n // 2 + 1:
            n_sign += 1
            assert float(t[e] @ t_ref) > 0, (e, n, in_front)
        if g["clear"]:
            assert abs(info["cost"][e] - g["cost"]) <= 1e-9 * max(1.0, g["cost"])
    print("parity: %d edges, %d clear, %d signs compared, worst angle %.3e rad at edge %d (bound %.3e = 4 x spread_max)"
          % (len(batch["pairs"]), n_clear, n_sign, worst, worst_e, bound))
    assert n_clear >= 0.9 * len(batch["pairs"])
    assert info["kernel_ms"] > 0


def test_two_calls_return_identical_bytes(batch, device):
    t2, info2 = refine(batch)
    t, info = device
    assert np.array_equal(t.view(np.uint64), t2.view(np.uint64))
    assert np.array_equal(info["cost"].view(np.uint64), info2["cost"].view(np.uint64))
    assert np.array_equal(info["iterations"], info2["iterations"]) and np.array_equal(info["status"], info2["status"])


def permuted(b, perm):
    counts = np.diff(b["match_ptr"].astype(np.int64))
    ptr = np.concatenate([[0], np.cumsum(counts[perm])]).astype(np.uint64)
    rows = np.concatenate([np.arange(b["match_ptr"][e], b["match_ptr"][e + 1], dtype=np.int64) for e in perm])
    return dict(b, edge_i=b["edge_i"][perm], edge_j=b["edge_j"][perm], match_ptr=ptr, matches=b["matches"][rows],
                intrinsics=b["intrinsics"][perm], rel_t=b["rel_t"][perm])


def test_permuting_the_edges_permutes_the_outputs_bit_for_bit(batch, device):
    perm = np.random.Generator(np.random.PCG64(5)).permutation(len(batch["pairs"]))
    tp, ip = refine(permuted(batch, perm))
    t, info = device
    assert np.array_equal(tp.view(np.uint64), t[perm].view(np.uint64))
    assert np.array_equal(ip["cost"].view(np.uint64), info["cost"][perm].view(np.uint64))
    assert np.array_equal(ip["iterations"], info["iterations"][perm]) and np.array_equal(ip["status"], info["status"][perm])


def small(batch, edges):
    """the given edges of the batch as a problem of their own"""
    return permuted(batch, np.array(edges))


def test_edges_with_fewer_than_two_matches_are_skipped(batch):
    b = small(batch, [2, 3, 4])
    counts = [0, 1, 65]
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    t, info = refine(b, match_ptr=ptr, matches=b["matches"][:66])
    assert list(info["status"]) == [1, 1, 0] and list(info["iterations"][:2]) == [0, 0] and info["iterations"][2] > 0
    assert np.array_equal(t[:2].view(np.uint64), b["rel_t"][:2].view(np.uint64))
    assert abs(np.linalg.norm(t[2]) - 1.0) <= 1e-12
    # all edges empty, no match at all
    t0, info0 = refine(b, match_ptr=np.zeros(4, dtype=np.uint64), matches=np.zeros((0, 4)))
    assert list(info0["status"]) == [1, 1, 1] and np.array_equal(t0, b["rel_t"])


def test_all_zero_constraints_give_status_2_or_a_finite_unit_vector(batch):
    """the features of both views identical and the rotations equal: every constraint is (R^T f) x (R^T f)"""
    b = small(batch, [5])
    m = b["matches"].copy()
    m[:, 2:] = m[:, :2]
    K = b["intrinsics"].copy()
    K[:, 3:] = K[:, :3]
    rot = b["rot_aa"].copy()
    rot[b["edge_j"][0]] = rot[b["edge_i"][0]]
    t, info = refine(b, matches=m, intrinsics=K, rot_aa=rot)
    assert np.all(np.isfinite(t)) and np.isfinite(info["cost"][0])
    assert info["status"][0] in (0, 2)
    if info["status"][0] == 2:
        assert np.array_equal(t[0], b["rel_t"][0])
    else:
        assert abs(np.linalg.norm(t[0]) - 1.0) <= 1e-12
    # non-finite input: status 2, the input passed through
    m2 = b["matches"].copy()
    m2[7, 0] = np.nan
    t2, info2 = refine(b, matches=m2)
    assert info2["status"][0] == 2 and np.array_equal(t2[0], b["rel_t"][0])


def test_invalid_arguments_are_rejected_on_the_host(batch):
    b = small(batch, [0, 1, 2])
    with pytest.raises(solver.SolverError, match="out-of-range camera"):
        refine(b, edge_j=np.array([1, b["n_cams"], 5], dtype=np.uint32))
    ptr = b["match_ptr"].copy()
    ptr[1], ptr[2] = ptr[2], ptr[1]
    assert ptr[2] < ptr[1]
    with pytest.raises(solver.SolverError, match="match_ptr decreases"):
        refine(b, match_ptr=ptr)
    # NULL required pointers, straight at the C entry
    lib = _abi.load_library()
    E = 3
    out, status = np.empty((E, 3)), np.zeros(E, dtype=np.int32)
    dp, u32, i32 = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    good = [b["n_cams"], E, b["edge_i"].ctypes.data_as(u32), b["edge_j"].ctypes.data_as(u32), b["match_ptr"].ctypes.data_as(C.POINTER(C.c_uint64)),
            b["matches"].ctypes.data_as(dp), b["intrinsics"].ctypes.data_as(dp), b["rot_aa"].ctypes.data_as(dp), b["rel_t"].ctypes.data_as(dp),
            out.ctypes.data_as(dp), status.ctypes.data_as(i32), None, None, None]
    assert lib.gsfm_pos_refine_relative_translations(*good) == 0      # the optional outputs may be NULL
    for k in (2, 3, 4, 5, 6, 7, 8, 9, 10):
        args = list(good)
        args[k] = None
        assert lib.gsfm_pos_refine_relative_translations(*args) == _abi.ERR_INVALID_ARG, k
    args = list(good)
    args[1] = 0
    assert lib.gsfm_pos_refine_relative_translations(*args) == 0      # no edges
