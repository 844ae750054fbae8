"""Every entry that takes cameras and a track CSR, and every entry that takes the one-leaf loss, answers the calls of tests/track_refusals.py
as the commit before csrc/track_scene.hpp did: the same status, the same message, the same bytes left in the outputs
(tests/golden/track_refusals.json, recorded by tools/make_track_refusals_golden.py from a library built from that commit).  All of it is host
code that runs before the device is looked up.  The rows that end in GSFM_ERR_NO_DEVICE are replayed only where there is no device."""
import json
import os

from globalsfmpy_amd import _abi

from conftest import have_gpu
import track_refusals as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "track_refusals.json")


def test_every_call_of_the_table_is_answered_as_recorded():
    with open(GOLDEN) as f:
        gold = {(r["entry"], r["case"]): r for r in json.load(f)}
    table = TR.cases()
    assert sorted(gold) == sorted((e, c) for e, c, _ in table)
    lib = _abi.load_library()
    device, replayed, wrong = have_gpu(), 0, []
    for entry, case, over in table:
        want = gold[(entry, case)]
        if device and want["status"] == _abi.ERR_NO_DEVICE:
            continue
        status, message, outputs = TR.replay(lib, entry, over)
        replayed += 1
        if (status, message, outputs) != (want["status"], want["message"], want["outputs"]):
            wrong.append((entry, case, status, message, want["status"], want["message"], {k for k in outputs if outputs[k] != want["outputs"].get(k)}))
    print("%d of %d calls replayed" % (replayed, len(table)))
    assert not wrong, wrong
    statuses = {r["status"] for r in gold.values()}
    assert statuses == {_abi.OK, _abi.ERR_INVALID_ARG, _abi.ERR_NO_DEVICE} and replayed >= 150


def test_the_table_holds_what_it_is_meant_to_pin():
    with open(GOLDEN) as f:
        gold = {(r["entry"], r["case"]): r for r in json.load(f)}
    for e in TR.ONE_SHOT + TR.CREATES:   # the caller's name in the message of the missing device
        assert gold[(e, "valid scene")]["status"] == _abi.ERR_NO_DEVICE
    assert "the track triangulation" in gold[(TR.TRI, "valid scene")]["message"] and "the outlier rule" in gold[(TR.OUTLIER, "valid scene")]["message"]
    assert "gsfm_ba_problem_create" in gold[(TR.BA, "valid scene")]["message"] and "gsfm_ba6_problem_create" in gold[(TR.BA6, "valid scene")]["message"]
    # gsfm_tracks_launch_order does not look at track_ptr[0]; the others refuse it
    assert gold[(TR.ORDER, "track_ptr[0] = 1")]["status"] == _abi.OK and gold[(TR.TRI, "track_ptr[0] = 1")]["message"] == "track_ptr[0] must be 0"
    # the two size rules, and which fault of two is reported
    assert gold[(TR.TRI, "a decrease after a track of 2^31")]["message"].startswith("track 0 is too long")
    assert gold[(TR.BA, "a decrease after a track of 2^31")]["message"] == "track_ptr decreases at track 1"
    assert gold[(TR.BA6, "2^30 cameras")]["message"] == "problem too large (2^31 observations or nodes)"
    assert "max_reprojection_error_pixels" in gold[(TR.OUTLIER, "both bounds negative")]["message"]
    assert "min_triangulation_angle_degrees" in gold[(TR.TRI, "both bounds negative")]["message"]
    assert "one leaf" in gold[(TR.REFINE, "bad loss and bad CSR")]["message"] and "tolerances" in gold[(TR.REFINE, "bad tolerance and bad CSR")]["message"]
    assert "one leaf" in gold[(TR.REFINE, "loss n = 2 and a NULL program")]["message"] and gold[(TR.REFINE, "loss n = 1 and a NULL program")]["message"] == "NULL argument"
    # no track estimated: answered without a device
    r = gold[(TR.OUTLIER, "no track is estimated")]
    assert r["status"] == _abi.OK and r["outputs"]["status_out"][:2] == [1, 1] and r["outputs"]["counts_out"][:5] == [0, 2, 0, 0, 0] and r["outputs"]["kernel_ms"] == [0.0]
