"""The argument checks of the entries that take cameras and a track CSR (gsfm_tracks_triangulate, gsfm_tracks_triangulate_refine,
gsfm_tracks_outlier_tracks, gsfm_tracks_launch_order, gsfm_ba_problem_create, gsfm_ba6_problem_create) and of the one-leaf loss
(the refinement, gsfm_ba_set_loss, gsfm_ba6_set_loss) as a table of calls: cases() lists (entry, case name, overrides of the small valid
scene), replay() makes one call and returns (status, message, outputs).  Every check runs on the host before the device is looked up, so
the table is recorded and replayed without one.  tools/make_track_refusals_golden.py writes tests/golden/track_refusals.json from it,
tests/test_track_refusals.py replays it."""
import ctypes as C
import re

import numpy as np

from globalsfmpy_amd import _abi

NAN = float("nan")
TRI, REFINE, OUTLIER, ORDER = "gsfm_tracks_triangulate", "gsfm_tracks_triangulate_refine", "gsfm_tracks_outlier_tracks", "gsfm_tracks_launch_order"
BA, BA6, BA_LOSS, BA6_LOSS = "gsfm_ba_problem_create", "gsfm_ba6_problem_create", "gsfm_ba_set_loss", "gsfm_ba6_set_loss"
ONE_SHOT, CREATES = (TRI, REFINE, OUTLIER), (BA, BA6)

_CAMS = "n_cams rot_aa cam_pos intrinsics cam_estimated n_tracks track_ptr obs_cam obs_xy "
_OUT = "status_out n_views_out mean_sq_err_out "
ARGS = {TRI: _CAMS + "min_angle max_err point_out " + _OUT + "counts_out kernel_ms",
        REFINE: _CAMS + "min_angle max_err options loss n_loss point_out " + _OUT + "iterations_out initial_cost_out final_cost_out termination_out counts_out kernel_ms",
        OUTLIER: _CAMS + "points point_estimated max_err min_angle " + _OUT + "counts_out kernel_ms",
        ORDER: "n_tracks track_ptr order_out class_begin_out",
        BA: "n_cams rot_aa intrinsics cam_estimated n_tracks track_ptr obs_cam obs_xy point_estimated out",
        BA6: "n_cams intrinsics cam_estimated n_tracks track_ptr obs_cam obs_xy point_estimated out",
        BA_LOSS: "handle loss n_loss", BA6_LOSS: "handle loss n_loss"}
REQUIRED = {TRI: "track_ptr point_out status_out rot_aa cam_pos intrinsics obs_cam obs_xy", REFINE: "track_ptr point_out status_out rot_aa cam_pos intrinsics obs_cam obs_xy",
            OUTLIER: "track_ptr points status_out rot_aa cam_pos intrinsics obs_cam obs_xy", ORDER: "class_begin_out track_ptr order_out",
            BA: "out rot_aa intrinsics track_ptr obs_cam obs_xy", BA6: "out intrinsics track_ptr obs_cam obs_xy"}
OUTPUTS = ("point_out", "status_out", "n_views_out", "mean_sq_err_out", "iterations_out", "initial_cost_out", "final_cost_out", "termination_out",
           "counts_out", "kernel_ms", "order_out", "class_begin_out", "out", "handle")


def defaults():
    """A valid scene of 3 cameras and 2 tracks of 2 observations, and outputs (room for 4 tracks) filled with 7 so that what a call wrote shows"""
    f64, i32 = (lambda *shape: np.full(shape, 7.0)), (lambda n: np.full(n, 7, dtype=np.int32))
    return dict(n_cams=3, rot_aa=np.zeros((3, 3)), cam_pos=np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), intrinsics=np.tile([1000.0, 500.0, 400.0], (3, 1)),
                cam_estimated=None, n_tracks=2, track_ptr=np.array([0, 2, 4], np.uint64), obs_cam=np.array([0, 1, 2, 0], np.uint32), obs_xy=np.zeros((4, 2)),
                min_angle=4.0, max_err=15.0, options=None, loss=None, n_loss=0, points=np.ones((2, 3)), point_estimated=None,
                point_out=f64(4, 3), status_out=i32(4), n_views_out=i32(4), mean_sq_err_out=f64(4), iterations_out=i32(4), initial_cost_out=f64(4),
                final_cost_out=f64(4), termination_out=i32(4), counts_out=np.full(7, 7, dtype=np.uint64), kernel_ms=f64(1),
                order_out=np.full(4, 7, dtype=np.uint32), class_begin_out=np.full(4, 7, dtype=np.uint64), out=np.full(1, 7, dtype=np.uint64),
                handle=np.zeros(1 << 13, dtype=np.uint64))   # (a handle that is no problem: the set-loss entries refuse before they read it)


def _options(**fields):
    def make(lib):
        o = _abi.TrackRefineOptions()
        lib.gsfm_tracks_refine_default_options(C.byref(o))
        for k, v in fields.items():
            setattr(o, k, v)
        return o
    return make


def _u64(*v):
    return np.array(v, dtype=np.uint64)


def cases():
    rows = []

    def add(entries, name, **over):
        rows.extend((e, name, over) for e in ([entries] if isinstance(entries, str) else entries))
    csr = ONE_SHOT + CREATES
    bad_ptr0, decrease = dict(track_ptr=_u64(1, 2, 4)), dict(track_ptr=_u64(0, 3, 2, 4), n_tracks=3)
    bad_cam = dict(obs_cam=np.array([0, 1, 3, 0], np.uint32))
    for e, keys in REQUIRED.items():
        for k in keys.split():
            add(e, "NULL " + k, **{k: None})
    add(csr, "no observations and NULL obs_cam, obs_xy", track_ptr=_u64(0, 0, 0), obs_cam=None, obs_xy=None)
    everything = {k: None for k, v in defaults().items() if isinstance(v, np.ndarray) and k != "out"}
    add(ONE_SHOT + (ORDER,), "no tracks and everything NULL", n_cams=0, n_tracks=0, **everything)
    add(ONE_SHOT, "no tracks and NULL cameras", n_tracks=0, **everything)
    add(ORDER, "no tracks", n_tracks=0, track_ptr=None, order_out=None)
    add(CREATES, "no tracks, no cameras and everything NULL", n_cams=0, n_tracks=0, **everything)
    add(csr + (ORDER,), "track_ptr[0] = 1", **bad_ptr0)
    add(csr + (ORDER,), "decrease at track 1", **decrease)
    add(csr, "camera 3 of 3 at observation 2", **bad_cam)
    for key in ("min_angle", "max_err"):
        add(ONE_SHOT, key + " negative", **{key: -1.0})
        add(ONE_SHOT, key + " NaN", **{key: NAN})
        add(ONE_SHOT, key + " infinite", **{key: float("inf")})
    add(ONE_SHOT, "both bounds negative", min_angle=-1.0, max_err=-2.0)
    add(ONE_SHOT + (ORDER,), "2^31 tracks", n_tracks=1 << 31, track_ptr=_u64(0))
    add(ONE_SHOT + (ORDER,), "a track of 2^31 observations", n_tracks=1, track_ptr=_u64(0, 1 << 31), obs_cam=None, obs_xy=None)
    add(CREATES, "2^31 observations", n_tracks=1, track_ptr=_u64(0, 1 << 31), obs_cam=None, obs_xy=None)
    add(CREATES, "2^31 - 1 cameras and a track", n_cams=(1 << 31) - 1, n_tracks=1, track_ptr=_u64(0, 0))
    add(BA6, "2^30 cameras", n_cams=1 << 30, n_tracks=0, track_ptr=_u64(0))
    # two faults at once: which one is reported
    add(ONE_SHOT, "bad angle and NULL track_ptr", min_angle=-1.0, track_ptr=None)
    add(ONE_SHOT, "NULL cameras and 2^31 tracks", rot_aa=None, n_tracks=1 << 31, track_ptr=_u64(0))
    add(ONE_SHOT + (ORDER,), "2^31 tracks and track_ptr[0] = 1", n_tracks=1 << 31, track_ptr=_u64(1))
    add(csr + (ORDER,), "track_ptr[0] = 1 and a decrease", track_ptr=_u64(1, 3, 2, 4), n_tracks=3)
    add(csr + (ORDER,), "a decrease after a track of 2^31", track_ptr=_u64(0, 1 << 31, 2), obs_cam=None, obs_xy=None)
    add(csr, "NULL obs_xy and a bad camera", obs_xy=None, **bad_cam)
    add(CREATES, "NULL cameras and NULL track_ptr", intrinsics=None, track_ptr=None)
    add(CREATES, "NULL track_ptr and NULL obs_cam", track_ptr=None, obs_cam=None)
    add(CREATES, "2^31 observations after track_ptr[0] = 1", n_tracks=1, track_ptr=_u64(1, 1 << 31), obs_cam=None, obs_xy=None)
    huber = [(_abi.LOSS_HUBER, 10.0)]
    add(REFINE, "bad loss and bad CSR", loss=huber + huber, n_loss=2, **decrease)
    add(REFINE, "bad tolerance and bad CSR", options=_options(function_tolerance=-1.0), **decrease)
    add(REFINE, "bad loss and bad tolerance", loss=[(_abi.LOSS_MAGSAC, 0.02, 3, 0)], n_loss=1, options=_options(function_tolerance=NAN))
    add(REFINE, "bad radius and bad angle", options=_options(initial_trust_region_radius=0.0), min_angle=NAN)
    add(REFINE, "bad tolerance and bad radius", options=_options(gradient_tolerance=NAN, max_trust_region_radius=-1.0))
    add(REFINE, "refinement off", options=_options(refine=0))
    add(REFINE, "refinement off and bad CSR", options=_options(refine=0), **decrease)
    # the one-leaf loss
    losses = (REFINE, BA_LOSS, BA6_LOSS)
    add(losses, "loss n = -1", loss=huber, n_loss=-1)
    add(losses, "loss n = 2", loss=huber + huber, n_loss=2)
    add(losses, "loss n = 1 and a NULL program", loss=None, n_loss=1)
    add(losses, "loss n = 2 and a NULL program", loss=None, n_loss=2)
    add(losses, "MAGSAC leaf", loss=[(_abi.LOSS_MAGSAC, 0.02, 3, 0)], n_loss=1)
    add(losses, "Cauchy leaf", loss=[(_abi.LOSS_CAUCHY, 10.0)], n_loss=1)
    add(losses, "NaN parameter", loss=[(_abi.LOSS_HUBER, 10.0, NAN)], n_loss=1)
    add(losses, "NaN width", loss=[(_abi.LOSS_HUBER, NAN)], n_loss=1)
    add(losses, "zero width", loss=[(_abi.LOSS_TUKEY, 0.0)], n_loss=1)
    add(losses, "MAGSAC leaf with a NaN parameter", loss=[(_abi.LOSS_MAGSAC, NAN, 3, 0)], n_loss=1)
    add((BA_LOSS, BA6_LOSS), "NULL handle", handle=None, loss=huber, n_loss=1)
    # answered on the host, and the valid scene that needs the device
    add(OUTLIER, "no track is estimated", point_estimated=np.zeros(2, np.uint8))
    add(OUTLIER, "no track is estimated, optional outputs NULL", point_estimated=np.zeros(2, np.uint8), n_views_out=None, mean_sq_err_out=None, counts_out=None, kernel_ms=None)
    add(csr, "valid scene")
    add(REFINE, "valid scene under Huber", loss=huber, n_loss=1)
    return rows


def replay(lib, entry, over):
    """One call: (status, message or "", {output name: list of what the call left in it})"""
    a = dict(defaults(), **over)
    if callable(a["options"]):
        a["options"] = a["options"](lib)
    if a["loss"] is not None:
        a["loss"] = _abi.make_program(a["loss"])[0]
    fn = getattr(lib, entry)
    names = ARGS[entry].split()
    keep = [a[k] for k in names]   # (the arrays outlive the call)
    argv = [C.cast(v.ctypes.data, t) if isinstance(v, np.ndarray) else C.byref(v) if isinstance(v, C.Structure) else v for v, t in zip(keep, fn.argtypes)]
    status = int(fn(*argv))
    message = lib.gsfm_last_error().decode("utf-8", "replace") if status else ""
    # (the missing device's message quotes the HIP runtime's own words for it, which are not this library's to keep)
    message = re.sub(r"\(hipGetDeviceCount: .*?, \d+ devices;", "(hipGetDeviceCount: ...;", message)
    outputs = {k: a[k].ravel().tolist() for k in names if k in OUTPUTS and a[k] is not None}
    if "handle" in outputs:
        outputs["handle"] = [int(np.count_nonzero(a["handle"]))]
    return status, message, outputs
