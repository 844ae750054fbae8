"""The argument checks of gsfm_tracks_select_good and gsfm_tracks_select_good_from_statistics (include/gsfm_tracks.h).  Every check runs on the
host before the device is looked up, so all of this passes without one: a refusal is GSFM_ERR_INVALID_ARG whether a device is there or not,
and the calls that have nothing to select answer GSFM_OK with kernel_ms = 0."""
import ctypes as C

import numpy as np
import pytest

from globalsfmpy_amd import _abi

DEVICE, HOST = "gsfm_tracks_select_good", "gsfm_tracks_select_good_from_statistics"
ARGS = {DEVICE: "n_cams rot_aa cam_pos intrinsics cam_estimated n_tracks track_ptr obs_cam obs_xy points point_estimated L S K hash_capacity_log2 "
                "selected_out n_views_out mean_sq_err_out counts_out kernel_ms top_up_out",
        HOST: "n_cams cam_estimated n_tracks track_ptr obs_cam obs_xy point_estimated n_views mean_sq_err L S K selected_out counts_out"}
REQUIRED = {DEVICE: "rot_aa cam_pos intrinsics track_ptr obs_cam obs_xy points selected_out", HOST: "track_ptr obs_cam obs_xy n_views mean_sq_err selected_out"}
BOTH = (DEVICE, HOST)


def defaults():
    """A valid scene of 3 cameras and 2 tracks of 2 observations; the outputs are filled with 7 so that what a call wrote shows"""
    return dict(n_cams=3, rot_aa=np.zeros((3, 3)), cam_pos=np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), intrinsics=np.tile([1000.0, 500.0, 400.0], (3, 1)),
                cam_estimated=None, n_tracks=2, track_ptr=np.array([0, 2, 4], np.uint64), obs_cam=np.array([0, 1, 2, 0], np.uint32),
                obs_xy=np.array([[10.0, 20.0], [30.0, 40.0], [-50.0, 60.0], [70.0, 80.0]]), points=np.ones((2, 3)), point_estimated=None,
                n_views=np.array([2, 2], np.int32), mean_sq_err=np.array([1.0, 2.0]), L=10, S=100, K=200, hash_capacity_log2=0,
                selected_out=np.full(2, 7, np.uint8), n_views_out=np.full(2, 7, np.int32), mean_sq_err_out=np.full(2, 7.0),
                counts_out=np.full(6, 7, np.uint64), kernel_ms=np.full(1, 7.0), top_up_out=np.full(2, 7.0))


def call(entry, **over):
    lib = _abi.load_library()
    a = dict(defaults(), **over)
    fn = getattr(lib, entry)
    keep = [a[k] for k in ARGS[entry].split()]
    argv = [C.cast(v.ctypes.data, t) if isinstance(v, np.ndarray) else v for v, t in zip(keep, fn.argtypes)]
    status = int(fn(*argv))
    return status, (lib.gsfm_last_error().decode("utf-8", "replace") if status else ""), a


def refused(entry, **over):
    status, message, a = call(entry, **over)
    assert status == _abi.ERR_INVALID_ARG, (entry, over.keys(), status, message)
    assert message
    if a["selected_out"] is not None:
        assert (a["selected_out"] == 7).all()          # nothing was written
    if a["counts_out"] is not None:
        assert not a["counts_out"].any()               # but the counts are cleared first
    return message


def test_the_exports_are_present():
    lib = _abi.load_library()
    for entry in BOTH:
        assert getattr(lib, entry).restype is C.c_int and len(getattr(lib, entry).argtypes) == len(ARGS[entry].split())


@pytest.mark.parametrize("entry", BOTH)
def test_null_required_pointers(entry):
    for name in REQUIRED[entry].split():
        assert "NULL" in refused(entry, **{name: None}), name


@pytest.mark.parametrize("entry", BOTH)
def test_parameters_out_of_range(entry):
    assert "long_track_length_threshold" in refused(entry, L=0)
    assert "image_grid_cell_size_pixels" in refused(entry, S=0)
    assert "image_grid_cell_size_pixels" in refused(entry, S=-100)
    assert "min_num_optimized_tracks_per_view" in refused(entry, K=-1)
    assert "long_track_length_threshold" in refused(entry, L=0, track_ptr=None)   # the parameters are reported before the arrays


def test_hash_capacity_out_of_range():
    assert "hash_capacity_log2" in refused(DEVICE, hash_capacity_log2=-1)
    assert "hash_capacity_log2" in refused(DEVICE, hash_capacity_log2=32)
    assert "fewer slots than the 4 items" in refused(DEVICE, hash_capacity_log2=1)   # 2 slots for 4 items
    # the items count, not the observations: with camera 0 unestimated two items are left and two slots hold them
    status, message, _ = call(DEVICE, hash_capacity_log2=1, cam_estimated=np.array([0, 1, 1], np.uint8))
    assert status in (_abi.OK, _abi.ERR_NO_DEVICE), message


@pytest.mark.parametrize("entry", BOTH)
def test_coordinates_off_the_grid(entry):
    for bad in (np.nan, np.inf, -np.inf):
        xy = defaults()["obs_xy"]
        xy[2, 1] = bad
        assert "not finite" in refused(entry, obs_xy=xy)
    xy = defaults()["obs_xy"]
    xy[1, 0] = -(2.0 ** 31) * 100.0
    assert "2^31" in refused(entry, obs_xy=xy)
    xy[1, 0] = 2.0 ** 31
    assert "2^31" in refused(entry, obs_xy=xy, S=1)
    xy[1, 0] = 2.0 ** 31 - 0.5                          # truncates to 2^31 - 1: inside
    status, message, _ = call(entry, obs_xy=xy, S=1)
    assert status in (_abi.OK, _abi.ERR_NO_DEVICE), message
    # an observation of a track or a camera that is not estimated is checked as well
    xy = defaults()["obs_xy"]
    xy[3, 0] = np.nan
    assert "not finite" in refused(entry, obs_xy=xy, point_estimated=np.array([1, 0], np.uint8))


@pytest.mark.parametrize("entry", BOTH)
def test_the_rules_of_the_track_arrays(entry):
    assert "track_ptr[0]" in refused(entry, track_ptr=np.array([1, 2, 4], np.uint64))
    assert "decreases at track 1" in refused(entry, track_ptr=np.array([0, 3, 2, 4], np.uint64), n_tracks=3,
                                             n_views=np.zeros(3, np.int32), mean_sq_err=np.zeros(3), points=np.ones((3, 3)), selected_out=np.full(3, 7, np.uint8))
    assert "out-of-range camera" in refused(entry, obs_cam=np.array([0, 1, 3, 0], np.uint32))
    assert "2^31 tracks" in refused(entry, n_tracks=1 << 31, track_ptr=np.array([0], np.uint64))
    assert "too long" in refused(entry, n_tracks=1, track_ptr=np.array([0, 1 << 31], np.uint64), obs_cam=None, obs_xy=None)
    assert "2^31 observations" in refused(entry, n_tracks=2, track_ptr=np.array([0, 1 << 30, 1 << 31], np.uint64))


def test_a_negative_n_views_of_an_estimated_track():
    assert "negative n_views" in refused(HOST, n_views=np.array([2, -1], np.int32))
    status, message, _ = call(HOST, n_views=np.array([2, -1], np.int32), point_estimated=np.array([1, 0], np.uint8))
    assert status == _abi.OK, message


@pytest.mark.parametrize("entry", BOTH)
def test_nothing_to_select(entry):
    nothing = {k: None for k, v in defaults().items() if isinstance(v, np.ndarray) and k not in ("counts_out", "kernel_ms", "top_up_out")}
    status, message, a = call(entry, n_tracks=0, **nothing)
    assert status == _abi.OK, message
    assert not a["counts_out"].any() and (entry == HOST or (a["kernel_ms"][0] == 0.0 and not a["top_up_out"].any()))
    status, message, a = call(entry, point_estimated=np.zeros(2, np.uint8))   # no track is estimated: answered on the host
    assert status == _abi.OK, message
    assert not a["selected_out"].any() and not a["counts_out"].any()
    if entry == DEVICE:
        assert a["kernel_ms"][0] == 0.0 and not a["n_views_out"].any() and not a["mean_sq_err_out"].view(np.uint64).any()
    status, message, a = call(entry, point_estimated=np.zeros(2, np.uint8), counts_out=None, kernel_ms=None, top_up_out=None, n_views_out=None, mean_sq_err_out=None)
    assert status == _abi.OK, message


def test_the_host_entry_on_the_valid_scene():
    status, message, a = call(HOST, K=0)
    assert status == _abi.OK, message
    # camera 0 holds both tracks in one cell (track 0 wins it), cameras 1 and 2 one track and one cell each
    assert a["selected_out"].tolist() == [1, 1] and a["counts_out"].tolist() == [2, 3, 2, 0, 0, 2]
