"""CPU checks of gsfm_rot_init_spanning_tree (the maximum-spanning-tree initialisation on the device): declaration, export, and the
argument checks that run on the host before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import have_gpu
from globalsfmpy_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSFM_ERR_INVALID_ARG, GSFM_ERR_NO_DEVICE, GSFM_ERR_EMPTY = 1, 2, 4


def _call(n_cams, ei, ej, rel, weight=None, null_edge_i=False):
    lib = _abi.load_library()
    ei = np.ascontiguousarray(ei, dtype=np.uint32)
    ej = np.ascontiguousarray(ej, dtype=np.uint32)
    rel = np.ascontiguousarray(rel, dtype=np.float64).reshape(-1, 3)
    rot = np.full((max(n_cams, 1), 3), 7.0)
    parent = np.full(max(n_cams, 1), 7, dtype=np.int64)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.int32)
    st = lib.gsfm_rot_init_spanning_tree(n_cams, ei.size, None if null_edge_i else u32(ei), u32(ej), rel.ctypes.data_as(C.POINTER(C.c_double)),
                                         None if w is None else w.ctypes.data_as(C.POINTER(C.c_int32)), rot.ctypes.data_as(C.POINTER(C.c_double)),
                                         parent.ctypes.data_as(C.POINTER(C.c_int64)), None, None, None, None)
    return st, lib.gsfm_last_error().decode(), rot, parent


def test_header_declares_the_entry_point_and_the_library_exports_it():
    with open(os.path.join(ROOT, "include", "gsfm_rot.h")) as f:
        h = f.read()
    assert re.search(r"gsfm_status\s+gsfm_rot_init_spanning_tree\s*\(", h)
    assert "#define GSFM_ROT_ABI_VERSION 4" in h
    lib = _abi.load_library()
    assert hasattr(lib, "gsfm_rot_init_spanning_tree")


def test_out_of_range_index_is_rejected_before_any_device_call():
    st, msg, _, _ = _call(4, [0, 1, 2], [1, 2, 4], np.zeros((3, 3)))
    assert st == GSFM_ERR_INVALID_ARG and "edge 2" in msg


def test_self_loop_is_rejected_before_any_device_call():
    st, msg, _, _ = _call(4, [0, 1, 2], [1, 1, 3], np.zeros((3, 3)))
    assert st == GSFM_ERR_INVALID_ARG and "edge 1" in msg


def test_null_edge_array_is_rejected():
    st, _, _, _ = _call(4, [0, 1, 2], [1, 2, 3], np.zeros((3, 3)), null_edge_i=True)
    assert st == GSFM_ERR_INVALID_ARG


def test_graph_without_edges_is_empty_and_leaves_zeros():
    st, _, rot, parent = _call(5, [], [], np.zeros((0, 3)))
    assert st == GSFM_ERR_EMPTY
    assert not rot.any() and (parent == -1).all()


@pytest.mark.skipif(have_gpu(), reason="CPU-only behaviour")
def test_valid_call_without_a_device_fails_loudly():
    st, msg, _, _ = _call(4, [0, 1, 2], [1, 2, 3], np.zeros((3, 3)), weight=[3, 1, 2])
    assert st == GSFM_ERR_NO_DEVICE and "no HIP device" in msg
