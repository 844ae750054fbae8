"""CPU checks of the exact step's host-side pieces: the component rest rule (csrc/comp_rest.hpp, compiled by the host compiler and run
on a table of cases), and the argument checks of gsfm_rot_dense_factor_check that run before any device call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from globalsfmpy_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSFM_ERR_INVALID_ARG, GSFM_ERR_UNSUPPORTED = 1, 6


def test_rest_rule_table(tmp_path):
    """Rejections that shrink a damped step, a tiny caller radius, NaN / +inf measurements and the MAGSAC losses never put a component to
    rest; a small step at weak damping, or one that halved at the same or a growing radius, does."""
    exe = str(tmp_path / "comp_rest_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "globalsfmpy_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "comp_rest_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "PASSED" in r.stdout, r.stdout + r.stderr


def test_the_kernel_decides_through_the_rule():
    """k_comp_activity takes its decision from comp_may_rest, not from a copy of it."""
    with open(os.path.join(ROOT, "globalsfmpy_amd", "csrc", "comp_kernels.hpp")) as f:
        src = f.read()
    body = src[src.index("k_comp_activity("):src.index("k_comp_assemble(")]
    assert re.search(r"comp_may_rest\(", body)
    assert "0.5 * prev" not in body


def _check(schedule, n, active=None):
    lib = _abi.load_library()
    n = np.ascontiguousarray(n, dtype=np.uint32)
    A = np.zeros(int((n.astype(np.int64) ** 2).sum()) or 1)
    b = np.zeros(int(n.sum()) or 1)
    x = np.zeros_like(b)
    info = np.zeros(max(n.size, 1), dtype=np.int32)
    act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
    DP = C.POINTER(C.c_double)
    st = lib.gsfm_rot_dense_factor_check(schedule, n.size, n.ctypes.data_as(C.POINTER(C.c_uint32)), A.ctypes.data_as(DP), b.ctypes.data_as(DP),
                                         None if act is None else act.ctypes.data_as(C.POINTER(C.c_int32)), x.ctypes.data_as(DP), None,
                                         info.ctypes.data_as(C.POINTER(C.c_int32)))
    return st, lib.gsfm_last_error().decode()


def test_dense_factor_check_refuses_what_the_product_does_not_run():
    """The product's own limits, checked before any device call: 32 * 500 unknowns on the default schedule, 32 * 64 on the fused one, 3 * 512
    per item of a batch (the default dense_cholesky_max_cams)."""
    with open(os.path.join(ROOT, "include", "gsfm_rot.h")) as f:
        assert re.search(r"gsfm_status\s+gsfm_rot_dense_factor_check\s*\(", f.read())
    assert _check(0, [16001])[0] == GSFM_ERR_UNSUPPORTED
    assert _check(1, [2049])[0] == GSFM_ERR_UNSUPPORTED
    assert _check(2, [96, 1537])[0] == GSFM_ERR_UNSUPPORTED
    for args in ((3, [4]), (-1, [4]), (0, [4, 4]), (1, [0]), (2, [4, 0]), (0, [4], [1])):
        st, err = _check(*args)
        assert st == GSFM_ERR_INVALID_ARG, (args, st, err)
