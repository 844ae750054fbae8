"""The transfer rule of csrc/host_common.hpp (DevBuf), held in the source: every fill and copy of problem memory is enqueued on a stream
the caller names; nothing uses the default stream or synchronises the device.  The separate multi-GPU libraries and the benchmark's crash
guard are not part of libgsfm_rot.so."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "globalsfmpy_amd", "csrc")
EXEMPT = {"gsfm_peer.hip", "gsfm_rccl.cpp", "bench_guard.c"}
BLOCKING = re.compile(r"hipDeviceSynchronize|hipMemcpy\(|hipMemset\(")   # (the ...Async( forms do not match)


def test_no_blocking_transfer_and_no_device_sync_in_the_library_sources():
    names = sorted(n for n in os.listdir(CSRC) if n not in EXEMPT and os.path.isfile(os.path.join(CSRC, n)))
    assert "host_common.hpp" in names and "gsfm_rot.hip" in names, names
    found = []
    for name in names:
        with open(os.path.join(CSRC, name), encoding="utf-8", errors="replace") as f:
            for no, line in enumerate(f, 1):
                if BLOCKING.search(line):
                    found.append("%s:%d: %s" % (name, no, line.strip()))
    assert not found, "\n".join(found)
