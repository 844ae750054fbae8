#!/usr/bin/env python3
"""Records what the entries that take cameras and a track CSR answer to the calls of tests/track_refusals.py -- status, message and what
they left in their outputs -- for tests/test_track_refusals.py.  Run on a machine without a device (every check runs before the device is
looked up; a valid scene then ends in GSFM_ERR_NO_DEVICE) with GSFM_ROT_LIB pointing at a library built from the commit whose answers are
to be kept (the one before the track front ends moved to csrc/track_scene.hpp):

    GSFM_ROT_LIB=/path/to/parent/libgsfm_rot.so python tools/make_track_refusals_golden.py

Writes tests/golden/track_refusals.json: a list of {entry, case, status, message, outputs}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from globalsfmpy_amd import _abi  # noqa: E402
import track_refusals as TR  # noqa: E402


def main():
    print("library: %s" % _abi.LIB_PATH)
    lib = _abi.load_library()
    rows = []
    for entry, case, over in TR.cases():
        status, message, outputs = TR.replay(lib, entry, over)
        rows.append({"entry": entry, "case": case, "status": status, "message": message, "outputs": outputs})
        print("%-32s %-48s %d %s" % (entry, case, status, message))
    assert len({(r["entry"], r["case"]) for r in rows}) == len(rows), "two cases of one name"
    assert not any(r["status"] == _abi.OK and r["case"].startswith("valid scene") for r in rows), "record on a machine without a device"
    path = os.path.join(ROOT, "tests", "golden", "track_refusals.json")
    with open(path, "w") as f:
        json.dump(rows, f, indent=0)
    print("%d calls -> %s" % (len(rows), path))


if __name__ == "__main__":
    main()
