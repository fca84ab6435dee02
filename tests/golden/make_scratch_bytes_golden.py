#!/usr/bin/env python3
"""Record tests/golden/scratch_bytes.json: what every mrg_*_temp_bytes call of the stages with a carved scratch returns,
as the library that is built in this tree reports it.

    python tests/golden/make_scratch_bytes_golden.py

Needs no GPU.  Run it on a commit whose scratch layouts are known good -- the committed fixture was recorded on the commit
before the layout structs of capi.hip were rewritten on the one carver, so tests/test_scratch_bytes_native.py holds the
rewritten layouts to the old ones' sizes.  The calls, the sizes and the limits are the test module's own: only data is
written.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import test_scratch_bytes_native as sizes  # noqa: E402

OUT = os.path.join(HERE, "scratch_bytes.json")


def main():
    from mirge_amd import _native
    calls = sizes.record(_native.load())
    with open(OUT, "w") as fh:
        json.dump(dict(sizes=list(sizes.SIZES), limits={k: list(v) for k, v in sizes.LIMITS.items()}, calls=calls), fh,
                  separators=(",", ":"))
        fh.write("\n")
    print("wrote %s: %d calls, %d values, %d bytes" % (OUT, len(calls), sum(len(v) for v in calls.values()), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
