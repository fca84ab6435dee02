#!/usr/bin/env python3
"""Record tests/golden/cascade_routes.json: the cascade's route table (tests/test_gpu_cascade_routes.py) as the library
that is built in this tree reports it.

    python tests/golden/make_cascade_routes_golden.py

Needs the GPU.  Run it on a commit whose routes are known good -- the committed fixture was recorded before the host driver
(capi.hip: cascade_run_impl) was restructured, so the test holds the restructured driver to the old one's routes, counters
and outputs.  The world, the batches, the cases and what a case records are the test module's own: only data is written.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import test_gpu_cascade_routes as routes  # noqa: E402

OUT = os.path.join(HERE, "cascade_routes.json")


def main():
    world = routes.make_world()
    engine = routes.make_engine(world)
    batches = routes.make_batches(world, engine)
    passes = engine.mirge_passes()
    cases = {}
    for name, options, packed, names in routes.CASES:
        cases[name] = routes.run_case(engine, batches, passes, options, packed, names)
        print("%-28s %s" % (name, " ".join("%s:%s" % (b, "/".join(str(r[0]) for r in cases[name][b]["passes"])) for b in names)))
    engine.close()
    with open(OUT, "w") as fh:
        json.dump(dict(fields=list(routes.FIELDS), cases=cases), fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote %s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
