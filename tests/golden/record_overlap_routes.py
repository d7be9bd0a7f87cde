"""Records tests/golden/overlap_routes.json: every case of tests/overlap_routes.py, run twice through the public Python API on one GPU; a field that
differs between the two runs is refused (it depends on scheduling and pins nothing).  Run from the repository root on the commit whose behaviour is the
reference:  python tests/golden/record_overlap_routes.py [--out FILE] [case ...]   (cases given without --out: only those are run and printed,
nothing is written)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository

import overlap_routes as routes      # noqa: E402


def main(argv):
    out_path = None
    if argv[:1] == ["--out"]:
        out_path, argv = argv[1], argv[2:]
    names = argv or routes.ALL_CASES
    out = {}
    for name in names:
        a, b = routes.run_case(name), routes.run_case(name)
        if a != b:
            raise SystemExit("case %s differs between two runs on the same commit: %r / %r" % (name, a, b))
        out[name] = a
        print(name, json.dumps(a), flush=True)
    if out_path or not argv:
        with open(out_path or os.path.join(HERE, "overlap_routes.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
