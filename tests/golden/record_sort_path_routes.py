"""Records tests/golden/sort_path_routes.json: every case of tests/sort_path_routes.py, run twice through the public Python API on one GPU; a field that
differs between the two runs is refused (it depends on scheduling and pins nothing) and counted in the last line printed.  Run from the repository root
on the commit whose behaviour is the reference:  python tests/golden/record_sort_path_routes.py [case ...]   (cases given: only those are run and
printed, nothing is written)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository

import sort_path_routes as routes      # noqa: E402


def _fields(rec):
    return {(i, f): v for i, r in enumerate(rec if isinstance(rec, list) else [rec]) for f, v in r.items()}


def main(argv):
    names = argv or routes.ALL_CASES
    out, refused = {}, []
    for name in names:
        a, b = routes.run_case(name), routes.run_case(name)
        fa, fb = _fields(a), _fields(b)
        refused += [(name,) + key for key in sorted(set(fa) | set(fb)) if fa.get(key) != fb.get(key)]
        out[name] = a
        print(name, json.dumps(a), flush=True)
    print("fields refused (they differ between two runs on the same commit): %d %r" % (len(refused), refused), flush=True)
    if refused:
        raise SystemExit(1)
    if not argv:
        with open(os.path.join(HERE, "sort_path_routes.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
