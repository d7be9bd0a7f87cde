"""Records tests/golden/csr_build_routes.json: every case of tests/csr_build_routes.py, run twice through the public Python API on one GPU.  A field that
differs between the two runs is refused: it depends on scheduling and pins nothing, so it is left out of the fixture and named on the last line.  Run
from the repository root on the commit whose behaviour is the reference:  python tests/golden/record_csr_build_routes.py [case ...]   (cases given:
only those are run and printed, nothing is written)"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                    # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the repository

import csr_build_routes as routes      # noqa: E402


def _agreed(name, a, b, refused):
    if isinstance(a, list):
        return [_agreed("%s[%d]" % (name, i), x, y, refused) for i, (x, y) in enumerate(zip(a, b))]
    refused += ["%s.%s" % (name, f) for f in a if a[f] != b.get(f)]
    return {f: a[f] for f in a if a[f] == b.get(f)}


def main(argv):
    names = argv or routes.ALL_CASES
    out, refused = {}, []
    for name in names:
        out[name] = _agreed(name, routes.run_case(name), routes.run_case(name), refused)
        print(name, json.dumps(out[name]), flush=True)
    if not argv:
        with open(os.path.join(HERE, "csr_build_routes.json"), "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    print("refused (differ between two runs):", ", ".join(refused) or "none", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
