"""Record ``tests/golden/chain_dispatch.json``: which kernel every row of the chain-kernel dispatch launches (counter deltas) and
the bits it returns (SHA-256 of the H column and of v_{k+1}) for the single steps of ``tests/support/chain_dispatch_cases.py``.
Needs an MI355X; run from the repository root, at the commit whose behaviour is to be pinned:

    python tools/gen_chain_dispatch_golden.py [--out FILE] [--against FILE]

``--against FILE``: compare with an earlier recording instead of trusting one run - a case whose hashes differ between the two
keeps its counters and loses its hashes in the file written (and is named on stdout); a case whose counters differ is an error.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "chain_dispatch.json"))
    ap.add_argument("--against", default=None)
    args = ap.parse_args()
    from krypy_amd import _hip
    from tests.support import chain_dispatch_cases as cd

    ctx = _hip.get_context()
    cus = ctx.info()["compute_units"]
    out = {"compute_units": int(cus), "cases": {}}
    t00 = time.time()
    for c in cd.CASES:
        t0 = time.time()
        r = cd.run_case(ctx, c)
        out["cases"][c["name"]] = r
        print("%-55s %5.1f s  %s  h %s v %s" % (c["name"], time.time() - t0,
                                               " ".join("%s=%d" % (k[2:], v) for k, v in sorted(r["counters"].items()) if v),
                                               r["h"][:8], r["v"][:8]), flush=True)
    print("%d cases in %.1f s on %d compute units" % (len(cd.CASES), time.time() - t00, cus))
    rc = 0
    if args.against:
        with open(args.against) as f:
            other = json.load(f)["cases"]
        for name, r in out["cases"].items():
            o = other[name]
            if o["counters"] != r["counters"]:
                print("COUNTERS DIFFER run to run: %s: %r / %r" % (name, o["counters"], r["counters"]))
                rc = 1
            if (o.get("h"), o.get("v")) != (r["h"], r["v"]):
                print("not stable run to run, hashes dropped: %s" % name)
                del r["h"], r["v"]
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))
    return rc


if __name__ == "__main__":
    sys.exit(main())
