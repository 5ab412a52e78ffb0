"""Timing tool (TEST TOOL): one provisioning problem WITH existing nodes AND topology groups on the general engine ("general"), on
"auto-nodes-spread" and on "spread-nodes" (the spread engine with its existing-node path, csrc/topo_nodes.h), on the device. The
problem is with_daemonsets(with_existing_nodes(config3(pods, types), nodes, seed 3), kind "c"). Per engine: one warm-up solve, then
`--repeats` solves timed with the host clock around Solve() (which ends in a device synchronise); prints ONE JSON line with, per
engine, the engine that ran, the fallback reason, the median seconds per solve, the spread (max - min) and pods/s,
pack_kernel_ms, the counters (pods on nodes, NodeClaims, queue pops, evaluations), the Results digest, and — with --oracle —
whether the Results equal the oracle's. An engine that refuses the problem is reported as {"refused": reason}.
The problem comes from this file's own tree; --tree DIR solves it with the karpenter_amd package of another checkout (one that
predates the node path: only --engines general works there), so that two commits are timed on identical inputs.
usage: python tests/tools/spread_nodes_engines.py [--pods N] [--nodes N] [--types N] [--fill lo,hi] [--repeats N] [--engines a,b] [--tree DIR] [--oracle]"""
import argparse
import json
import os
import statistics
import sys

import engine_timing as et


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--fill", default="0.2,0.9", help="lo,hi: how full the existing nodes are (fixtures.with_existing_nodes)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engines", default="general,auto-nodes-spread,spread-nodes")
    ap.add_argument("--tree", default=et.ROOT)
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    fx = et.own_fixtures("spread_nodes_fixtures")
    tree = os.path.abspath(args.tree)
    et.use_tree(tree)
    import parity
    from karpenter_amd.scheduling import Unsupported
    prob = fx.with_daemonsets(fx.with_existing_nodes(fx.config3(pods=args.pods, n_types=args.types), args.nodes, seed=3, fill=tuple(float(x) for x in args.fill.split(","))), "c")
    out = {"tool": "spread_nodes_engines", "tree": os.path.relpath(tree, et.ROOT), "pods": args.pods, "nodes": args.nodes, "fill": args.fill, "types": args.types, "engines": {}}
    want = et.oracle_digest(prob) if args.oracle else None
    for engine in args.engines.split(","):
        try:
            r, times, kernel = et.timed_on_one_handle(prob, engine, args.repeats)
        except Unsupported as e:   # "spread-nodes" refuses what "auto-nodes-spread" hands to the general engine
            out["engines"][engine] = {"refused": str(e)}
            continue
        print(f"{engine}: {[round(x, 3) for x in times]} s", file=sys.stderr, flush=True)   # (progress: the JSON line comes last)
        c = r["counters"]
        leg_errors = len(r["podErrors"])
        med = statistics.median(times)
        leg = {"engine": c["engine"], "engineFallbackReason": c["engineFallbackReason"], "claims": c["claims"], "podErrors": leg_errors,
               "podsOnNodes": sum(len(e["pods"]) for e in r.get("existingNodes", [])), "pops": c["pops"], "binEvaluations": c["binEvaluations"],
               "referenceBinEvaluations": c["referenceBinEvaluations"], "solve_s": [round(x, 4) for x in times], "median_s": round(med, 4), "spread_s": round(max(times) - min(times), 4),
               "pods_per_s": round(args.pods / med), "pack_kernel_ms": [round(k, 3) for k in kernel], "results_digest": parity.results_digest(r)[0]}
        if want is not None:
            leg["equals_oracle"] = leg["results_digest"] == want
        out["engines"][engine] = leg
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
