"""Timing tool (TEST TOOL): one provisioning problem WITH existing nodes on the general engine ("general"), on "auto-nodes" and on
"cursor-nodes" (the cursor engine with its existing-node stage, csrc/node_stage.h), on the device. The problem is
with_daemonsets(with_existing_nodes(config2(pods, types), nodes), kind "a": two DaemonSets). Per engine: one warm-up solve, then
`--repeats` solves timed with the host clock around Solve() (which ends in a device synchronise); prints ONE JSON line with, per
engine, the engine that ran, the fallback reason, the memory variant of the node stage, the median seconds per solve and pods/s,
pack_kernel_ms, the counters (pods on nodes, NodeClaims, queue pops, evaluations), the Results digest, and — with --oracle —
whether the Results equal the oracle's.
The problem comes from this file's own tree; --tree DIR solves it with the karpenter_amd package of another checkout (one that
predates the node stage: only --engines general works there), so that two commits are timed on identical inputs.
usage: python tests/tools/existing_nodes_engines.py [--pods N] [--nodes N] [--types N] [--repeats N] [--engines a,b] [--tree DIR] [--oracle]"""
import argparse
import json
import os
import statistics

import engine_timing as et


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--nodes", type=int, default=2000)
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engines", default="general,auto-nodes,cursor-nodes")
    ap.add_argument("--tree", default=et.ROOT)
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    fx = et.own_fixtures("existing_nodes_fixtures")
    tree = os.path.abspath(args.tree)
    et.use_tree(tree)
    import parity
    prob = fx.with_daemonsets(fx.with_existing_nodes(fx.config2(pods=args.pods, n_types=args.types, seed=42), args.nodes, seed=42), "a")
    out = {"tool": "existing_nodes_engines", "tree": os.path.relpath(tree, et.ROOT), "pods": args.pods, "nodes": args.nodes, "types": args.types, "engines": {}}
    want = et.oracle_digest(prob) if args.oracle else None
    for engine in args.engines.split(","):
        r, times, kernel = et.timed_on_one_handle(prob, engine, args.repeats)
        c = r["counters"]
        med = statistics.median(times)
        leg = {"engine": c["engine"], "engineFallbackReason": c["engineFallbackReason"], "nodeStageVariant": c["phaseCycles"][19], "claims": c["claims"],
               "podsOnNodes": sum(len(e["pods"]) for e in r.get("existingNodes", [])), "pops": c["pops"], "binEvaluations": c["binEvaluations"],
               "referenceBinEvaluations": c["referenceBinEvaluations"], "solve_s": [round(x, 4) for x in times], "median_s": round(med, 4),
               "pods_per_s": round(args.pods / med), "pack_kernel_ms": [round(k, 3) for k in kernel], "results_digest": parity.results_digest(r)[0]}
        if want is not None:
            leg["equals_oracle"] = leg["results_digest"] == want
        out["engines"][engine] = leg
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
