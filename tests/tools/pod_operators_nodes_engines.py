"""Timing tool (TEST TOOL): the configs[1] mix of tests/tools/pod_operators_engines.py (fixtures.config2 with zone NotIn [one zone] on
every third pod group and capacity-type NotIn [spot] on every eighteenth) WITH existing nodes (fixtures.with_existing_nodes), on
"auto-pod-operators-spread" (29: the existing-node stage hands a batch with negative pods to the general engine, reason 4) and on
"auto-pod-operators-nodes" (32: the stage's pod operators, csrc/node_stage.h "Pod operators beside existing nodes"), on the device, at
each of --pods x --nodes. Every repeat is a FRESH handle and the time is the host clock around its first Solve() without result
download (which ends in a device synchronise), as tests/tools/pod_operators_engines.py measures.

--positive: the same mix WITHOUT the negative requirements under both settings — identical work on ksolve_pack_nodes_lds / _hbm (29)
and on ksolve_pack_nodes_lds_p / _hbm_p (32) — on ONE handle per setting (neither falls back), with pack_kernel_ms of every solve;
--tree DIR solves with the karpenter_amd package of another checkout (the parent commit's build) for the run-to-run spread of 29 there.

Prints ONE JSON line: per size and setting the engine that ran, the fallback reason, the seconds per solve, pods/s, the pods on
existing nodes and the Results digest; whether the digests of a size agree (with --oracle: and equal the oracle's).
usage: python tests/tools/pod_operators_nodes_engines.py [--pods 20000,100000] [--nodes 1000,10000] [--types N] [--repeats N]
                                                         [--engines a,b] [--oracle] [--positive] [--tree DIR]"""
import argparse
import json
import statistics

import engine_timing as et

BELOW, SWITCH = "auto-pod-operators-spread", "auto-pod-operators-nodes"


def on_nodes(res):
    return sum(len(e["pods"]) for e in res.get("existingNodes", []))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", default="20000,100000")
    ap.add_argument("--nodes", default="1000,10000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engines", default=f"{BELOW},{SWITCH}")
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--positive", action="store_true")
    ap.add_argument("--tree")
    args = ap.parse_args()
    if args.tree:
        et.use_tree(args.tree)
    fx = et.own_fixtures("own_fixtures")
    import pod_operators_engines as po

    out = {"tool": "pod_operators_nodes_engines", "types": args.types, "positive": args.positive, "tree": args.tree or ".", "sizes": {}}
    for pods in [int(x) for x in args.pods.split(",")]:
        for nodes in [int(x) for x in args.nodes.split(",")]:
            if args.positive:
                base, f_zone, f_ct = fx.config2(pods=pods, n_types=args.types, seed=42), 0.0, 0.0
            else:
                base, f_zone, f_ct = po.workload(fx, pods, args.types)
            prob = fx.with_existing_nodes(base, nodes, seed=7)
            size = {"podsWithZoneNotIn": round(f_zone, 3), "podsWithCapacityTypeNotIn": round(f_ct, 3), "engines": {}}
            want = et.oracle_digest(prob) if args.oracle else None
            for engine in args.engines.split(","):
                if args.positive:
                    r, times, kernel = et.timed_on_one_handle(prob, engine, args.repeats)
                    import parity
                    c = r["counters"]
                    leg = {"engine": c["engine"], "engineFallbackReason": c["engineFallbackReason"], "claims": c["claims"], "solve_s": [round(x, 5) for x in times],
                           "median_s": round(statistics.median(times), 5), "pack_kernel_ms": [round(x, 4) for x in kernel], "median_pack_kernel_ms": round(statistics.median(kernel), 4),
                           "spread_pack_kernel_ms": round(max(kernel) - min(kernel), 4), "results_digest": parity.results_digest(r)[0]}
                else:
                    r, times, leg = et.timed_leg(prob, engine, args.repeats, pods=pods)
                    leg.update(min_s=round(min(times), 4), max_s=round(max(times), 4))
                leg.update(podsOnNodes=on_nodes(r), podErrors=len(r["podErrors"]), stageVariant=r["counters"]["phaseCycles"][19])
                if want is not None:
                    leg["equals_oracle"] = leg["results_digest"] == want
                size["engines"][engine] = leg
            legs = size["engines"]
            size["digests_agree"] = et.digests_agree(legs)
            if BELOW in legs and SWITCH in legs:
                size["below_over_switch"] = et.over(legs, BELOW, SWITCH)
                if args.positive:
                    size["switch_over_below_pack_kernel"] = round(legs[SWITCH]["median_pack_kernel_ms"] / legs[BELOW]["median_pack_kernel_ms"], 4)
            out["sizes"][f"{pods}x{nodes}"] = size
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
