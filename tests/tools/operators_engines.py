"""Timing tool (TEST TOOL): the configs[1] mix (fixtures.config2: nodeSelector + taints, two NodePools on the kwok catalogue) with
the requirements the NodePool examples carry — instance-cpu Gt 1 and instance-family NotIn [c] on BOTH pools — on "auto" (the host
finds the bounds and the general engine solves the batch, reason 1), on "general" and on "auto-operators" (the cursor engine with
complement templates, csrc/fast_engine.h FastCold::setup), on the device, at each of --pods. Every repeat is a FRESH handle and the
time is the host clock around its first Solve() without result download (which ends in a device synchronise), as
tests/tools/limits_engines.py measures. Prints ONE JSON line with, per size and setting, the engine that ran, the fallback reason,
the seconds per solve and pods/s, the NodeClaims per pool, the requirement on instance-cpu the claims print, and the Results digest;
whether the digests of a size agree (with --oracle: and equal the oracle's).
usage: python tests/tools/operators_engines.py [--pods 20000,100000] [--types N] [--repeats N] [--engines a,b] [--oracle]"""
import argparse
import json

import engine_timing as et


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", default="20000,100000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engines", default="auto,general,auto-operators")
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    from karpenter_amd import fixtures as fx

    out = {"tool": "operators_engines", "types": args.types, "poolRequirements": ["instance-cpu Gt 1", "instance-family NotIn [c]"], "sizes": {}}
    for pods in [int(x) for x in args.pods.split(",")]:
        prob = fx.config2(pods=pods, n_types=args.types, seed=42)
        for p in prob["nodePools"]:
            p["requirements"] = list(p["requirements"]) + [fx.req(fx.KWOK_CPU, "Gt", 1), fx.req(fx.KWOK_FAMILY, "NotIn", "c")]
        size = {"engines": {}}
        want = et.oracle_digest(prob) if args.oracle else None
        for engine in args.engines.split(","):
            r, _, leg = et.timed_leg(prob, engine, args.repeats, pods=pods)
            cpu_reqs = {}
            for cl in r["newNodeClaims"]:
                for q in cl["requirements"]:
                    if q["key"] == fx.KWOK_CPU:
                        k = f"{q['operator']} gte={q['gte']}"
                        cpu_reqs[k] = cpu_reqs.get(k, 0) + 1
            leg.update(claimsByPool=et.claims_by_pool(r), instanceCpuRequirements=cpu_reqs, podErrors=len(r["podErrors"]))
            if want is not None:
                leg["equals_oracle"] = leg["results_digest"] == want
            size["engines"][engine] = leg
        legs = size["engines"]
        size["digests_agree"] = et.digests_agree(legs)
        if "auto" in legs and "auto-operators" in legs:
            size["auto_over_auto_operators"] = et.over(legs, "auto", "auto-operators")
        if "general" in legs and "auto-operators" in legs:
            size["general_over_auto_operators"] = et.over(legs, "general", "auto-operators")
        out["sizes"][str(pods)] = size
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
