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
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", default="20000,100000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engines", default="auto,general,auto-operators")
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import parity
    from karpenter_amd import fixtures as fx
    from karpenter_amd.scheduling import NewScheduler

    def solve_fresh(prob, engine, want_results):
        s = NewScheduler(dict(prob, options=dict(prob["options"], engine=engine)))
        try:
            t = time.perf_counter()
            r = s.Solve(want_results=want_results)
            return r, time.perf_counter() - t
        finally:
            s.close()

    out = {"tool": "operators_engines", "types": args.types, "poolRequirements": ["instance-cpu Gt 1", "instance-family NotIn [c]"], "sizes": {}}
    for pods in [int(x) for x in args.pods.split(",")]:
        prob = fx.config2(pods=pods, n_types=args.types, seed=42)
        for p in prob["nodePools"]:
            p["requirements"] = list(p["requirements"]) + [fx.req(fx.KWOK_CPU, "Gt", 1), fx.req(fx.KWOK_FAMILY, "NotIn", "c")]
        size = {"engines": {}}
        want = None
        if args.oracle:
            import oracle
            want = parity.results_digest(oracle.solve(prob))[0]
        for engine in args.engines.split(","):
            solve_fresh(prob, engine, False)   # warm-up
            times = [solve_fresh(prob, engine, False)[1] for _ in range(args.repeats)]
            r, _ = solve_fresh(prob, engine, True)
            c = r["counters"]
            med = statistics.median(times)
            pools, cpu_reqs = {}, {}
            for cl in r["newNodeClaims"]:
                pools[cl["nodePool"]] = pools.get(cl["nodePool"], 0) + 1
                for q in cl["requirements"]:
                    if q["key"] == fx.KWOK_CPU:
                        k = f"{q['operator']} gte={q['gte']}"
                        cpu_reqs[k] = cpu_reqs.get(k, 0) + 1
            leg = {"engine": c["engine"], "engineFallbackReason": c["engineFallbackReason"], "claims": c["claims"], "claimsByPool": pools, "instanceCpuRequirements": cpu_reqs,
                   "podErrors": len(r["podErrors"]), "solve_s": [round(x, 4) for x in times], "median_s": round(med, 4), "pods_per_s": round(pods / med),
                   "results_digest": parity.results_digest(r)[0]}
            if want is not None:
                leg["equals_oracle"] = leg["results_digest"] == want
            size["engines"][engine] = leg
        legs = size["engines"]
        size["digests_agree"] = len({l["results_digest"] for l in legs.values()}) == 1
        if "auto" in legs and "auto-operators" in legs:
            size["auto_over_auto_operators"] = round(legs["auto"]["median_s"] / legs["auto-operators"]["median_s"], 2)
        if "general" in legs and "auto-operators" in legs:
            size["general_over_auto_operators"] = round(legs["general"]["median_s"] / legs["auto-operators"]["median_s"], 2)
        out["sizes"][str(pods)] = size
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
