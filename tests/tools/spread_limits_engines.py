"""Timing tool (TEST TOOL): the benchmark's topology mix over two NodePools, the heavier of which carries a cpu limit that BINDS, on
"auto" (the spread engine's attempt, which stops at the first exclusion with reason 23 / 24, then the general engine's re-solve),
on "general" and on "spread-limits" (the spread engine with limit stages, csrc/topo_engine.h TopoEngine::limit_stage), on the
device. The problem is fixtures.config3(pods, types) with its single pool doubled: "limited" (weight 10) and "open", as
tests/spread_limit_cases.mix_problem builds it. A first solve without limits says how many NodeClaims "limited" opens; its
limits.cpu is then a third of that count (and a half) times the largest cpu capacity of the catalogue — subtractMax
(scheduler.go:1049-1066) charges a claim the largest capacity it lists — so that the limit binds after about a third of the claims.
Under "auto" a handle that fell back solves later batches on the general engine at once, so every solve is a FRESH handle: per
setting one solve with the results (engine, counters, digest), then `--repeats` solves timed with the host clock around Solve()
(which ends in a device synchronise). Per size ONE JSON line — printed only after the digests of all settings were found equal
(an assertion; with --oracle: and equal to the oracle's): per setting the engine that ran, the fallback reason, the median seconds
per solve and pods/s, the limit stages created and the claims open at the first exclusion, the NodeClaims per pool and the digest.
--tree DIR solves the same problems with the karpenter_amd package of another checkout (one that predates engines 13 / 14: only
"auto" and "general" work there), so that two commits are timed on identical inputs.
usage: python tests/tools/spread_limits_engines.py [--sizes 20000,100000] [--types N] [--repeats N] [--engines a,b] [--tree DIR] [--oracle]"""
import argparse
import json
import os
import sys

import engine_timing as et


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--engines", default="auto,general,spread-limits")
    ap.add_argument("--tree", default=et.ROOT)
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    et.use_tree(tree)
    import spread_limit_cases as sl   # (this file's own tree has it, whichever package solves the problems)
    fx = sl.fx

    for pods in (int(x) for x in args.sizes.split(",")):
        cfg = (pods, args.types, 42)
        free, _ = et.solve_fresh(sl.mix_problem(cfg, None), "auto", True)
        assert free["counters"]["engine"] == "spread", free["counters"]
        n_heavy = sum(1 for c in free["newNodeClaims"] if c["nodePool"] == "limited")
        top_cpu = max(fx.quantity_float(it["capacity"]["cpu"]) for it in fx.config3(pods=5, n_types=args.types, seed=42)["instanceTypes"])
        limit = int((max(1, n_heavy // 3) + 0.5) * top_cpu)   # (the half: one narrower list before the pool is used up)
        prob = sl.mix_problem(cfg, {"cpu": str(limit)})
        out = {"tool": "spread_limits_engines", "tree": os.path.relpath(tree, et.ROOT), "pods": pods, "types": args.types, "limitCpu": limit,
               "claimsWithoutLimits": {"all": len(free["newNodeClaims"]), "limited": n_heavy}, "engines": {}}
        want = et.oracle_digest(prob) if args.oracle else None
        for engine in args.engines.split(","):
            print(f"{pods} pods, {engine}: solving", file=sys.stderr, flush=True)   # (progress, no figure: the JSON line comes last)
            r, _, leg = et.timed_leg(prob, engine, args.repeats, pods=pods)
            leg.update(claimsByPool=et.claims_by_pool(r), podErrors=len(r["podErrors"]))
            if leg["engine"] == "spread" and engine in ("spread-limits", "auto-limits-spread"):
                leg["limitStages"], leg["claimsAtFirstExclusion"] = sl.stages(r)
            if want is not None:
                leg["equals_oracle"] = leg["results_digest"] == want
            out["engines"][engine] = leg
        legs = out["engines"]
        assert et.digests_agree(legs, want), {e: l["results_digest"] for e, l in legs.items()}
        out["digests_agree"] = True
        if "auto" in legs and "spread-limits" in legs:
            out["auto_over_spread_limits"] = et.over(legs, "auto", "spread-limits")
        if "general" in legs and "spread-limits" in legs:
            out["general_over_spread_limits"] = et.over(legs, "general", "spread-limits")
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
