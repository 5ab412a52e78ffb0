"""Timing tool (TEST TOOL): one provisioning problem whose heavier NodePool carries a cpu limit that BINDS, on "auto" (the cursor
engine's attempt, which stops at the first exclusion with reason 23 / 24, then the general engine's re-solve), on "general" and on
"auto-limits" (the cursor engine with limit stages, csrc/fast_engine.h FastLimits), on the device. The problem is
config2(pods, types): two NodePools, `dedicated` (weight 10, tainted) and `default`. A first solve without limits says how many
NodeClaims `dedicated` opens; its limits.cpu is then set to a third of that count (and a half) times the largest cpu capacity of the catalogue —
subtractMax (scheduler.go:1049-1066) charges a claim the largest capacity it lists — so that the limit binds after roughly a third
of the pool's claims. Under "auto" a handle that fell back solves later batches on the general engine at once, so every repeat is
a FRESH handle and the time is the host clock around its first Solve() (which ends in a device synchronise); the same for the other
two settings. Prints ONE JSON line with, per setting, the engine that ran, the fallback reason, the median seconds per solve and
pods/s, the limit stages created and the claims open at the first exclusion, the NodeClaims per pool and the Results digest, and
whether the three digests agree (with --oracle: and equal the oracle's).
usage: python tests/tools/limits_engines.py [--pods N] [--types N] [--repeats N] [--engines a,b] [--oracle]"""
import argparse
import copy
import json

import engine_timing as et


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engines", default="auto,general,auto-limits")
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    from karpenter_amd import fixtures as fx

    base = fx.config2(pods=args.pods, n_types=args.types, seed=42)
    free, _ = et.solve_fresh(base, "auto", True)
    heavy = max(base["nodePools"], key=lambda p: p["weight"])["name"]
    n_heavy = sum(1 for c in free["newNodeClaims"] if c["nodePool"] == heavy)
    top_cpu = max(fx.quantity_float(it["capacity"]["cpu"]) for it in base["instanceTypes"])
    limit = int((max(1, n_heavy // 3) + 0.5) * top_cpu)   # (the half: one narrower list before the pool is used up)
    prob = copy.deepcopy(base)
    for p in prob["nodePools"]:
        if p["name"] == heavy:
            p["limits"] = {"cpu": str(limit)}
    out = {"tool": "limits_engines", "pods": args.pods, "types": args.types, "limitedPool": heavy, "limitCpu": limit,
           "claimsWithoutLimits": {"all": len(free["newNodeClaims"]), heavy: n_heavy}, "engines": {}}
    want = et.oracle_digest(prob) if args.oracle else None
    for engine in args.engines.split(","):
        r, _, leg = et.timed_leg(prob, engine, args.repeats, pods=args.pods)
        c = r["counters"]
        leg.update(claimsByPool=et.claims_by_pool(r), podErrors=len(r["podErrors"]))
        if engine in ("auto-limits", "cursor-limits") and c["engine"] == "cursor":
            v = c["phaseCycles"][23] & 0xFFFFFFFFFFFFFFFF   # stages | rows of class slots << 16 | claims at the first exclusion << 32
            leg["limitStages"] = v & 0xFFFF
            leg["claimsAtFirstExclusion"] = None if (v >> 32) == 0xFFFFFFFF else v >> 32
        if want is not None:
            leg["equals_oracle"] = leg["results_digest"] == want
        out["engines"][engine] = leg
    legs = out["engines"]
    out["digests_agree"] = et.digests_agree(legs)
    if "auto" in legs and "auto-limits" in legs:
        out["auto_over_auto_limits"] = et.over(legs, "auto", "auto-limits")
    if "general" in legs and "auto-limits" in legs:
        out["general_over_auto_limits"] = et.over(legs, "general", "auto-limits")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
