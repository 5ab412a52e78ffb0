"""Timing tool (TEST TOOL): batches that leave pods unschedulable, under "auto-operators-spread" (18: the cursor engine stops at the
first such pod, reason 27, and the general engine solves the batch again) against "auto-unschedulable" (20: the cursor engine sets
the pods aside, csrc/fast_engine.h "Unschedulable pods"), on the device:
  * fixtures.config1 at each of --pods with 1% and 10% of the pods unschedulable — half of them one oversized class (the head of the
    queue), half one class that selects an absent zone (its tail);
  * fixtures.config2(pods=100000, n_types=--types) with cpu limits on BOTH pools, so that the batch ends unschedulable (15% and 55% of the batch's cpu request).
Every solve is a FRESH handle and the time is the host clock around its Solve() without result download (which ends in a device
synchronise), as tests/tools/limits_engines.py measures: --repeats solves per leg after one warm-up, then one more with Results for the
digest. Prints ONE JSON line: per case and setting the engine that ran, the fallback reason, pops, pod errors by code, the seconds of
each solve and their median, the Results digest; whether the digests of a case agree, and the ratio of the medians.
usage: python tests/tools/unschedulable_engines.py [--pods 20000,100000] [--types N] [--repeats N]"""
import argparse
import json
import sys
from collections import Counter

import engine_timing as et

ENGINES = ("auto-operators-spread", "auto-unschedulable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", default="20000,100000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from karpenter_amd import fixtures as fx

    cases = []
    for pods in [int(x) for x in args.pods.split(",")]:
        for percent in (1, 10):
            bad = pods * percent // 100
            prob = fx.config1(pods=pods - bad)
            prob["podGroups"] = prob["podGroups"] + [
                {"count": bad // 2, "uidSeed": 7001, "template": fx.pod(uid="t", requests={"cpu": "10000", "memory": "1Gi"})},
                {"count": bad - bad // 2, "uidSeed": 7002, "template": fx.pod(uid="t", requests={"cpu": "1m"}, node_selector={fx.ZONE: "no-such-zone"})}]
            cases.append((f"config1-{pods}-{percent}pct", pods, prob))
    prob = fx.config2(pods=100000, n_types=args.types, seed=42)
    total_m = sum(g["count"] * fx.quantity_float(g["template"]["requests"]["cpu"]) * 1000 for g in prob["podGroups"])
    for p, share in zip(prob["nodePools"], (0.15, 0.55)):   # the pools' claims may list types worth 70% of the batch's cpu request: the rest is unschedulable
        p["limits"] = {"cpu": f"{int(total_m * share)}m"}
    cases.append(("config2-100000-limits", 100000, prob))

    out = {"tool": "unschedulable_engines", "types": args.types, "repeats": args.repeats, "cases": {}}
    for name, pods, prob in cases:
        case = {"pods": pods, "engines": {}}
        for engine in ENGINES:
            r, _, leg = et.timed_leg(prob, engine, args.repeats, pods=pods)
            leg.update(pops=r["counters"]["pops"], podErrors={str(k): v for k, v in sorted(Counter(e["code"] for e in r["podErrors"].values()).items())})
            case["engines"][engine] = leg
        legs = case["engines"]
        case["digests_agree"] = et.digests_agree(legs)
        case["base_over_unschedulable"] = et.over(legs, *ENGINES)
        out["cases"][name] = case
    print(json.dumps(out), flush=True)
    return 0 if all(c["digests_agree"] for c in out["cases"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
