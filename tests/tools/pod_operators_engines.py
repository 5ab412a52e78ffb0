"""Timing tool (TEST TOOL): the configs[1] mix (fixtures.config2: nodeSelector + taints, two NodePools on the kwok catalogue) with
negative node-affinity requirements on the pods — zone NotIn [one zone] on every third pod group (about a third of the pods),
capacity-type NotIn [spot] on every eighteenth (about a tenth of the pods) — on "auto-filters-spread" (the cursor engine declines a class that is not positive and the
general engine solves the batch, reason 4) and on "auto-pod-operators" (the cursor engine with pod operators, csrc/fast_engine.h
"The cursor engine's pod operators"), on the device, at each of --pods. Every repeat is a FRESH handle and the time is the host clock
around its first Solve() without result download (which ends in a device synchronise), as tests/tools/operators_engines.py
measures. Prints ONE JSON line with, per size and setting, the engine that ran, the fallback reason, the seconds per solve and
pods/s, the NodeClaims per pool, the requirements on the zone the claims print, and the Results digest; whether the digests of a size
agree (with --oracle: and equal the oracle's).
usage: python tests/tools/pod_operators_engines.py [--pods 20000,100000] [--types N] [--repeats N] [--engines a,b] [--oracle]"""
import argparse
import json

import engine_timing as et


def workload(fx, pods, types):
    """fixtures.config2 with the negative requirements; returns (problem, fraction of pods with zone NotIn, with capacity-type NotIn)."""
    prob = fx.config2(pods=pods, n_types=types, seed=42)
    n_zone = n_ct = 0
    for gi, g in enumerate(prob["podGroups"]):
        t, reqs = g["template"], []
        sel = t.get("nodeSelector", {})
        if gi % 3 == 0:
            out = fx.KWOK_ZONES[gi % 4]
            if sel.get(fx.ZONE) == out:   # (never the zone the pod pins itself to)
                out = fx.KWOK_ZONES[(gi + 1) % 4]
            reqs.append(fx.req(fx.ZONE, "NotIn", out))
            n_zone += g["count"]
        if gi % 18 == 0 and sel.get(fx.CAPACITY_TYPE) != "spot":
            reqs.append(fx.req(fx.CAPACITY_TYPE, "NotIn", "spot"))
            n_ct += g["count"]
        if reqs:
            t["nodeAffinity"] = {"required": [reqs]}
    return prob, n_zone / pods, n_ct / pods


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", default="20000,100000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--engines", default="auto-filters-spread,auto-pod-operators")
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    from karpenter_amd import fixtures as fx

    out = {"tool": "pod_operators_engines", "types": args.types, "podRequirements": ["zone NotIn [one zone] on every third pod group", "capacity-type NotIn [spot] on every eighteenth"], "sizes": {}}
    for pods in [int(x) for x in args.pods.split(",")]:
        prob, f_zone, f_ct = workload(fx, pods, args.types)
        size = {"podsWithZoneNotIn": round(f_zone, 3), "podsWithCapacityTypeNotIn": round(f_ct, 3), "engines": {}}
        want = et.oracle_digest(prob) if args.oracle else None
        for engine in args.engines.split(","):
            r, times, leg = et.timed_leg(prob, engine, args.repeats, pods=pods)
            zone_reqs = {}
            for cl in r["newNodeClaims"]:
                q = next((q for q in cl["requirements"] if q["key"] == fx.ZONE), None)
                k = "none" if q is None else f"{q['operator']} x{len(q['values'])}"
                zone_reqs[k] = zone_reqs.get(k, 0) + 1
            leg.update(claimsByPool=et.claims_by_pool(r), zoneRequirements=zone_reqs, podErrors=len(r["podErrors"]), min_s=round(min(times), 4), max_s=round(max(times), 4))
            if want is not None:
                leg["equals_oracle"] = leg["results_digest"] == want
            size["engines"][engine] = leg
        legs = size["engines"]
        size["digests_agree"] = et.digests_agree(legs)
        if "auto-filters-spread" in legs and "auto-pod-operators" in legs:
            size["fallback_over_pod_operators"] = et.over(legs, "auto-filters-spread", "auto-pod-operators")
        out["sizes"][str(pods)] = size
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
