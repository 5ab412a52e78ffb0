"""Timing tool of the spread engine's pod operators (TEST TOOL; csrc/topo_engine.h "The spread engine's pod operators"), on the device.

fixtures.config3(n_types=--types) — the BASELINE configs[2] topology mix — at each of --pods, two ways:
  * negative: every third Deployment that owns a spread constraint carries zone NotIn [one zone] as a required node-affinity term, and
    every eighteenth capacity-type NotIn [spot] — a Deployment with a zonal spread and a negative node-affinity term. One such pod
    sends the batch to the general engine under "auto-pod-operators" (26: the parent's behaviour, reason 4);
    "auto-pod-operators-spread" (29) solves it on the spread engine.
  * plain: the mix as it is, under "auto-filters-spread" (24) and 29: the new kernels (ksolve_pack_topo_p) against
    ksolve_pack_topo_f on a batch that never turns the phantom layout on.
Every solve is a FRESH handle, the time is the host clock around Solve() without result download: --repeats solves per leg after one
warm-up, then one more with Results for the digest. --oracle adds the oracle's digest of the negative batch. Prints ONE JSON line;
exit status 1 when a pair of digests differs.
usage: python tests/tools/spread_pod_operators_engines.py [--pods 20000,100000] [--types N] [--repeats N] [--variants negative,plain] [--oracle]"""
import argparse
import copy
import json
import sys

import engine_timing as et

NEGATIVE = ("auto-pod-operators", "auto-pod-operators-spread")
PLAIN = ("auto-filters-spread", "auto-pod-operators-spread")


def with_negative_terms(fx, base):
    """A Deployment is the pod groups of the mix that differ in their requests alone (one label, one spread constraint), counted in the
    order the mix lists them: zonal and hostname spreads alternate. Every third gets zone NotIn [one zone]; every eighteenth, counted
    from the third — all of them zonal spreads — capacity-type NotIn [spot]. A TopologyNodeFilter is part of a group's identity
    (topologygroup.go Hash), so every term a selector's owners carry is one more group: the seven hostname selectors and the
    anti-affinity pair are nine of the sixteen hostname groups the engine counts in one word (kTopoMaxHost), the zone term makes
    them sixteen, and a second kind of term on a hostname spread would be reason 46 — the batch would stay on the general engine."""
    prob = copy.deepcopy(base)
    deployments = {}
    for g in prob["podGroups"]:
        t = g["template"]
        if t.get("topologySpreadConstraints"):
            deployments.setdefault(repr((sorted(t["labels"].items()), t["topologySpreadConstraints"])), []).append(g)
    for d, groups in enumerate(deployments.values()):
        term = [fx.req(fx.ZONE, "NotIn", fx.KWOK_ZONES[2])] if d % 3 == 0 else [fx.req(fx.CAPACITY_TYPE, "NotIn", "spot")] if d % 18 == 2 else None
        for g in groups if term else []:
            g["template"]["nodeAffinity"] = {"required": [term]}
    return prob


def variants(fx, pods, types, which):
    out = []
    base = fx.config3(pods=pods, n_types=types)
    if "negative" in which:
        out.append((f"negative-{pods}", with_negative_terms(fx, base), NEGATIVE))
    if "plain" in which:
        out.append((f"plain-{pods}", base, PLAIN))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", default="20000,100000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--variants", default="negative,plain")
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    from karpenter_amd import fixtures as fx

    out = {"tool": "spread_pod_operators_engines", "types": args.types, "repeats": args.repeats, "cases": {}}
    for pods in [int(x) for x in args.pods.split(",")]:
        for name, prob, engines in variants(fx, pods, args.types, args.variants.split(",")):
            case = {"pods": pods, "engines": {}}
            for engine in engines:
                r, times, leg = et.timed_leg(prob, engine, args.repeats)
                leg.update(min_s=round(min(times), 4), max_s=round(max(times), 4), pops=r["counters"]["pops"], podErrors=len(r["podErrors"]))
                case["engines"][engine] = leg
            legs = case["engines"]
            want = None
            if args.oracle and name.startswith("negative"):
                want = case["oracle_digest"] = et.oracle_digest(fx.expand_pod_groups(prob))
            case["digests_agree"] = et.digests_agree(legs, want)
            case["base_over_new"] = et.over(legs, *engines)
            out["cases"][name] = case
            print(json.dumps({name: case}), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)
    return 0 if all(c["digests_agree"] for c in out["cases"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
