"""Timing tool of the spread engine's pod operators beside existing nodes (TEST TOOL; csrc/topo_nodes.h "Pod operators beside existing
nodes on the spread engine"), on the device.

fixtures.config3(n_types=--types) — the BASELINE configs[2] topology mix — with the negative terms of
tests/tools/spread_pod_operators_engines.py (zone NotIn [one zone] on every third Deployment that owns a spread constraint) and
capacity-type NotIn [spot] on every tenth, counted from the third, WITH existing nodes (fixtures.with_existing_nodes), at each of
--pods x --nodes, under "auto-pod-operators-nodes" (32: the parent's behaviour — the batch goes to the general engine, reason 4) and
"auto-pod-operators-spread-nodes" (35: ksolve_pack_topo_nodes_pn), in one build. Every solve is a FRESH handle, the time is the host
clock around Solve() without result download: --repeats solves per leg after one warm-up, then one more with Results for the digest.
--oracle adds the oracle's digest. --plain: the mix WITHOUT the terms under both settings — both run ksolve_pack_topo_nodes_p, the
parent's kernel (a positive batch never launches the new one). Prints ONE JSON line; exit status 1 when a pair of digests differs.
--engines a,b picks the legs; --once makes one timed solve per leg with Results and no warm-up (the general engine takes minutes per
solve at the larger sizes).
usage: python tests/tools/spread_pod_operators_nodes_engines.py [--pods 20000,100000] [--nodes 1000,10000] [--types N] [--repeats N] [--engines a,b] [--once] [--plain] [--oracle]"""
import argparse
import copy
import json
import sys

import engine_timing as et

BELOW, SWITCH = "auto-pod-operators-nodes", "auto-pod-operators-spread-nodes"


def with_negative_terms(fx, base):
    """spread_pod_operators_engines.with_negative_terms with the capacity-type term on every tenth Deployment, counted from the third
    (all of them zonal spreads that carry no zone term)."""
    prob = copy.deepcopy(base)
    deployments = {}
    for g in prob["podGroups"]:
        t = g["template"]
        if t.get("topologySpreadConstraints"):
            deployments.setdefault(repr((sorted(t["labels"].items()), t["topologySpreadConstraints"])), []).append(g)
    for d, groups in enumerate(deployments.values()):
        term = [fx.req(fx.ZONE, "NotIn", fx.KWOK_ZONES[2])] if d % 3 == 0 else [fx.req(fx.CAPACITY_TYPE, "NotIn", "spot")] if d % 10 == 2 else None
        for g in groups if term else []:
            g["template"]["nodeAffinity"] = {"required": [term]}
    return prob


def on_nodes(res):
    return sum(len(e["pods"]) for e in res.get("existingNodes", []))


def problem(fx, pods, nodes, types, plain=False):
    base = fx.config3(pods=pods, n_types=types)
    return fx.with_existing_nodes(base if plain else with_negative_terms(fx, base), nodes, seed=7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", default="20000,100000")
    ap.add_argument("--nodes", default="1000,10000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--engines", default=f"{BELOW},{SWITCH}")
    ap.add_argument("--once", action="store_true", help="one timed solve per leg, with Results, no warm-up: for the general engine's leg at sizes where it takes minutes")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--oracle", action="store_true")
    args = ap.parse_args()
    from karpenter_amd import fixtures as fx
    import parity

    out = {"tool": "spread_pod_operators_nodes_engines", "types": args.types, "repeats": args.repeats, "plain": args.plain, "sizes": {}}
    for pods in [int(x) for x in args.pods.split(",")]:
        for nodes in [int(x) for x in args.nodes.split(",")]:
            prob = problem(fx, pods, nodes, args.types, args.plain)
            size = {"engines": {}}
            for engine in args.engines.split(","):
                if args.once:
                    r, t = et.solve_fresh(prob, engine, True)
                    times, leg = [t], {"engine": r["counters"]["engine"], "engineFallbackReason": r["counters"]["engineFallbackReason"], "claims": r["counters"]["claims"],
                                       "solve_s": [round(t, 4)], "median_s": round(t, 4), "results_digest": parity.results_digest(r)[0]}
                else:
                    r, times, leg = et.timed_leg(prob, engine, args.repeats)
                leg.update(min_s=round(min(times), 4), max_s=round(max(times), 4), podsOnNodes=on_nodes(r), podErrors=len(r["podErrors"]), pack_kernel_ms=round(r["timings"][0].get("pack_kernel_ms", -1), 3))
                size["engines"][engine] = leg
            want = None
            if args.oracle:
                want = size["oracle_digest"] = et.oracle_digest(fx.expand_pod_groups(prob))
            size["digests_agree"] = et.digests_agree(size["engines"], want)
            if BELOW in size["engines"] and SWITCH in size["engines"]:
                size["below_over_switch"] = et.over(size["engines"], BELOW, SWITCH)
            out["sizes"][f"{pods}x{nodes}"] = size
            print(json.dumps({f"{pods}x{nodes}": size}), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)
    return 0 if all(s["digests_agree"] for s in out["sizes"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
