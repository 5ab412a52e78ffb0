"""Timing tool (TEST TOOL): the benchmark's topology mix (BASELINE configs[2], fixtures.config3) over a NodePool that also carries
instance-cpu Gt 1 and instance-family NotIn [c] — what the reference's own NodePool examples carry — on "auto-operators" (no fast
engine takes a topology batch over such a pool there: the general engine, reason 0 because of the bounds) and on
"auto-operators-spread" (the spread engine's complement templates, csrc/topo_engine.h), in ONE process on the device. Per setting
one solve of a fresh handle with the results (engine, fallback reason, digest), then `--repeats` solves of fresh handles timed with
the host clock around Solve() (which ends in a device synchronise). Per size ONE JSON line — printed only after the digests of the
settings were found equal (an assertion; with --oracle: and equal to the oracle's): per setting the engine that ran, the fallback
reason, the seconds of every solve, their median and pods/s, the NodeClaims, how many of them still print the pool's own Gt / NotIn,
and the digest; then the ratio of the two medians. No ratio is asserted.
usage: python tests/tools/spread_operators_engines.py [--sizes 20000,100000] [--types N] [--repeats N] [--engines a,b] [--oracle]"""
import argparse
import json
import sys

import engine_timing as et


def problem(fx, pods, types):
    prob = fx.config3(pods=pods, n_types=types, seed=42)
    for pool in prob["nodePools"]:
        pool["requirements"] = list(pool["requirements"]) + [fx.req(fx.KWOK_CPU, "Gt", 1), fx.req(fx.KWOK_FAMILY, "NotIn", "c")]
    return prob


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--engines", default="auto-operators,auto-operators-spread")
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--solver-lib", default=None, help="a test build of the solver library (the host emulation), to try the tool without a device")
    args = ap.parse_args()
    from karpenter_amd import fixtures as fx

    for pods in (int(x) for x in args.sizes.split(",")):
        prob = problem(fx, pods, args.types)
        out = {"tool": "spread_operators_engines", "pods": pods, "types": args.types, "engines": {}}
        want = et.oracle_digest(prob) if args.oracle else None
        for engine in args.engines.split(","):
            print(f"{pods} pods, {engine}: solving", file=sys.stderr, flush=True)   # (progress, no figure: the JSON line comes last)
            r, _, leg = et.timed_leg(prob, engine, args.repeats, pods=pods, solver_lib=args.solver_lib)
            kept = sum(1 for cl in r["newNodeClaims"] if any(q["complement"] for q in cl["requirements"]))
            leg.update(claimsWithAComplementRequirement=kept, podErrors=len(r["podErrors"]))
            if want is not None:
                leg["equals_oracle"] = leg["results_digest"] == want
            out["engines"][engine] = leg
        legs = out["engines"]
        assert et.digests_agree(legs, want), {e: l["results_digest"] for e, l in legs.items()}
        out["digests_agree"] = True
        if "auto-operators" in legs and "auto-operators-spread" in legs:
            out["auto_operators_over_auto_operators_spread"] = et.over(legs, "auto-operators", "auto-operators-spread")
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
