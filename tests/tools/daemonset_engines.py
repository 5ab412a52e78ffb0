"""Timing tool (TEST TOOL): DaemonSet problems on the fast engines against the general engine, on the device. For a given size it solves
with_daemonsets(config2) and with_daemonsets(config3) on `auto` and on engine="general", and the same problems without DaemonSets on
`auto`; prints ONE JSON line with, per leg, the engine that ran, the fallback reason, pack_kernel_ms, seconds per solve (host clock
around Solve(), which ends in a device synchronise; one warm-up solve first), the NodeClaim count and the Results digest.
The problems come from this file's own tree; --tree DIR solves them with the karpenter_amd package of another checkout (one
that predates fixtures.with_daemonsets), so that two commits are timed on identical inputs.
usage: python tests/tools/daemonset_engines.py [--pods N] [--types N] [--kind a|b|c] [--repeats N] [--tree DIR] [--skip-general]"""
import argparse
import json
import os

import engine_timing as et


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100000)
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--kind", default="c")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tree", default=et.ROOT)
    ap.add_argument("--skip-general", action="store_true")
    args = ap.parse_args()
    fx = et.own_fixtures("daemonset_fixtures")
    tree = os.path.abspath(args.tree)
    et.use_tree(tree)
    import parity
    out = {"tool": "daemonset_engines", "tree": os.path.relpath(tree, et.ROOT), "pods": args.pods, "types": args.types, "kind": args.kind, "legs": {}}
    shapes = {"config2": fx.config2(pods=args.pods, n_types=args.types, seed=42), "config3": fx.config3(pods=args.pods, n_types=args.types, seed=42)}
    for shape, base in shapes.items():
        legs = [("daemonsets_auto", fx.with_daemonsets(base, args.kind), "auto"), ("plain_auto", base, "auto")]
        if not args.skip_general:
            legs.insert(1, ("daemonsets_general", fx.with_daemonsets(base, args.kind), "general"))
        for leg, prob, engine in legs:
            r, times, kernel = et.timed_on_one_handle(prob, engine, args.repeats)
            out["legs"][f"{shape}.{leg}"] = {"engine": r["counters"]["engine"], "engineFallbackReason": r["counters"]["engineFallbackReason"], "claims": r["counters"]["claims"],
                                            "pack_kernel_ms": [round(k, 3) for k in kernel], "solve_s": [round(x, 4) for x in times],
                                            "results_digest": parity.results_digest(r)[0]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
