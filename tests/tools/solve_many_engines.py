"""K topology problems at once, three ways (TEST TOOL, device only; built on engine_timing.py): K in {16, 64, 256} members of
fixtures.config3(pods=20000, n_types=144, seed=...) under "auto-filters-spread" —
  (a) lone     K Solve() calls in sequence                     (the parent's path)
  (b) batch    one SolveBatch                                  (the parent's path: under this setting every member keeps a set-aside
               list, so solve_batch_plain solves each one alone through solve(), on the spread engine, one after another)
  (c) many     one SolveMany                                   (this tree: the spread engine's many-problem launch)
Fresh handles per repeat, one warm-up, the median of five, the host clock around the call(s) without result download; one more run
with Results for every member's digest. A process loads one karpenter_amd package, so every (leg, K) is a child process of its own;
the driver starts them one after another, the parent checkout's legs alternating with this tree's:
  python tests/tools/solve_many_engines.py --parent PATH_TO_PARENT_CHECKOUT --out profiles/solve_many/solve_many_engines.json
  python tests/tools/solve_many_engines.py --leg many --k 64            (one child; prints one JSON line)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import engine_timing as et

SETTING = "auto-filters-spread"
KS = (16, 64, 256)
REPEATS = 5


def child(leg, k, tree, pods):
    if tree:
        et.use_tree(tree)
    fx = et.own_fixtures("own_fixtures")
    import parity
    from karpenter_amd import scheduling as sch
    probs = [fx.config3(pods=pods, n_types=144, seed=100 + i) for i in range(k)]
    probs = [dict(p, options=dict(p["options"], engine=SETTING)) for p in probs]

    def once(want_results):
        scheds = [sch.NewScheduler(p) for p in probs]
        try:
            stats = {}
            t = time.perf_counter()
            if leg == "lone":
                res = [s.Solve(want_results=want_results) for s in scheds]
            elif leg == "batch":
                res = sch.SolveBatch(scheds, want_results=want_results)
            else:
                res = sch.SolveMany(scheds, want_results=want_results, stats=stats)
            return res, time.perf_counter() - t, stats
        finally:
            for s in scheds:
                s.close()

    once(False)
    runs = [once(False) for _ in range(REPEATS)]
    times = [r[1] for r in runs]
    res, _, stats = once(True)
    pack = [r["timings"][0]["pack_kernel_ms"] for r in runs[-1][0]]
    out = {"leg": leg, "k": k, "pods": pods, "tree": "parent checkout" if tree else "this tree", "solve_s": [round(x, 4) for x in times], "median_s": round(statistics.median(times), 4),
           "spread_s": round(max(times) - min(times), 4), "engines": sorted({r["counters"]["engine"] for r in res}),
           "pack_kernel_ms_max": round(max(pack), 3), "pack_kernel_ms_sum": round(sum(pack), 3), "stats": stats,
           "digests": [parity.results_digest(r)[0] for r in res]}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["lone", "batch", "many"])
    ap.add_argument("--k", type=int)
    ap.add_argument("--tree")
    ap.add_argument("--parent")
    ap.add_argument("--pods", type=int, default=20000)
    ap.add_argument("--ks", default=",".join(map(str, KS)))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg:
        child(args.leg, args.k, args.tree, args.pods)
        return
    if not args.parent:
        ap.error("--parent: a built checkout of the parent commit (legs a and b are its paths)")
    doc = {"setting": SETTING, "pods": args.pods, "repeats": REPEATS, "legs": []}
    ok = True
    for k in [int(x) for x in args.ks.split(",")]:
        legs = {}
        for leg, tree in (("lone", args.parent), ("many", None), ("batch", args.parent)):   # (parent, this tree, parent)
            print(f"solve_many_engines: K = {k}, leg {leg} ...", file=sys.stderr, flush=True)
            cmd = [sys.executable, __file__, "--leg", leg, "--k", str(k), "--pods", str(args.pods)] + (["--tree", tree] if tree else [])
            line = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=900).stdout.strip().splitlines()[-1]
            legs[leg] = json.loads(line)
        agree = legs["lone"]["digests"] == legs["batch"]["digests"] == legs["many"]["digests"]
        spread = max(v["spread_s"] for v in legs.values())
        faster = legs["many"]["median_s"] + spread < min(legs["lone"]["median_s"], legs["batch"]["median_s"])
        summary = {"k": k, "digests_agree": agree, "largest_spread_s": spread, "many_faster_than_both_by_more_than_the_spread": faster,
                   "outside_the_pack_launch_s": round(legs["many"]["median_s"] - legs["many"]["pack_kernel_ms_max"] / 1e3, 4)}
        for v in legs.values():
            v.pop("digests")
        doc["legs"].append(dict(summary, **legs))
        print(json.dumps(dict(summary, **{n: (v["median_s"], v["pack_kernel_ms_max"]) for n, v in legs.items()})), flush=True)
        ok = ok and agree
    if args.out:
        if os.path.exists(args.out):   # a K measured in an earlier session stays (--ks 256 alone is a quarter of an hour): this run's replace their own
            with open(args.out) as f:
                old = json.load(f)
            if (old.get("setting"), old.get("pods"), old.get("repeats")) == (SETTING, args.pods, REPEATS):
                mine = {leg["k"] for leg in doc["legs"]}
                doc["legs"] = sorted([leg for leg in old["legs"] if leg["k"] not in mine] + doc["legs"], key=lambda leg: leg["k"])
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
