"""Tool of the spread engine's unschedulable pods (TEST TOOL; csrc/topo_engine.h "The spread engine's unschedulable pods"), two uses.

1. Timing, on the device: topology batches with pods the first round cannot place, under "auto-unschedulable" (20: the spread engine
   stops at the first such pod, reason 27, and the general engine solves the batch again) against "auto-unschedulable-spread" (22:
   the spread engine sets the pods aside and retries them). fixtures.config3(n_types=--types) at each of --pods in three variants:
     * big:    1% of the pods replaced by one 10,000-cpu class (the head of the queue; InstanceTypes);
     * limit:  a cpu limit on the pool that is used up after about a third of the claims the batch opens without it (Limits);
     * chain:  5% of the pods in an affinity chain a -> b -> c whose targets sort behind them (placed by the second round).
   Every solve is a FRESH handle, the time is the host clock around Solve() without result download: --repeats solves per leg after
   one warm-up, then one more with Results for the digest. Prints ONE JSON line.
   usage: python tests/tools/spread_unschedulable_engines.py [--pods 20000,100000] [--types N] [--repeats N] [--variants big,limit,chain]

2. --record-parent REV: builds the host emulation of commit REV in a scratch copy (git archive; nothing in the tree is touched but
   the output file), solves PARENT_CASES under every NAMED setting of that commit's engine table and writes
   {case: {name: [engine, reason, digest] | ["refused", text]}} to tests/golden/spread_unschedulable_parent.json — what
   test_spread_engine_unschedulable.test_settings_0_to_21_are_unchanged compares the tree with."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

import engine_timing as et

ROOT = et.ROOT
ENGINES = ("auto-unschedulable", "auto-unschedulable-spread")
PARENT_CASES = ["spread+big", "chain", "limits"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "spread_unschedulable_parent.json")


def canonical(prob):
    """The problem with its pods' uids (and names) numbered by position: fixtures.pod draws uids from a process-wide counter, and
    the Results digest covers them."""
    pods = [dict(p, uid=f"00000000-0000-0000-0000-{i + 1:012d}", name=f"pod-{i + 1}") for i, p in enumerate(prob["pods"])]
    return dict(prob, pods=pods)


def settings_table(lib, prob, names):
    """{name: [engine, reason, digest]} of one problem (uids canonical) under each engine name; a refusal reads ["refused", its text]."""
    import parity
    from karpenter_amd.scheduling import NewScheduler, Unsupported
    out = {}
    prob = canonical(prob)
    for name in names:
        s = NewScheduler(dict(prob, options=dict(prob.get("options", {}), engine=name)), solver_lib=lib)
        try:
            r = s.Solve()
            out[name] = [r["counters"]["engine"], r["counters"]["engineFallbackReason"], parity.results_digest(r)[0]]
        except Unsupported as e:
            out[name] = ["refused", str(e)]
        finally:
            s.close()
    return out


def setting_names(header_text):
    """The names of the engine table's rows, in row order (a row without a name has none)."""
    return re.findall(r'^\s*/\*\s*\d+\s*\*/\s*\{.*?"([a-z-]+)"\},', header_text, re.M)


def record_parent(rev):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import spread_unschedulable_cases as suc
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "karpenter_amd/csrc", "include", "tests/emu"], check=True, stdout=subprocess.PIPE).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        lib = os.path.join(tmp, "libksolve_emu.so")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", lib, os.path.join(tmp, "tests", "emu", "ksolve_emu.cpp")])
        with open(os.path.join(tmp, "karpenter_amd", "csrc", "engine_setting.h")) as f:
            names = setting_names(f.read())
        problems = {n: p for n, p, _ in suc.hand_problems()}
        golden = {case: settings_table(lib, problems[case], names) for case in PARENT_CASES}
    with open(GOLDEN, "w") as f:
        json.dump(golden, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{GOLDEN}: {len(names)} settings of {rev} x {len(PARENT_CASES)} cases")
    return 0


def variants(fx, pods, types, which):
    from karpenter_amd.scheduling import NewScheduler
    out = []
    if "big" in which:
        bad = pods // 100
        prob = fx.config3(pods=pods - bad, n_types=types)
        prob["podGroups"] = prob["podGroups"] + [{"count": bad, "uidSeed": 7101, "template": fx.pod(uid="t", requests={"cpu": "10000", "memory": "1Gi"})}]
        out.append((f"big-{pods}", prob))
    if "limit" in which:
        prob = fx.config3(pods=pods, n_types=types)
        s = NewScheduler(dict(prob, options=dict(prob["options"], engine="auto")))
        try:
            claims = s.Solve(want_results=False)["counters"]["claims"]
        finally:
            s.close()
        top = max(fx.quantity_float(it["capacity"]["cpu"]) for it in prob["instanceTypes"])   # subtractMax charges the largest type a claim lists
        prob["nodePools"][0]["limits"] = {"cpu": str(int(claims // 3 * top))}
        out.append((f"limit-{pods}", prob))
    if "chain" in which:
        n = pods // 20
        prob = fx.config3(pods=pods - n, n_types=types)
        third = n // 3
        mk = lambda lab, cpu, **kw: fx.pod(uid="t", requests={"cpu": cpu, "memory": "300Mi"}, labels={"chain": lab}, **kw)
        prob["podGroups"] = prob["podGroups"] + [
            {"count": third, "uidSeed": 7201, "template": mk("a", "1400m", pod_requirements=[fx.affinity_term(fx.ZONE, {"chain": "b"})])},
            {"count": third, "uidSeed": 7202, "template": mk("b", "900m", pod_requirements=[fx.affinity_term(fx.ZONE, {"chain": "c"})])},
            {"count": n - 2 * third, "uidSeed": 7203, "template": mk("c", "300m", node_selector={fx.ZONE: fx.KWOK_ZONES[0]})}]
        out.append((f"chain-{pods}", prob))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", default="20000,100000")
    ap.add_argument("--types", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--variants", default="big,limit,chain")
    ap.add_argument("--record-parent", default=None, metavar="REV")
    args = ap.parse_args()
    if args.record_parent:
        return record_parent(args.record_parent)
    from karpenter_amd import fixtures as fx
    out = {"tool": "spread_unschedulable_engines", "types": args.types, "repeats": args.repeats, "cases": {}}
    for pods in [int(x) for x in args.pods.split(",")]:
        for name, prob in variants(fx, pods, args.types, args.variants.split(",")):
            case = {"pods": pods, "engines": {}}
            for engine in ENGINES:
                r, _, leg = et.timed_leg(prob, engine, args.repeats)
                leg.update(pops=r["counters"]["pops"], podErrors={str(k): v for k, v in sorted(Counter(e["code"] for e in r["podErrors"].values()).items())})
                case["engines"][engine] = leg
            legs = case["engines"]
            case["digests_agree"] = et.digests_agree(legs)
            case["pops_agree"] = len({l["pops"] for l in legs.values()}) == 1
            case["base_over_spread_unschedulable"] = et.over(legs, *ENGINES)
            out["cases"][name] = case
            print(json.dumps({name: case}), file=sys.stderr, flush=True)
    print(json.dumps(out), flush=True)
    return 0 if all(c["digests_agree"] and c["pops_agree"] for c in out["cases"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
