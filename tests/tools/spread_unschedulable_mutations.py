#!/usr/bin/env python3
"""Do the tests of tests/test_spread_engine_unschedulable.py notice a wrong set-aside list, second round or kept verdict on the
spread engine? (CPU only; a tool, not a pytest test.)

Copies karpenter_amd/csrc, include/ and tests/emu to a temporary directory, applies ONE textual mutation at a time to the copy,
builds the host emulation from it and runs the checks of tests/test_spread_engine_unschedulable.py with that library: every hand
problem (named test_hand_problem[<case>]) and the tests without parameters but for the fuzz and the settings table. One line per
mutation: the checks that failed, and whether the one NAMED for the mutation is among them. A mutation whose search text does not
occur exactly once is an error of this tool (the source moved on: mend the list), never a pass; a mutation its named check does not
catch makes the exit status 1. Nothing in the tree is changed but the output file.

    python tests/tools/spread_unschedulable_mutations.py [-j N] [--out profiles/spread_unschedulable/mutations.txt]
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

os.environ.setdefault("KSOLVE_TEST_SOLVER_LIB", "1")   # a test tool: may hand a test build of the solver library to NewScheduler(solver_lib=)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

T = "topo_engine.h"
HANG = "(the checks do not end)"   # a run ended at its time limit; no mutation is named for it: retry_unschedulable bounds its pops
# (name, file under karpenter_amd/csrc, search text, replacement, the check that must catch it)
MUTATIONS = [
    ("no epoch bump on a node placement (the loop)", T,
     "if constexpr (US) epoch++;   // a pod on a node", "",
     "test_hand_problem[interleaved-nodes]"),
    ("no epoch bump on a node placement (second round)", T,
     "this->us_epoch++;   // a pod on a node", "",
     "test_hand_problem[chain-on-nodes]"),
    ("the error of the first attempt is kept", T,
     "const int r = fast_uniform(attempt(q));", "const int e0_ = F.us_err[head - 1u], d0_ = F.us_diag[head - 1u]; const int r = fast_uniform(attempt(q)); if (r == 0) { this->us_err_ = e0_; this->us_diag_ = d0_; }",
     "test_error_changes_at_the_retry"),
    ("no epoch bump on a claim commit (second round)", T,
     "this->us_epoch++;   // a pod on a claim", "",
     "test_hand_problem[chain+tail40]"),
    ("no epoch bump on a claim commit (the loop)", T,
     "if constexpr (US) epoch++;   // a pod on a claim", "",
     "test_hand_problem[interleaved]"),
    ("no epoch bump on a new claim", T,
     "if constexpr (US) this->us_epoch++;   // a new claim (and its limit subtraction): no kept verdict stands", "",
     "test_error_changes_at_the_retry"),
    ("lastLen off by one", T,
     "F.us_last[tail] = tail + 1u - head;", "F.us_last[tail] = tail - head;",
     "test_hand_problem[chain+web+big]"),
    ("the stop rule compares the original length", T,
     "if ((uint32_t)W::uniform((uint64_t)F.us_last[head]) == len) break;", "if ((uint32_t)W::uniform((uint64_t)F.us_last[head]) == (uint32_t)W::uniform((uint64_t)*F.us_n)) break;",
     "test_hand_problem[chain]"),
    ("hostname numbers not drawn on a replayed walk", T,
     "cold.host_seq += tried;", "",
     "test_hand_problem[chain+tail40]"),
    ("hostname numbers not drawn on a failed walk", T,
     "      cold.host_seq++;\n      n_ref++;\n      // CanAdd on the fresh claim", "      if (possible && possible2) cold.host_seq++;\n      n_ref++;\n      // CanAdd on the fresh claim",
     "test_hand_problem[chain]"),
    ("the claims are not counted on a replayed verdict", T,
     "(unsigned long long)order.n + (unsigned long long)tried;", "(unsigned long long)tried;",
     "test_hand_problem[chain+tail40]"),
    ("the claims are not counted when no domain is possible", T,
     "    n_ref += (unsigned long long)n;\n    LaneVar<uint64_t> zkv, zkw;", "    LaneVar<uint64_t> zkv, zkw;\n    { LaneVar<uint64_t> a_, b_; bool p_ = true, q_ = true; choose_domains(tc.zg[0], (tc.zself & 1u) != 0, cs.cvmask, a_, p_); choose_domains(tc.zg[1], (tc.zself & 2u) != 0, cs.cvmask, b_, q_); if (p_ && q_) n_ref += (unsigned long long)n; }",
     "test_hand_problem[absent-affinity]"),
    ("Topology reported as Incompatible", T,
     "return ok ? 0 : E_TOPOLOGY;", "return ok ? 0 : E_INCOMPATIBLE;",
     "test_hand_problem[absent-affinity]"),
    ("the retry skips sort_cold", T,
     "if (order.defect_claim >= 0) {   // scheduler.go:598", "if (false) {   // scheduler.go:598",
     "test_the_unschedulable_fuzz_seed_ends_on_the_spread_engine"),
    ("a success does not shorten the queue", T,
     "        if (r == 0) {\n          if (tail == cap)", "        if (r >= 0) {\n          if (tail == cap)",
     "test_hand_problem[chain]"),
]


def check(lib):
    """The checks against one library: the names of those that failed."""
    import oracle
    import test_spread_engine_unschedulable as t
    oracle.build()
    wanted = {name: oracle.solve(prob) for name, prob in t.PROBLEMS.items()}
    runs = [(f"test_hand_problem[{name}]", lambda name=name: t.test_hand_problem(oracle, lib, wanted, name)) for name in t.NAMES]
    runs += [("test_error_changes_at_the_retry", lambda: t.test_error_changes_at_the_retry(oracle, lib, wanted)),
             ("test_step_limit_inside_the_second_round", lambda: t.test_step_limit_inside_the_second_round(lib)),
             ("test_repeated_solves", lambda: t.test_repeated_solves(lib, wanted)),
             ("test_the_unschedulable_fuzz_seed_ends_on_the_spread_engine", lambda: t.test_the_unschedulable_fuzz_seed_ends_on_the_spread_engine(oracle, lib))]
    failed = []
    for name, fn in runs:
        try:
            fn()
        except Exception:   # (an assertion, or the library refusing / failing where the test expects a result)
            failed.append(name)
    print("FAILED " + " ".join(failed))


def build_and_check(work, i, mutation):
    name, fname, old, new, _ = mutation
    tree = os.path.join(work, f"m{i}")
    for d in ("karpenter_amd/csrc", "include", "tests/emu"):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(tree, d), ignore=shutil.ignore_patterns("_obj", "*.so", "*.lock", "*.tmp"))
    if old is not None:
        path = os.path.join(tree, "karpenter_amd", "csrc", fname)
        with open(path) as f:
            text = f.read()
        if text.count(old) != 1:
            return name, None, f"TOOL ERROR: the search text occurs {text.count(old)} times in {fname}"
        with open(path, "w") as f:
            f.write(text.replace(old, new))
    lib = os.path.join(tree, "libksolve_emu.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", lib, os.path.join(tree, "tests", "emu", "ksolve_emu.cpp")])
    try:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--check", lib], capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        shutil.rmtree(tree)
        return name, [HANG], ""
    shutil.rmtree(tree)
    line = next((l for l in p.stdout.splitlines() if l.startswith("FAILED")), None)
    if p.returncode != 0 or line is None:
        return name, None, f"the run ended with status {p.returncode} before every check had run"
    return name, line.split()[1:], ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="(internal) run the checks against this library")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spread_unschedulable", "mutations.txt"))
    args = ap.parse_args()
    if args.check:
        check(args.check)
        return 0
    every = [("(no mutation)", None, None, None, None)] + MUTATIONS
    with tempfile.TemporaryDirectory() as work, ThreadPoolExecutor(max_workers=args.j) as pool:
        results = list(pool.map(lambda im: build_and_check(work, *im), enumerate(every)))
    lines = []
    bad = 0
    for (name, failed, note), m in zip(results, every):
        if failed is None:
            lines.append(f"{name}: {note}")
            bad += 1
        elif m[1] is None:
            lines.append(f"{name}: " + ("clean, every check passes" if not failed else "THE UNMUTATED SOURCE FAILS " + ", ".join(failed)))
            bad += bool(failed)
        else:
            ok = m[4] in failed
            bad += not ok
            lines.append(f"{name} ({m[1]})\n    named check {m[4]}: {'caught' if ok else 'NOT CAUGHT'}; every check that failed: {', '.join(failed) or '-'}")
    lines.append(f"{len(MUTATIONS)} mutations, {bad} problems")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
