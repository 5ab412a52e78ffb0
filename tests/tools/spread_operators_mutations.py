#!/usr/bin/env python3
"""Do the tests of tests/test_spread_engine_operators.py notice a wrong treatment of complement templates on the spread engine?
(CPU only; a tool, not a pytest test.)

Copies karpenter_amd/csrc, include/ and tests/emu to a temporary directory, applies ONE textual mutation at a time to the copy,
builds the host emulation from it and calls every test function of tests/test_spread_engine_operators.py with that library. One
line per mutation: the tests that failed, and whether the test NAMED for the mutation is among them. A mutation whose search text
does not occur exactly once is an error of this tool (the source moved on: mend the list), never a pass; a mutation its named test
does not catch makes the exit status 1.

    python tests/tools/spread_operators_mutations.py [-j N] [--out profiles/spread_operators/mutations.txt]
"""
import argparse
import inspect
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

# (name, file under karpenter_amd/csrc, search text, replacement, the test that must catch it)
MUTATIONS = [
    ("record_zonal ignores the guard bit", "topo_engine.h",
     "if ((m2 >> (off + width)) & 1) continue;", "",
     "test_counted_but_not_narrowed"),
    ("a limit stage drops the guard bits", "fast_engine.h",
     "Mp->tvmask[s] = (Mp->tvmask[t] & ~(0xFFull << 56)) | ((uint64_t)s << 56);",
     "{ const FastVar fv_ = *F.var; uint64_t gm_ = 0; for (int j_ = 0; j_ < fv_.nv; ++j_) gm_ |= 1ull << (fv_.voff[j_] + fv_.vwidth[j_]); "
     "Mp->tvmask[s] = (Mp->tvmask[t] & ~gm_ & ~(0xFFull << 56)) | ((uint64_t)s << 56); }",
     "test_limit_stages"),
    ("plain_topo accepts pod-side bounds", "ksolve_impl.h",
     "const bool no_topo_bounds = h->eng.spread_operators ? !pod_bounds : no_bounds;", "const bool no_topo_bounds = h->eng.spread_operators ? true : no_bounds;",
     "test_still_outside_the_shape"),
    ("the records kernel prints the field of a guarded claim", "fast_engine.h",
     "if (own) { if (!(tr.defined & kb)) vdef &= ~kb; }",
     "if (own && !(tr.defined & kb)) vdef &= ~kb;",
     "test_counted_but_not_narrowed"),   # (the claims that must still print NotIn [test-zone-1, test-zone-2]; in operator_cases.spread_problem() a spread pod narrows every claim of the pool)
    ("a spread handle of every setting accepts complement templates", "ksolve_impl.h",
     "fw.ops = h->eng.spread_operators ? 1 : 0;", "fw.ops = 1;",
     "test_old_settings_stay_as_they_are"),
    ("the batch path forgets the complement templates", "solve_calls.h",
     "(h->daemon_groups || h->tw.nd.dom || h->spread_complement || h->fw.unsched)", "(h->daemon_groups || h->tw.nd.dom || h->fw.unsched)",
     "test_in_a_batch"),
    ("with existing nodes the templates' bounds still decline", "ksolve_impl.h",
     "uint32_t why = nodes_decline(common && no_topo_bounds);", "uint32_t why = nodes_decline(common && no_bounds);",
     "test_existing_nodes"),
    ("setup() declines complement templates on behalf of the spread engine", "fast_engine.h",
     "const bool ops = F.ops != 0;", "const bool ops = F.ops != 0 && !topo;",
     "test_bounds"),
]


def check(lib):
    """Every test function of tests/test_spread_engine_operators.py against one library: the names of those that failed."""
    import oracle
    import test_spread_engine_operators as t
    oracle.build()
    failed = []
    for name, fn in sorted(inspect.getmembers(t, inspect.isfunction)):
        if not name.startswith("test_"):
            continue
        kw = {k: (oracle if k == "oracle" else lib) for k in inspect.signature(fn).parameters}
        try:
            fn(**kw)
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
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--check", lib], capture_output=True, text=True)
    shutil.rmtree(tree)
    line = next((l for l in p.stdout.splitlines() if l.startswith("FAILED")), None)
    if p.returncode != 0 or line is None:
        return name, None, f"the run ended with status {p.returncode} before every test had run"
    return name, line.split()[1:], ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="(internal) run the tests against this library")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spread_operators", "mutations.txt"))
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
            lines.append(f"{name}: " + ("clean, every test passes" if not failed else "THE UNMUTATED SOURCE FAILS " + ", ".join(failed)))
            bad += bool(failed)
        else:
            ok = m[4] in failed
            bad += not ok
            lines.append(f"{name} ({m[1]})\n    named test {m[4]}: {'caught' if ok else 'NOT CAUGHT'}; every test that failed: {', '.join(failed) or '-'}")
    lines.append(f"{len(MUTATIONS)} mutations, {bad} problems")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
