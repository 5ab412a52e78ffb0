#!/usr/bin/env python3
"""Do the tests of tests/test_spread_engine_pod_operators.py notice a wrong treatment of negative pods and filter terms on the spread
engine? (CPU only; a tool, not a pytest test.)

Copies karpenter_amd/csrc, include/ and tests/emu to a temporary directory, applies ONE textual mutation at a time to the copy,
builds the host emulation from it and calls every test function of tests/test_spread_engine_pod_operators.py with that library. One
line per mutation: the tests that failed, and whether the test NAMED for the mutation is among them. A mutation whose search text
does not occur exactly once is an error of this tool (the source moved on: mend the list), never a pass; a mutation its named test
does not catch makes the exit status 1.

    python tests/tools/spread_pod_operators_mutations.py [-j N] [--out profiles/spread_pod_operators/mutations.txt]
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
    ("claim_cut reads every guard bit over an undefined key as undefined (rule 2 dropped)", "topo_engine.h",
     "if constexpr (PO) { if (pod_ops() && (m & Mp->fmask[j]) != Mp->fmask[j]) continue; }", "",
     "test_notin_pod_defines_the_key"),
    ("a NotIn term fails a bin that does not define the key, like an In term", "topo_nodes.h",
     "if ((undef >> gb) & 1) { if (!((s.fvm[i] >> gb) & 1)) ok = false; }", "if ((undef >> gb) & 1) ok = false;",
     "test_notin_term_on_an_undefined_key"),
    ("the phantom bit is admitted as a domain", "topo_engine.h",
     "const uint32_t D = (uint32_t)fast_uniform((int)hd.dom);", "const uint32_t D = (uint32_t)fast_uniform((int)hd.dom) | (pod_ops() ? 1u << (hd.width - 1) : 0u);",
     "test_unschedulable_pods"),
    # (dropping the guard test alone changes nothing for a pod-made complement set: its phantom bit keeps popc(f) != 1 as well)
    ("record_zonal counts a claim narrowed to one dictionary value and the phantom bit", "topo_engine.h",
     "if ((m2 >> (off + width)) & 1) continue;", "if ((m2 >> (off + width)) & 1) { if (!pod_ops()) continue; m2 &= ~(1ull << (off + width - 1)); }",
     "test_counted_but_not_concrete"),
    ("existing nodes with negative pods run on the spread engine", "fast_engine.h",
     "if (!need || P.n_nodes > 0) pod_ops = false;", "if (!need) pod_ops = false;",
     "test_still_declined"),
    ("a spread handle of every setting gets the pod operators", "ksolve_impl.h",
     "fw.podops = h->eng.spread_pod_operators && fw.unsched && fw.filt ? dz<ks::FastPodOps>(h, 1) : nullptr;", "fw.podops = fw.unsched && fw.filt ? dz<ks::FastPodOps>(h, 1) : nullptr;",
     "test_old_settings_stay_as_they_are"),
    ("a member with the switch shares the many-problem launch (of the kernels with the filters)", "solve_calls.h",
     "ks::pack_topo_many_row(ks::topo_flavour(h->fw),", "ks::pack_topo_many_row(h->fw.podops ? ks::TopoFlavour::Filter : ks::topo_flavour(h->fw),",
     "test_members_of_one_solve_many"),
    ("a class that selects nothing is ALWAYS inside a NotIn term", "topo_engine.h",
     "if (!(defined && !(cf & ~tf))) always = false;", "if (!(defined && (!(cf & ~tf) || !sel))) always = false;",
     "test_seeded_fuzz"),
    ("the DoesNotExist owner's term is packed as Exists", "topo_engine.h",
     "fvm |= ph | neg;", "fvm |= Mp->fmask[j];",
     "test_does_not_exist_term"),
]


def check(lib):
    """Every test function of tests/test_spread_engine_pod_operators.py against one library: the names of those that failed."""
    import oracle
    import test_spread_engine_pod_operators as t
    oracle.build()
    failed = []
    for name, fn in sorted(inspect.getmembers(t, inspect.isfunction)):
        if not name.startswith("test_"):
            continue
        kw = {k: (oracle if k == "oracle" else lib) for k in inspect.signature(fn).parameters}
        if "tmp_path" in kw:   # (the engine table: no library involved)
            continue
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spread_pod_operators", "mutations.txt"))
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
