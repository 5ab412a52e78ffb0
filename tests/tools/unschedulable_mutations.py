#!/usr/bin/env python3
"""Do the tests of tests/test_cursor_engine_unschedulable.py notice a wrong treatment of unschedulable pods on the cursor engine?
(CPU only; a tool, not a pytest test.)

Copies karpenter_amd/csrc, include/ and tests/emu to a temporary directory, applies ONE textual mutation at a time to the copy,
builds the host emulation from it and calls every test of tests/test_cursor_engine_unschedulable.py with that library (each case of
a parametrised test; the reversed-lanes cases, which need a second build, are left out). One line per mutation: the tests that
failed, and whether the test NAMED for the mutation is among them. A mutation whose search text does not occur exactly once is an
error of this tool (the source moved on: mend the list), never a pass; a mutation its named test does not catch makes the exit
status 1. A mutation named for no test is one that no CPU test can show; the log says why (UNOBSERVABLE).

    python tests/tools/unschedulable_mutations.py [-j N] [--out profiles/unschedulable/mutations.txt]
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

# (name, file under karpenter_amd/csrc, search text, replacement, the test that must catch it or None)
MUTATIONS = [
    ("no retry pass", "fast_engine.h",
     "if (!F.unsched || fast_uniform(h->status) != 0 || (F.nodes && F.nodes->limit_hit)) return 0;", "return 0;",
     "test_hand_problem[big-first]"),
    ("the stop rule ignored", "fast_engine.h",
     "if ((uint32_t)W::uniform((uint64_t)F.us_last[i]) == nu) break;", "",
     "test_hand_problem[absent-last-alone]"),
    ("the last template's error instead of the first", "fast_engine.h",
     "if (!fast_fields_ok(m, cs.dmask)) { if (!first_err) first_err = E_INCOMPATIBLE; continue; }", "if (!fast_fields_ok(m, cs.dmask)) { first_err = E_INCOMPATIBLE; continue; }",
     "test_hand_problem[tainted-first]"),
    ("the flags from the wrong template", "fast_engine.h",
     "first_diag = (int)W::uniform((uint64_t)(uint32_t)filter_diag(m, cs.size));", "first_diag = (int)W::uniform((uint64_t)(uint32_t)filter_diag(Mp->tvmask[0] & cs.cvmask, cs.size));",
     "test_hand_problem[inactive-first]"),
    ("the flags without the daemon overhead", "fast_engine.h",
     "const int64_t* eff = eff_alloc(P, tr);   // allocatable less the template's daemon overhead, as in create_entry", "const int64_t* eff = P.it_alloc;",
     "test_hand_problem[daemonset]"),
    ("a skipped template reports nothing", "fast_engine.h",
     "if (ts == -1) { if (!first_err) first_err = E_LIMITS; continue; }", "if (ts == -1) continue;",
     "test_hand_problem[cpu-chain]"),
    ("taints and requirements not told apart", "fast_engine.h",
     "first_err = (P.tmpl_taints[t] & ~P.cls_tolerates[k]) ? E_TAINTS : E_INCOMPATIBLE;", "first_err = E_INCOMPATIBLE;",
     "test_hand_problem[tainted-first]"),
    ("no sort on a failing attempt", "fast_engine.h",
     "if (fast_uniform(h->pend_new)) place_new_claim(n); else slow_sort(n, fast_uniform(h->pend_a), 0);", "",
     "test_hand_problem[sort-at-retry]"),
    ("no hostname number at a retry", "fast_engine.h",
     "      host_seq++;\n      n_ref_extra++;", "      if (!retry) host_seq++;\n      n_ref_extra++;",
     "test_hand_problem[two-big]"),   # (the templates a walk attempted are counted from the numbers it drew: the verdict kept per class carries them into the evaluation count)
    ("the templates left out of the retry's count", "fast_engine.h",
     "      host_seq++;\n      n_ref_extra++;", "      host_seq++;\n      if (!retry) n_ref_extra++;",
     "test_hand_problem[big-first]"),
    ("the nodes left out of the retry's count", "fast_engine.h",
     "n_ref_extra += (unsigned long long)(F.nodes ? P.n_nodes : 0);", "",
     "test_hand_problem[tail-run-nodes]"),
    ("the queue length of the compacted queue", "fast_engine.h",
     "const uint32_t pos = F.nodes ? F.pod_qpos[F.nd_pod[e]] : (uint32_t)e;", "const uint32_t pos = (uint32_t)e;",
     "test_hand_problem[tail-run-nodes]"),
    ("the error not re-evaluated at the retry", "fast_engine.h",
     "F.us_err[i] = (uint8_t)this->us_err_; F.us_diag[i] = (uint8_t)this->us_diag_; F.us_last[i] = nu;", "F.us_last[i] = nu;",
     "test_error_changes_at_the_retry"),
    ("a cached verdict outlives a change of the limits", "fast_engine.h",
     "if constexpr (US) if (lm) this->us_epoch++;", "",
     "test_error_changes_at_the_retry"),
    ("a cached verdict counts no template", "fast_engine.h",
     "host_seq += tried; n_ref_extra += (unsigned long long)tried;", "host_seq += tried;",
     "test_hand_problem[two-big]"),
    ("the cached verdicts not reset in setup()", "fast_engine.h",
     "W::for_n(nc, [&](int c) { uc[c] = 0; });", "",
     None),
    ("the set-aside list not reset in setup()", "fast_engine.h",
     "W::store(F.us_n, 0u); W::sync();", "W::sync();",
     "test_repeated_solves"),
    ("the step limit ignored at a retry", "fast_engine.h",
     "if (ms >= 0 && before + steps >= ms) { status = 2; break; }", "",
     "test_step_limit[plain]"),
    ("a handle of every setting keeps unschedulable pods", "ksolve_impl.h",
     "fw.unsched = h->eng.unschedulable && !h->eng.pair ? 1 : 0;", "fw.unsched = 1;",
     "test_hand_problem[big-first]"),
]


# why no CPU test can catch the mutations named for no test
UNOBSERVABLE = {
    "the cached verdicts not reset in setup()": "the emulation numbers the classes alike in every solve of a handle, so a stale verdict equals the fresh one; on the device class ids change from solve to solve",
}


def cases(t):
    """(id, callable taking the library and the oracle's results of the hand problems) of every test of the module but the
    reversed-lanes ones."""
    import oracle

    def bind(fn, **extra):
        params = inspect.signature(fn).parameters
        return lambda lib, wanted: fn(**extra, **{k: v for k, v in (("oracle", oracle), ("emu", lib), ("wanted", wanted)) if k in params})
    out = []
    for name, fn in sorted(inspect.getmembers(t, inspect.isfunction)):
        if not name.startswith("test_") or "reversed" in name:
            continue
        params = inspect.signature(fn).parameters
        if "name" in params:
            out += [(f"{name}[{n}]", bind(fn, name=n)) for n, _, _ in t.HAND]
        elif "nodes" in params:
            out += [(f"{name}[{label}]", bind(fn, nodes=v)) for label, v in (("plain", False), ("nodes", True))]
        else:
            out.append((name, bind(fn)))
    return out


def check(lib):
    import oracle
    import test_cursor_engine_unschedulable as t
    oracle.build()
    wanted = {name: oracle.solve(prob) for name, prob, _ in t.HAND}
    failed = []
    for cid, call in cases(t):
        try:
            call(lib, wanted)
        except Exception:   # (an assertion, or the library refusing / failing where the test expects a result)
            failed.append(cid)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unschedulable", "mutations.txt"))
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
        elif m[4] is None:
            lines.append(f"{name} ({m[1]})\n    named for no test ({UNOBSERVABLE[name]}); every test that failed: {', '.join(failed) or '-'}")
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
