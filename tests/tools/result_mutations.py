#!/usr/bin/env python3
"""Do the cases of tests/result_cases.py notice a wrong finalize, Go-sort, effective allocatable, claim record or scatter? (CPU only; a
tool, not a pytest test.)

Copies include/, karpenter_amd/, oracle/ and tests/ to a temporary directory once per mutation, applies ONE textual mutation to the
copy, builds the host emulation from it and runs tests/test_result_kernels.py there. One block per mutation: the tests that fail. A
mutation whose search text does not occur exactly once is an error of this tool (the source moved on: mend the list), never a pass; a
mutation nothing catches makes the exit status 1, unless the list marks it EQUIVALENT and says why. Nothing mutated is ever run on a GPU.

    python tests/tools/result_mutations.py [-j N] [--out profiles/result_tests/mutations.txt]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, file under karpenter_amd/csrc, search text, replacement[, why no input can tell the two apart])
MUTATIONS = [
    ("go_sort choose_pivot: l >= 50 -> l > 50", "go_sort.h", "if (l >= 50) { i = median(", "if (l > 50) { i = median("),
    ("go_sort sort: length <= 12 -> < 12", "go_sort.h", "if (length <= 12) { insertion_sort(a, b); break; }", "if (length < 12) { insertion_sort(a, b); break; }"),
    ("go_sort break_patterns: xorshift 13 -> 12", "go_sort.h", "r ^= r << 13;", "r ^= r << 12;"),
    ("go_sort choose_pivot: swaps == 12 -> 11", "go_sort.h", "(swaps == 12 ? 2 : 0)", "(swaps == 11 ? 2 : 0)"),
    ("go_sort partial_insertion_sort: j >= 1 -> j > a", "go_sort.h", "for (int j = i - 1; j >= 1; j--)", "for (int j = i - 1; j > a; j--)",
     "EQUIVALENT: a range with a > 0 lies right of a pivot that is <= all of it (pdqsort's invariant), so less(a, a - 1) is false and the loop stops at j == a either way"),
    ("go_sort sort: limit == 0 never true", "go_sort.h", "if (cur.limit == 0) { heap_sort(a, b); break; }", "if (false) { heap_sort(a, b); break; }"),
    ("finalize: cells shift * 4 -> * 3", "kernels.h", "cells |= (uint64_t)cts << (__builtin_ctz(zz) * 4);", "cells |= (uint64_t)cts << (__builtin_ctz(zz) * 3);"),
    ("finalize: capacity type tested in the reserved branch", "kernels.h",
     "if (((held >> a.resv_id[o]) & 1) && ((zones >> a.resv_zone[o]) & 1) && a.resv_price[o] < best) best = a.resv_price[o];",
     "if (((held >> a.resv_id[o]) & 1) && ((zones >> a.resv_zone[o]) & 1) && (cts & 1u) && a.resv_price[o] < best) best = a.resv_price[o];"),
    ("finalize: p < best -> <=", "kernels.h", "if (p < best) best = p;", "if (p <= best) best = p;",
     "EQUIVALENT: the minimum of a set of doubles is the same value whichever of two equal candidates is kept"),
    ("finalize: failed ? n : keep swapped", "kernels.h", "(uint32_t)(failed ? n : keep);", "(uint32_t)(failed ? keep : n);"),
    ("finalize: the union over n types for keep", "kernels.h", "for (int i = 0; i < keep; ++i) u |= a.it_reqs.mask", "for (int i = 0; i < n; ++i) u |= a.it_reqs.mask"),
    ("finalize: cur_empty = g_empty dropped in the else branch", "kernels.h", "cur[r] = v < cur[r] ? v : cur[r]; } cur_empty = g_empty; }", "cur[r] = v < cur[r] ? v : cur[r]; } }"),
    ("finalize: first appearance over the claim's types", "kernels.h",
     "uint64_t m = a.dg_its[(size_t)g * iw + w] & a.t_its[(size_t)t * iw + w]; if (m)", "uint64_t m = a.dg_its[(size_t)g * iw + w] & its[w]; if (m)"),
    ("finalize: dg_nonempty >> (pick - g0)", "kernels.h", "!((a.dg_nonempty >> pick) & 1);", "!((a.dg_nonempty >> (pick - g0)) & 1);"),
    ("finalize: c_reserved[c] for [src] (the sort)", "kernels.h", "const uint64_t held = (a.c_reserved ? a.c_reserved[src] : 0ull);", "const uint64_t held = (a.c_reserved ? a.c_reserved[c] : 0ull);"),
    ("finalize: c_reserved[c] for [src] (the cheapest price)", "kernels.h", "const uint64_t held = a.c_reserved[src];", "const uint64_t held = a.c_reserved[c];"),
    ("claim_gather: c_reserved[i] for [src]", "kernels.h", "a.out_reserved[i] = a.c_reserved[src];", "a.out_reserved[i] = a.c_reserved[i];"),
    ("eff_alloc: g1 - g0 > 1 -> >= 1", "kernels.h", "if (g1 - g0 > 1) {", "if (g1 - g0 >= 1) {"),
    ("eff_alloc: the last matching group", "kernels.h", "for (int x = g0; x < g1 && g < 0; ++x)", "for (int x = g0; x < g1; ++x)"),
    ("fast_record: it >= n_its dropped", "fast_engine.h", "if (it >= n_its || !((in >> l) & 1)) return false;\n      bool f = true;", "if (!((in >> l) & 1)) return false;\n      bool f = true;"),
    ("fast_record: <= -> < against eff", "fast_engine.h", "f = f && (int64_t)st.req[r] <= eff[(size_t)r * n_its + it];", "f = f && (int64_t)st.req[r] < eff[(size_t)r * n_its + it];"),
    ("fast_record: real[ts] dropped", "fast_engine.h", "const int t = a.fw.lim ? (int)a.fw.lim->real[ts] : ts;", "const int t = ts < P.n_templates ? ts : 0;"),
    ("fast_record: bounds kept on a concrete key", "fast_engine.h", "concrete |= kb; vcompl &= ~kb; vhg &= ~kb; vhl &= ~kb; }", "concrete |= kb; vcompl &= ~kb; }"),
    ("fast_record: the cold record written always", "fast_engine.h", "if (vhg | vhl) {   // the cold record is read only then", "if (true) {   // the cold record is read only then"),
    ("fast_scatter: the 0xFFFFFFFF test dropped", "fast_engine.h", "if (c == 0xFFFFFFFFu) return;\n  const uint32_t p = a.sorted[i];", "const uint32_t p = a.sorted[i];"),
]


def run_mutation(i, work):
    name, fname, old, new = MUTATIONS[i][:4]
    d = os.path.join(work, f"m{i + 1:02d}")
    for sub in ("include", "karpenter_amd", "oracle", "tests"):
        shutil.copytree(os.path.join(ROOT, sub), os.path.join(d, sub), ignore=shutil.ignore_patterns("_obj", "_ref", "libksolve*.so", "libksched.so", "__pycache__", "*.lock", "*.tmp"))
    shutil.copy(os.path.join(ROOT, "__graft_entry__.py"), d)
    path = os.path.join(d, "karpenter_amd", "csrc", fname)
    with open(path) as f:
        text = f.read()
    if text.count(old) != 1:
        raise SystemExit(f"mutation {i + 1} ({name}): its search text occurs {text.count(old)} times in {fname}")
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", os.path.join(d, "tests", "emu", "libksolve_emu.so"), os.path.join(d, "tests", "emu", "ksolve_emu.cpp")])
    r = subprocess.run([sys.executable, "-m", "pytest", "tests/test_result_kernels.py", "-q", "-p", "no:cacheprovider", "--tb=no", "-rf"], cwd=d, capture_output=True, text=True)
    return name, re.findall(r"^FAILED (\S+)", r.stdout, re.M), r.stdout[-400:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=4)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines, missed = [], 0
    with tempfile.TemporaryDirectory() as work, ThreadPoolExecutor(max_workers=args.j) as pool:
        for i, (name, failed, tail) in enumerate(pool.map(lambda i: run_mutation(i, work), range(len(MUTATIONS)))):
            why = MUTATIONS[i][4] if len(MUTATIONS[i]) > 4 else None
            if failed:
                lines.append(f"{i + 1:2d}. {name}: caught by {len(failed)} tests" + (" (listed as equivalent: mend the list)" if why else ""))
                lines += [f"      {t}" for t in failed[:12]] + ([f"      ... and {len(failed) - 12} more"] if len(failed) > 12 else [])
            elif why:
                lines += [f"{i + 1:2d}. {name}: not caught", f"      {why}"]
            else:
                lines += [f"{i + 1:2d}. {name}: NOT CAUGHT", "      " + tail.replace("\n", "\n      ")]
                missed += 1
    lines.append(f"{len(MUTATIONS) - missed} of {len(MUTATIONS)} mutations caught or shown equivalent")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
