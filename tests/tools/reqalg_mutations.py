#!/usr/bin/env python3
"""Do the cases of tests/reqalg_cases.py notice a wrong requirement algebra? (CPU only; a tool, not a pytest test.)

Copies karpenter_amd/csrc, include/ and tests/emu to a temporary directory, applies ONE textual mutation at a time to the copy,
builds the host emulation from it and runs the cases of tests/test_reqalg.py against that library. One line per mutation: caught
or not by the reference's tables, by the generated pairs, by the index cases. A mutation whose search text does not occur exactly
once is an error of this tool (the source moved on: mend the list), never a pass; a mutation nothing catches makes the exit
status 1. The atomic OR of it_index_body exists in the device build only (the emulation's loop is serial): it is listed as
"device only" with the case that holds it on the GPU.

    python tests/tools/reqalg_mutations.py [-j N] [--out profiles/reqalg_tests/mutations.txt]
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, file under karpenter_amd/csrc, search text, replacement, device_only)
MUTATIONS = [
    ("inbounds_word: value_is_int filter dropped", "reqalg.h",
     "uint64_t c = candidates & d.value_is_int[w];", "uint64_t c = candidates;", False),
    ("reqbuf_add: collapse at gte >= lte", "reqalg.h",
     "if (bd.hg && bd.hl && bd.g > bd.l) {", "if (bd.hg && bd.hl && bd.g >= bd.l) {", False),
    ("has_intersection: collapse at gte >= lte", "reqalg.h",
     "if (bd.hg && bd.hl && bd.g > bd.l) return false;", "if (bd.hg && bd.hl && bd.g >= bd.l) return false;", False),
    ("reqbuf_add: qm & ~am swapped to am & ~qm", "reqalg.h",
     "(ac && !qc) ? (qm & ~am)", "(ac && !qc) ? (am & ~qm)", False),
    ("reqs_intersect: NotIn / DoesNotExist escape removed", "reqalg.h",
     "if (op_negative(req_op(d, q, k)) && op_negative(req_op(d, r, k))) continue;", "", False),
    ("reqbuf_add: bounds kept on concrete results", "reqalg.h",
     "if (!comp) bd.hg = bd.hl = false;", "", False),
    ("reqbuf_add: minValues min instead of max", "reqalg.h",
     "int32_t mv = acc.minv[k] > qmv ? acc.minv[k] : qmv;", "int32_t mv = acc.minv[k] < qmv ? acc.minv[k] : qmv;", False),
    ("key_nonempty: only the key's first word", "reqalg.h",
     "for (uint32_t w = d.key_word_off[k]; w < d.key_word_off[k + 1]; ++w) if (mask[w]) return true;",
     "for (uint32_t w = d.key_word_off[k]; w < d.key_word_off[k] + 1; ++w) if (mask[w]) return true;", False),
    ("req_values_word: without value_valid", "reqalg.h",
     "const uint64_t base = bit(r.complement, k) ? (~r.mask[w] & d.value_valid[w]) : r.mask[w];",
     "const uint64_t base = bit(r.complement, k) ? (~r.mask[w]) : r.mask[w];", False),
    ("combine_bounds: lte max instead of min", "reqalg.h",
     "(alv < blv ? alv : blv)", "(alv > blv ? alv : blv)", False),
    ("reqs_compatible: well_known_mask ignored", "reqalg.h",
     "if (allow_undefined) undef &= ~d.well_known_mask;", "", False),
    ("req_has: bounds ignored on complement sets", "reqalg.h",
     "if (hg || hl) {", "if ((hg || hl) && !bit(r.complement, k)) {", False),
    ("it_index_body: key_neg never written", "kernels.h",
     "if (op_negative(req_op(d, r, k))) atomic_or_u64(&a.key_neg[(size_t)k * iw + word], bitv);", "", False),
    ("it_index_body: value_valid dropped from the complement has", "kernels.h",
     "uint64_t has = comp ? (~r.mask[w] & d.value_valid[w]) : r.mask[w];", "uint64_t has = comp ? ~r.mask[w] : r.mask[w];", False),
    ("it_index_body: plain |= instead of the atomic OR", "kernels.h",
     "{ atomicOr((unsigned long long*)p, (unsigned long long)v); }", "{ *p |= v; }", True),
]


def check(lib):
    """The cases of tests/test_reqalg.py against one library: 'tables=0/1 pairs=0/1 index=0/1' (1 = a case failed)."""
    import reqalg_cases as rc

    def fails(fn):
        try:
            fn()
            return 0
        except AssertionError:
            return 1

    def pairs():
        for name in rc.SHAPES:
            rc.run_shape(lib, name)

    def index():
        for n_its, n_res in rc.INDEX_SIZES:
            rc.run_index(lib, n_its, n_res, "ordinary")
        for n_its in rc.CONTENTION_SIZES:
            rc.run_index(lib, n_its, 2, "contention")
        for kind in ("wrong-name", "bound"):
            rc.run_index(lib, 65, 2, kind)

    print(f"tables={fails(lambda: rc.run_tables(lib, rc.golden_tables()))} pairs={fails(pairs)} index={fails(index)}")


def build_and_check(work, i, mutation):
    name, fname, old, new, device_only = mutation
    tree = os.path.join(work, f"m{i}")
    for d in ("karpenter_amd/csrc", "include", "tests/emu"):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(tree, d), ignore=shutil.ignore_patterns("_obj", "*.so", "*.lock", "*.tmp"))
    if mutation is not None and old is not None:
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
    if p.returncode != 0:
        return name, dict(tables=1, pairs=1, index=1), f"the run ended with status {p.returncode}"
    return name, {k: int(v) for k, v in (kv.split("=") for kv in p.stdout.split())}, ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", help="(internal) run the cases against this library")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reqalg_tests", "mutations.txt"))
    args = ap.parse_args()
    if args.check:
        check(args.check)
        return 0
    every = [("(no mutation)", None, None, None, False)] + MUTATIONS
    with tempfile.TemporaryDirectory() as work, ThreadPoolExecutor(max_workers=args.j) as pool:
        results = list(pool.map(lambda im: build_and_check(work, *im), enumerate(every)))
    lines = [f"{'mutation':<62} {'tables':<8} {'pairs':<8} {'index':<8} verdict"]
    bad = 0
    for (name, got, note), m in zip(results, every):
        if got is None:
            lines.append(f"{name:<62} {note}")
            bad += 1
            continue
        word = lambda k: "caught" if got[k] else "-"
        caught = any(got.values())
        if m[1] is None:
            verdict = "clean" if not caught else "THE UNMUTATED SOURCE FAILS"
            bad += caught
        elif m[4]:
            verdict = ("device only: the emulation's loop is serial, its atomic_or_u64 is `*p |= v` already. On the GPU the contention case "
                       "(tests/test_gpu_reqalg.py::test_it_index_contention) holds it: the 64 threads of a word would read the same old word and "
                       "the last store would leave one bit of 64") if not caught else "caught (unexpected for a device-only mutation)"
        else:
            verdict = "caught" if caught else "NOT CAUGHT"
            bad += not caught
        lines.append(f"{name:<62} {word('tables'):<8} {word('pairs'):<8} {word('index'):<8} {verdict}" + (f" ({note})" if note else ""))
    lines.append(f"{sum(1 for m in MUTATIONS if not m[4])} host mutations, {bad} problems")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
