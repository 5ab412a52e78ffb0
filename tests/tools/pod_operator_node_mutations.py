#!/usr/bin/env python3
"""Do the cases of tests/pod_operator_node_cases.py notice a wrong definedness test in the existing-node stage's pod operators
(csrc/node_stage.h, "Pod operators beside existing nodes": reason 37)? (CPU only; a tool, not a pytest test.)

As tests/tools/fast_cold_mutations.py: copies include/, karpenter_amd/, oracle/ and tests/ to a temporary directory once per mutation,
applies ONE textual mutation to the copy, builds the host emulation from it and runs tests/test_cursor_engine_pod_operators_nodes.py
there. One block per mutation: the tests that fail. A mutation whose search text does not occur exactly once is an error of this tool
(the source moved on: mend the list), never a pass; a mutation nothing catches makes the exit status 1. Nothing mutated is ever run on
a GPU.

    python tests/tools/pod_operator_node_mutations.py [-j N] [--out profiles/pod_operators_nodes/mutations.txt] [--check] [--only N ...]
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
TESTS = "tests/test_cursor_engine_pod_operators_nodes.py"

# (name, file under karpenter_amd/csrc, search text, replacement)
MUTATIONS = [
    ("the definedness test dropped", "node_stage.h", "if (k_notin & k_positive & k_undef) out.bail = DECLINE_NODE_KEY_DEFINEDNESS;", ""),
    ("DoesNotExist treated like NotIn", "node_stage.h", "if (notin ? op == OP_NOTIN : (op == OP_IN || op == OP_EXISTS)) m |= 1ull << k;", "if (notin ? op_negative(op) : (op == OP_IN || op == OP_EXISTS)) m |= 1ull << k;"),
    ("the nodes' reduction skipped (every key counts as undefined somewhere)", "node_stage.h",
     "const uint32_t k_undef = (uint32_t)W::reduce_or(nn, [&](int e) { return (uint64_t)(~ndef[e] & all_keys); });", "const uint32_t k_undef = all_keys; (void)ndef;"),
    ("the nodes' reduction reads the first node alone", "node_stage.h",
     "const uint32_t k_undef = (uint32_t)W::reduce_or(nn, [&](int e) { return (uint64_t)(~ndef[e] & all_keys); });", "const uint32_t k_undef = ~ndef[0] & all_keys;"),
    ("the positive classes' reduction skipped (every key counts as selected)", "node_stage.h", "const uint32_t k_positive = keys_with(false);", "const uint32_t k_positive = all_keys;"),
    ("the NotIn classes' reduction skipped (every key counts as excluded from)", "node_stage.h", "const uint32_t k_notin = keys_with(true);", "const uint32_t k_notin = all_keys;"),
    ("Exists not counted beside In", "node_stage.h", "if (notin ? op == OP_NOTIN : (op == OP_IN || op == OP_EXISTS)) m |= 1ull << k;", "if (notin ? op == OP_NOTIN : op == OP_IN) m |= 1ull << k;"),
    ("the host launches the plain stage kernels under 32 / 33", "ksolve_impl.h", "h->eng.node_pod_operators && h->fw.podops);", "false);"),
    ("the host launches the _p stage kernels under every setting", "ksolve_impl.h", "h->eng.node_pod_operators && h->fw.podops);", "h->fw.podops != nullptr);"),
]


def checked(i):
    name, fname, old, new = MUTATIONS[i]
    with open(os.path.join(ROOT, "karpenter_amd", "csrc", fname)) as f:
        n = f.read().count(old)
    if n != 1:
        raise SystemExit(f"mutation {i + 1} ({name}): its search text occurs {n} times in {fname}")


def run_mutation(i, work):
    name, fname, old, new = MUTATIONS[i]
    d = os.path.join(work, f"m{i + 1:02d}")
    for sub in ("include", "karpenter_amd", "oracle", "tests"):
        shutil.copytree(os.path.join(ROOT, sub), os.path.join(d, sub), ignore=shutil.ignore_patterns("_obj", "_ref", "*.so", "__pycache__", "*.lock", "*.tmp", "fullsize", "sweeps", "go_dump"))
    shutil.copy(os.path.join(ROOT, "__graft_entry__.py"), d)
    path = os.path.join(d, "karpenter_amd", "csrc", fname)
    with open(path) as f:
        text = f.read()
    with open(path, "w") as f:
        f.write(text.replace(old, new))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", os.path.join(d, "tests", "emu", "libksolve_emu.so"), os.path.join(d, "tests", "emu", "ksolve_emu.cpp")])
    r = subprocess.run([sys.executable, "-m", "pytest", TESTS, "-q", "-p", "no:cacheprovider", "--tb=no", "-rf"], cwd=d, capture_output=True, text=True)
    shutil.rmtree(d, ignore_errors=True)
    failed = re.findall(r"^FAILED (\S+.*)", r.stdout, re.M)
    if not failed and not re.search(r"\d+ passed", r.stdout):
        failed = [f"(the test process died with exit status {r.returncode} before its summary)"]
    return name, failed, r.stdout[-400:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=4)
    ap.add_argument("--out")
    ap.add_argument("--check", action="store_true", help="only check that every search text occurs exactly once")
    ap.add_argument("--only", type=int, nargs="*", help="run these mutations alone (numbers as the report prints them)")
    args = ap.parse_args()
    for i in range(len(MUTATIONS)):
        checked(i)
    if args.check:
        return 0
    lines, missed = [], 0
    with tempfile.TemporaryDirectory() as work, ThreadPoolExecutor(max_workers=args.j) as pool:
        picked = [n - 1 for n in args.only] if args.only else list(range(len(MUTATIONS)))
        for i, (name, failed, tail) in zip(picked, pool.map(lambda i: run_mutation(i, work), picked)):
            if failed:
                lines.append(f"{i + 1:2d}. {name}: caught by {len(failed)} tests")
                lines += [f"      {t}" for t in failed[:8]] + ([f"      ... and {len(failed) - 8} more"] if len(failed) > 8 else [])
            else:
                lines += [f"{i + 1:2d}. {name}: NOT CAUGHT", "      " + tail.replace("\n", "\n      ")]
                missed += 1
    lines.append(f"{len(picked) - missed} of {len(picked)} mutations caught")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
