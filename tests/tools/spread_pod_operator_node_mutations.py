#!/usr/bin/env python3
"""Do the cases of tests/spread_pod_operator_node_cases.py notice a wrong piece of the spread engine's pod operators beside existing
nodes (csrc/topo_nodes.h, "Pod operators beside existing nodes on the spread engine": the node filter under the phantom layout, the
definedness test of reason 37, the switch)? (CPU only; a tool, not a pytest test.)

As tests/tools/pod_operator_node_mutations.py: copies include/, karpenter_amd/, oracle/ and tests/ to a temporary directory once per
mutation, applies ONE textual mutation to the copy, builds the host emulation from it and runs
tests/test_spread_engine_pod_operators_nodes.py there (without its seeded fuzz). One block per mutation: the tests that fail. A mutation
whose search text does not occur exactly once is an error of this tool (the source moved on: mend the list), never a pass; a mutation
nothing catches makes the exit status 1. Nothing mutated is ever run on a GPU.

    python tests/tools/spread_pod_operator_node_mutations.py [-j N] [--out profiles/spread_pod_operators_nodes/mutations.txt] [--check] [--only N ...]
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
TESTS = "tests/test_spread_engine_pod_operators_nodes.py"

TERM_HALF = "  k_positive |= (uint32_t)W::reduce_or((int)Pv.topo.f_first[Pv.topo.n_groups], [&](int i) { return keys_of(Pv.topo.f_reqs.at(d, i), false); });"
PO_CUT = "  return topo_filter_cut_po(ctx.ft, Mp, ctx.nv, ctx.fs, m, undef, [&](const TopoFiltSlot& s) { return !(s.taint && (taints & ~tol[s.group])); });"
NODE_WORD = "// one dictionary value: the phantom bit stays clear\n    else { m |= Mp->fmask[j] | guard; undef |= guard; }"
KEEP_ON = "if constexpr (NP) { if (!need || (P.n_nodes > 0 && !F.node_podops)) pod_ops = false; } else"
NODE_PODOPS = ("      fw.node_podops = h->eng.spread_node_pod_operators && fw.podops && tw.nd.dom &&\n"
               "                       (reqs_negative(d->pod_reqs, d->n_pod_rows, P.dict, req_words, d->n_keys) || reqs_negative(d->topo.filter_reqs, d->topo.filter_first[d->topo.n], P.dict, req_words, d->n_keys)) ? 1 : 0;")   # (the whole statement)
# (name, file under karpenter_amd/csrc, search text, replacement)
MUTATIONS = [
    ("the filter-term half of the 37 test dropped", "topo_nodes.h", TERM_HALF, ""),
    ("the positive topo_filter_cut on nodes", "topo_nodes.h", PO_CUT, PO_CUT.replace("topo_filter_cut_po(", "topo_filter_cut(")),
    ("the node word without the undef guard", "topo_nodes.h", NODE_WORD, NODE_WORD.replace(" undef |= guard;", "")),
    ("pod_ops left on for settings without the switch", "fast_engine.h", KEEP_ON, "if constexpr (NP) { if (!need) pod_ops = false; } else"),
    ("the 37 test dropped", "topo_nodes.h", "  if (k_notin & k_positive & k_undef) return DECLINE_NODE_KEY_DEFINEDNESS;", ""),
    ("DoesNotExist treated like NotIn in the 37 test", "topo_nodes.h", "if (notin ? op == OP_NOTIN : (op == OP_IN || op == OP_EXISTS)) m |= 1ull << k;", "if (notin ? op_negative(op) : (op == OP_IN || op == OP_EXISTS)) m |= 1ull << k;"),
    ("the nodes' reduction of the 37 test reads the first node alone", "topo_nodes.h",
     "  const uint32_t k_undef = (uint32_t)W::reduce_or(nn, [&](int e) { return (uint64_t)(~ndef[e] & all_keys); });", "  const uint32_t k_undef = ~ndef[0] & all_keys;"),
    ("the host sets the switch for positive batches too", "ksolve_impl.h", NODE_PODOPS, "      fw.node_podops = h->eng.spread_node_pod_operators && fw.podops && tw.nd.dom ? 1 : 0;"),
    ("the host never picks ksolve_pack_topo_nodes_pn", "ksolve_impl.h", "h->n_nodes > 0 && h->fw.node_podops; }", "h->n_nodes > 0 && h->fw.node_podops && false; }"),
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
    r = subprocess.run([sys.executable, "-m", "pytest", TESTS, "-q", "-p", "no:cacheprovider", "--tb=no", "-rf", "-k", "not seeded_fuzz"], cwd=d, capture_output=True, text=True)
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
