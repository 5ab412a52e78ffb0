"""CPU tests of the pod operators of the spread engine's existing-node path (csrc/topo_nodes.h, "Pod operators beside existing nodes on
the spread engine"; engines "auto-pod-operators-spread-nodes" / "spread-pod-operators-nodes", 35 / 36): through the host emulation of
the device code (tests/emu, test infrastructure only), the real C ABI and the real flattener, against the oracle in claims and their
order, node by node, pod errors, the reference-equivalent evaluation count and the packing cost. The problems and the checks are
tests/spread_pod_operator_node_cases.py's; the device run is tests/test_gpu_spread_pod_operators_nodes.py."""
import os
import subprocess

import pytest

import spread_pod_operator_node_cases as sc
from test_device_algorithm import emu  # noqa: F401  (fixture)


def test_a_lone_notin_pod_beside_a_zonal_spread(oracle, emu):
    """Nodes take pods first, the zone-3 nodes never take the pod that excludes the zone, the spread is 3 / 3 / 3 with the nodes' pods counted."""
    sc.check_lone_notin(oracle, emu)


def test_owners_that_carry_the_notin_node_then_claim_then_node(oracle, emu):
    sc.check_own_notin(oracle, emu)


@pytest.mark.parametrize("n_nodes", sc.BLOCK_EDGES)
def test_block_edges(oracle, emu, n_nodes):
    """The only node a negative class may take is the last of its alive word, or alone in the last word."""
    sc.check_block_edge(oracle, emu, n_nodes)


def test_does_not_exist_beside_in_on_one_key(oracle, emu):
    """DoesNotExist (and In []) pods on unlabelled nodes only, In [x] pods on labelled ones only: no decline."""
    sc.check_dedicated(oracle, emu)


@pytest.mark.parametrize("case", sc.filter_cases(), ids=lambda c: c[0])
def test_node_filter_on_a_node(oracle, emu, case):
    sc.check_filter_case(oracle, emu, case)


def test_reason_37_both_forms_and_their_twins(oracle, emu):
    """A key some node lacks with a NotIn class and an In class on it — the In once a plain pod's, once the term spread owners carry
    (their class's requirement too: the term half alone is test_definedness_check_directly's) —: declined by name before any pod is
    placed; with the key on every node the same batch stays on the spread engine."""
    sc.check_key_definedness(oracle, emu)


def test_pods_that_exclude_every_zone(oracle, emu):
    sc.check_no_zone(oracle, emu)


def test_with_a_binding_limit(oracle, emu):
    sc.check_limit(oracle, emu)


def test_with_daemonsets(oracle, emu):
    sc.check_daemonsets(oracle, emu)


def test_with_a_complement_nodepool(oracle, emu):
    sc.check_complement_pool(oracle, emu)


def test_settings_below_keep_engine_reason_and_digest(oracle, emu):
    sc.check_settings_below(oracle, emu)


def test_positive_batches_and_kernel_names(oracle, emu):
    sc.check_positive_batches(oracle, emu)


def test_repeated_solves_give_one_digest(oracle, emu):
    sc.check_repeated(oracle, emu, 20)


def test_solve_many(oracle, emu):
    sc.check_solve_many(oracle, emu)


# rows 32-37 of csrc/engine_setting.h's table with the new switch's column, and the lookups of the new names
# (value, run, nodes, s-nodes, pod-ops, s-pod-ops, node-pod-ops, s-node-pod-ops, name)
ENGINE_ROWS = """\
30 3 0 1 0 1 0 0 spread-pod-operators
32 0 1 1 1 1 1 0 auto-pod-operators-nodes
33 2 1 0 1 0 1 0 cursor-pod-operators-nodes
34 2 0 0 0 0 0 0 -
35 0 1 1 1 1 1 1 auto-pod-operators-spread-nodes
36 3 0 1 0 1 0 1 spread-pod-operators-nodes
37 2 0 0 0 0 0 0 -
35 36 32 0 34 37
"""   # (34: a hole like 17, 28 and 31; 37: past the table; the last line: the two new names, auto-pod-operators-nodes, no-such-name, the two counts)


def test_rows_of_the_engine_table(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "rows.cpp"
    src.write_text('#include <cstdio>\n#include "engine_setting.h"\nstatic void row(int v, const ksi::EnginePolicy& p) {\n'
                   '  printf("%d %d %d %d %d %d %d %d %s\\n", v, (int)p.run, p.nodes, p.spread_nodes, p.pod_operators, p.spread_pod_operators, p.node_pod_operators,\n'
                   '         p.spread_node_pod_operators, p.name ? p.name : "-");\n}\n'
                   'static_assert(ksi::kEngineSettingCount == 34, "rows 0-33");\n'
                   'int main() { const unsigned vs[] = {30, 32, 33, 34, 35, 36, 37}; for (unsigned v : vs) row((int)v, ksi::engine_policy(v));\n'
                   '  printf("%u %u %u %u %u %u\\n", ksi::engine_value("auto-pod-operators-spread-nodes"), ksi::engine_value("spread-pod-operators-nodes"),\n'
                   '         ksi::engine_value("auto-pod-operators-nodes"), ksi::engine_value("no-such-name"), ksi::kEngineSettingCount, ksi::kEngineTableRows); }\n')
    exe = tmp_path / "rows"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(root, "karpenter_amd", "csrc"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).splitlines() == ENGINE_ROWS.splitlines()


# ks::topo_nodes_definedness alone, on the host's loop-over-lanes wavefront: three keys (0: the group's key, 1 and 2: custom keys of one
# dictionary word each), per case the operator a class / a node-filter term uses on key 1 ("-": none; i In, n NotIn, e Exists, d
# DoesNotExist), which of two nodes carry key 1, and the domain index of node 1 on key 0 -> the reason. Through a problem the term
# form cannot be had alone (an owner's term is its class's requirement too), so the function is asked directly.
DEFINEDNESS = r"""
#include <cstddef>
#include <cstdio>
#include <cstring>
#include "engine.h"
#include "topo_nodes.h"
using namespace ks;
static int run(const char* cls_ops, const char* term_ops, unsigned node_has_key1, int dom1) {
  ProblemView P{}; Workspace S{}; TopoWork T{};
  Dict& d = P.dict; d.n_keys = 3; d.req_words = 3; for (int k = 0; k <= 3; ++k) d.key_word_off[k] = k;
  auto table = [&](const char* ops, uint64_t* mask, uint32_t* def, uint32_t* comp) {
    const int n = (int)strlen(ops);
    for (int i = 0; i < n; ++i) {
      def[i] = comp[i] = 0; mask[3 * i] = mask[3 * i + 1] = mask[3 * i + 2] = 0;
      if (ops[i] == '-') continue;
      def[i] = 2u;
      if (ops[i] == 'i' || ops[i] == 'n') mask[3 * i + 1] = 1;
      if (ops[i] == 'n' || ops[i] == 'e') comp[i] = 2u;
    }
    ReqTable t{}; t.mask = mask; t.defined = def; t.complement = comp;
    return t;
  };
  uint64_t cm[24], fm[24]; uint32_t cd[8], cc[8], fd[8], fc[8];
  P.cls_reqs = table(cls_ops, cm, cd, cc); P.n_classes = (int)strlen(cls_ops);
  P.topo.f_reqs = table(term_ops, fm, fd, fc);
  const uint32_t first[2] = {0, (uint32_t)strlen(term_ops)}; const int32_t key[1] = {0};
  P.topo.n_groups = 1; P.topo.f_first = first; P.topo.key = key;
  P.n_nodes = 2;
  uint32_t ndef[2] = {1u | ((node_has_key1 & 1u) ? 2u : 0u), 1u | ((node_has_key1 & 2u) ? 2u : 0u)};
  S.n_defined0 = ndef;
  uint8_t dom[6] = {0, (uint8_t)dom1, 0xFF, 0xFF, 0xFF, 0xFF};
  T.nd.dom = dom;
  return topo_nodes_definedness<Wave>(&P, &S, &T);
}
int main() {
  const struct { const char *cls, *term; unsigned has; int dom1; } cases[] = {
    {"ni", "", 1, 1}, {"ne", "", 2, 1}, {"n-", "i", 1, 1}, {"n", "e", 0, 1}, {"n", "-i", 2, 1},   // the class form, the term form: 37
    {"ni", "i", 3, 1}, {"n", "n", 0, 1}, {"di", "e", 0, 1}, {"i", "i", 0, 1}, {"n", "d", 1, 1},   // every node keyed; no positive user; DoesNotExist; no NotIn: 0
    {"n", "", 3, 14}, {"n", "", 3, 15}, {"ni", "", 0, 15}};                                         // the phantom bit's index: 36 (behind 37)
  for (const auto& c : cases) printf("%s|%s|%u|%d -> %d\n", c.cls, c.term, c.has, c.dom1, run(c.cls, c.term, c.has, c.dom1));
}
"""
DEFINEDNESS_WANT = """\
ni||1|1 -> 37
ne||2|1 -> 37
n-|i|1|1 -> 37
n|e|0|1 -> 37
n|-i|2|1 -> 37
ni|i|3|1 -> 0
n|n|0|1 -> 0
di|e|0|1 -> 0
i|i|0|1 -> 0
n|d|1|1 -> 0
n||3|14 -> 0
n||3|15 -> 36
ni||0|15 -> 37
"""


def test_definedness_check_directly(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src, exe = tmp_path / "definedness.cpp", tmp_path / "definedness"
    src.write_text(DEFINEDNESS)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "karpenter_amd", "csrc"), "-I", os.path.join(root, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).splitlines() == DEFINEDNESS_WANT.splitlines()


def test_seeded_fuzz(oracle, emu):
    """spread_pod_operator_cases' generator with 5, 64 or 130 nodes: every seed equals the oracle under "auto-pod-operators-spread-nodes";
    at least four fifths end on the spread engine with reason 0, the rest name 9-12, 35-37, 43 or 50; in at least half of the seeds the
    ORACLE places a pod of a negative class on a node, and at least one seed leaves a pod error (the generator does what it is for)."""
    n = len(sc.FUZZ_SEEDS)
    on_spread, rest, negative_on_nodes, errors = sc.run_fuzz(oracle, emu, sc.FUZZ_SEEDS)
    assert on_spread * 5 >= n * 4, (on_spread, rest)
    assert negative_on_nodes * 2 >= n, negative_on_nodes
    assert errors >= 1
