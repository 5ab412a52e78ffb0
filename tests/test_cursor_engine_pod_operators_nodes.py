"""CPU tests of the pod operators of the cursor engine's existing-node stage (csrc/node_stage.h, "Pod operators beside existing
nodes"; engines "auto-pod-operators-nodes" / "cursor-pod-operators-nodes", 32 / 33): through the host emulation of the device code
(tests/emu, test infrastructure only), the real C ABI and the real flattener, against the oracle in claims and their order, node by
node, pod errors, the reference-equivalent evaluation count and the packing cost. The problems and the checks are
tests/pod_operator_node_cases.py's; the device run is tests/test_gpu_cursor_pod_operators_nodes.py."""
import os
import subprocess

import pytest

import engine_checks as ec
import pod_operator_node_cases as nc
from karpenter_amd import fixtures as fx
from test_device_algorithm import emu  # noqa: F401  (fixture)


@pytest.mark.parametrize("n_nodes,block0_zone1", [(n, False) for n in nc.BLOCK_EDGES] + [(65, True), (129, True)])
def test_block_edges(oracle, emu, n_nodes, block0_zone1):
    """The cursor of a negative class through every block, over a block whose row is all dead, and past the last node."""
    nc.check_block_edge(oracle, emu, n_nodes, block0_zone1)


def test_one_custom_key_three_operators(oracle, emu):
    """DoesNotExist (and In []) pods on unlabelled nodes only, In [x] pods on labelled ones only, plain pods on both: no 37."""
    nc.check_dedicated(oracle, emu)


def test_notin_on_a_key_no_node_carries_and_no_positive_class_uses(oracle, emu):
    nc.check_unused_key(oracle, emu)


def test_exists_on_a_key_some_nodes_carry(oracle, emu):
    nc.check_exists(oracle, emu)


def test_reason_37_and_its_twin(oracle, emu):
    """A NotIn pod defines the key on a node that lacked it and In pods follow it there: declined by name; with the key on every node
    the same batch stays on the cursor engine."""
    nc.check_key_definedness(oracle, emu)


def test_with_a_binding_limit(oracle, emu):
    nc.check_limit(oracle, emu)


def test_with_a_complement_nodepool(oracle, emu):
    nc.check_complement_pool(oracle, emu)


def test_with_daemonsets(oracle, emu):
    nc.check_daemonsets(oracle, emu)


def test_a_pod_that_excludes_every_zone(oracle, emu):
    nc.check_no_zone(oracle, emu)


def test_the_loops_declines_are_still_named(oracle, emu):
    nc.check_loop_declines(oracle, emu)


def test_lds_and_hbm_variants(oracle, emu):
    nc.check_variants(oracle, emu, emu)


def test_repeated_solves_give_one_digest(oracle, emu):
    nc.check_repeated(oracle, emu, 20)


def test_solve_many(oracle, emu):
    nc.check_solve_many(oracle, emu)


def test_settings_below_keep_their_reasons_and_topology_stays_out(oracle, emu):
    """26 / 27 / 29 answer a batch with nodes and negative pods with 4 as before (pod_operator_cases.nodes_problem pins 26 / 27 too);
    a topology batch with nodes and a negative pod keeps 4 under 32."""
    import spread_node_cases as sn
    prob = nc.block_edge_problem(63)
    for setting in ("auto-pod-operators", "auto-pod-operators-spread", "auto-filters-spread"):
        assert ec.where(ec.solve(prob, setting, emu)) == ("general", 4), setting
    ec.refusal_says(ec.refusal(prob, "cursor-pod-operators", emu), "cursor", 4)
    topo = sn.mix_problem((300, 144, 1), 5)
    topo["pods"] = list(topo["pods"]) + [fx.pod(requests={"cpu": "100m"}, node_requirements=nc.notin(fx.ZONE, "test-zone-1"))]
    got = ec.solve(topo, nc.AUTO, emu)
    assert ec.where(got) == ("general", 4), got["counters"]
    ec.same(got, oracle.solve(topo), topo)


def test_positive_batches_count_the_same_work(emu):
    """A problem without such pods, with and without nodes, does the same work under the new names as under the names below them."""
    for prob, below in ((fx.config1(), "auto"), (fx.with_existing_nodes(fx.config2(pods=1500, n_types=60, seed=4), 70, seed=3), "auto-nodes")):
        a = ec.solve(prob, below, emu)["counters"]
        for engine in (nc.AUTO, nc.ENGINE):
            c = ec.solve(prob, engine, emu)["counters"]
            assert c["engine"] == "cursor" and c["engineFallbackReason"] == 0
            assert (c["binEvaluations"], c["slowSorts"], c["referenceBinEvaluations"], c["pops"], c["phaseCycles"][19]) == \
                   (a["binEvaluations"], a["slowSorts"], a["referenceBinEvaluations"], a["pops"], a["phaseCycles"][19])


# every row of csrc/engine_setting.h's table with the new switch's column, 34 (past the table) included, and four engine_value lookups
# (value, run, first plan, pick, pair, nodes, s-nodes, limits, s-limits, ops, s-ops, unsched, s-unsched, s-filters, pod-ops, s-pod-ops,
#  node-pod-ops, name)
ENGINE_TABLE = """\
0 0 0 1 0 0 0 0 0 0 0 0 0 0 0 0 0 auto
1 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 general
2 2 0 1 0 0 0 0 0 0 0 0 0 0 0 0 0 cursor
3 2 1 0 0 0 0 0 0 0 0 0 0 0 0 0 0 cursor-wide
4 2 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 cursor-hbm
5 2 0 0 1 0 0 0 0 0 0 0 0 0 0 0 0 cursor-pair
6 3 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 spread
7 0 0 1 0 1 0 0 0 0 0 0 0 0 0 0 0 auto-nodes
8 2 0 1 0 1 0 0 0 0 0 0 0 0 0 0 0 cursor-nodes
9 0 0 1 0 1 1 0 0 0 0 0 0 0 0 0 0 auto-nodes-spread
10 3 0 0 0 0 1 0 0 0 0 0 0 0 0 0 0 spread-nodes
11 0 0 1 0 1 0 1 0 0 0 0 0 0 0 0 0 auto-limits
12 2 0 1 0 1 0 1 0 0 0 0 0 0 0 0 0 cursor-limits
13 0 0 1 0 1 1 1 1 0 0 0 0 0 0 0 0 auto-limits-spread
14 3 0 0 0 0 1 0 1 0 0 0 0 0 0 0 0 spread-limits
15 0 0 1 0 1 1 1 1 1 0 0 0 0 0 0 0 auto-operators
16 2 0 1 0 1 0 1 0 1 0 0 0 0 0 0 0 cursor-operators
17 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 -
18 0 0 1 0 1 1 1 1 1 1 0 0 0 0 0 0 auto-operators-spread
19 3 0 0 0 0 1 0 1 0 1 0 0 0 0 0 0 spread-operators
20 0 0 1 0 1 1 1 1 1 1 1 0 0 0 0 0 auto-unschedulable
21 2 0 1 0 1 0 1 0 1 0 1 0 0 0 0 0 cursor-unschedulable
22 0 0 1 0 1 1 1 1 1 1 1 1 0 0 0 0 auto-unschedulable-spread
23 3 0 0 0 0 1 0 1 0 1 0 1 0 0 0 0 spread-unschedulable
24 0 0 1 0 1 1 1 1 1 1 1 1 1 0 0 0 auto-filters-spread
25 3 0 0 0 0 1 0 1 0 1 0 1 1 0 0 0 spread-filters
26 0 0 1 0 1 1 1 1 1 1 1 1 1 1 0 0 auto-pod-operators
27 2 0 1 0 1 0 1 0 1 0 1 0 0 1 0 0 cursor-pod-operators
28 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 -
29 0 0 1 0 1 1 1 1 1 1 1 1 1 1 1 0 auto-pod-operators-spread
30 3 0 0 0 0 1 0 1 0 1 0 1 1 0 1 0 spread-pod-operators
31 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 -
32 0 0 1 0 1 1 1 1 1 1 1 1 1 1 1 1 auto-pod-operators-nodes
33 2 0 1 0 1 0 1 0 1 0 1 0 0 1 0 1 cursor-pod-operators-nodes
34 2 0 0 0 0 0 0 0 0 0 0 0 0 0 0 0 -
32 33 29 0
"""   # (17, 28, 31: no row of their own, 34: past the table; the last line: the two new names, auto-pod-operators-spread, no-such-name)


def test_rows_of_the_engine_table(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "rows.cpp"
    src.write_text('#include <cstdio>\n#include "engine_setting.h"\nstatic void row(int v, const ksi::EnginePolicy& p) {\n'
                   '  printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %s\\n", v, (int)p.run, p.first_plan, p.pick_plan, p.pair, p.nodes, p.spread_nodes, p.limits, p.spread_limits,\n'
                   '         p.operators, p.spread_operators, p.unschedulable, p.spread_unschedulable, p.spread_filters, p.pod_operators, p.spread_pod_operators, p.node_pod_operators,\n'
                   '         p.name ? p.name : "-");\n}\n'
                   'static_assert(ksi::kEngineSettingCount == 34, "rows 0-33");\n'
                   'int main() { for (unsigned v = 0; v <= 34; ++v) row((int)v, ksi::engine_policy(v));\n'
                   '  printf("%u %u %u %u\\n", ksi::engine_value("auto-pod-operators-nodes"), ksi::engine_value("cursor-pod-operators-nodes"), ksi::engine_value("auto-pod-operators-spread"),\n'
                   '         ksi::engine_value("no-such-name")); }\n')
    exe = tmp_path / "rows"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(root, "karpenter_amd", "csrc"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).splitlines() == ENGINE_TABLE.splitlines()


def test_seeded_fuzz(oracle, emu):
    """Forty seeds of pc.fuzz_problem with 5, 64 or 130 existing nodes: each equals the oracle under "auto-pod-operators-nodes"; at
    least 30 end on the cursor engine with reason 0, the others name a by-design decline (9-12) or 37; and in at least half of the
    seeds the ORACLE places a pod of a negative class on a node (the generator and the nodes do what they are for)."""
    on_cursor, rest, negative_on_nodes = nc.run_fuzz(oracle, emu, nc.FUZZ_SEEDS)
    assert on_cursor >= 30, (on_cursor, rest)
    assert negative_on_nodes * 2 >= len(nc.FUZZ_SEEDS), negative_on_nodes
