"""GPU tests (run with -m gpu on an MI355X) of the pod operators of the spread engine's existing-node path (csrc/topo_nodes.h, "Pod
operators beside existing nodes on the spread engine"; kernel ksolve_pack_topo_nodes_pn of csrc/ksolve_pack_topo_nodes_pn.hip; engines
"auto-pod-operators-spread-nodes" / "spread-pod-operators-nodes"): the product library through the C ABI against the oracle, on the
problems and with the checks of tests/spread_pod_operator_node_cases.py — the ones tests/test_spread_engine_pod_operators_nodes.py
runs on the emulation, at the same small shapes. The kernels' names are asked of the gfx950 build with -DKSOLVE_TEST_HOOKS
(tests/emu/libksolve_hooks.so), as tests/test_gpu_kernel_table.py does."""
import pytest

import parity
import spread_pod_operator_node_cases as sc
from gpu_support import built  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def test_a_lone_notin_pod_beside_a_zonal_spread(oracle):
    sc.check_lone_notin(oracle, None)


def test_owners_that_carry_the_notin_node_then_claim_then_node(oracle):
    sc.check_own_notin(oracle, None)


@pytest.mark.parametrize("n_nodes", sc.BLOCK_EDGES)
def test_block_edges(oracle, n_nodes):
    sc.check_block_edge(oracle, None, n_nodes)


def test_does_not_exist_beside_in_on_one_key(oracle):
    sc.check_dedicated(oracle, None)


@pytest.mark.parametrize("case", sc.filter_cases(), ids=lambda c: c[0])
def test_node_filter_on_a_node(oracle, case):
    sc.check_filter_case(oracle, None, case)


def test_reason_37_both_forms_and_their_twins(oracle):
    sc.check_key_definedness(oracle, None)


def test_pods_that_exclude_every_zone(oracle):
    sc.check_no_zone(oracle, None)


def test_with_a_binding_limit(oracle):
    sc.check_limit(oracle, None)


def test_with_daemonsets(oracle):
    sc.check_daemonsets(oracle, None)


def test_with_a_complement_nodepool(oracle):
    sc.check_complement_pool(oracle, None)


def test_settings_below_keep_engine_reason_and_digest(oracle):
    sc.check_settings_below(oracle, None)


def test_positive_batches_and_kernel_names(oracle):
    sc.check_positive_batches(oracle, parity.build_hooks())


def test_repeated_solves_give_one_digest(oracle):
    """Class ids are drawn from an atomic counter and differ from solve to solve; the static rows are computed with every solve's classes."""
    sc.check_repeated(oracle, None, 50)


def test_solve_many(oracle):
    sc.check_solve_many(oracle, None)


def test_seeded_fuzz(oracle):
    """Every fourth seed of test_spread_engine_pod_operators_nodes.test_seeded_fuzz, under its conditions."""
    n = len(sc.GPU_FUZZ_SEEDS)
    on_spread, rest, negative_on_nodes, errors = sc.run_fuzz(oracle, None, sc.GPU_FUZZ_SEEDS)
    assert on_spread * 5 >= n * 4, (on_spread, rest)
    assert negative_on_nodes * 2 >= n, negative_on_nodes
    assert errors >= 1
