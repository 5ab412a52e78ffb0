"""GPU tests (run with -m gpu on an MI355X) of the pod operators of the cursor engine's existing-node stage (csrc/node_stage.h, "Pod
operators beside existing nodes"; kernels ksolve_pack_nodes_lds_p / ksolve_pack_nodes_hbm_p of csrc/ksolve_pack_nodes.hip in front of
the PodOps flavour of the loop; engines "auto-pod-operators-nodes" / "cursor-pod-operators-nodes"): the product library through the C
ABI against the oracle, on the problems and with the checks of tests/pod_operator_node_cases.py — the ones
tests/test_cursor_engine_pod_operators_nodes.py runs on the emulation, at the same small shapes. The kernels' names are asked of the
gfx950 build with -DKSOLVE_TEST_HOOKS (tests/emu/libksolve_hooks.so), as tests/test_gpu_kernel_table.py does."""
import pytest

import parity
import pod_operator_node_cases as nc
from gpu_support import built  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_nodes,block0_zone1", [(n, False) for n in nc.BLOCK_EDGES] + [(65, True), (129, True)])
def test_block_edges(oracle, n_nodes, block0_zone1):
    nc.check_block_edge(oracle, None, n_nodes, block0_zone1)


def test_one_custom_key_three_operators(oracle):
    nc.check_dedicated(oracle, None)


def test_notin_on_a_key_no_node_carries_and_no_positive_class_uses(oracle):
    nc.check_unused_key(oracle, None)


def test_exists_on_a_key_some_nodes_carry(oracle):
    nc.check_exists(oracle, None)


def test_reason_37_and_its_twin(oracle):
    nc.check_key_definedness(oracle, None)


def test_with_a_binding_limit(oracle):
    nc.check_limit(oracle, None)


def test_with_a_complement_nodepool(oracle):
    nc.check_complement_pool(oracle, None)


def test_with_daemonsets(oracle):
    nc.check_daemonsets(oracle, None)


def test_a_pod_that_excludes_every_zone(oracle):
    nc.check_no_zone(oracle, None)


def test_the_loops_declines_are_still_named(oracle):
    nc.check_loop_declines(oracle, None)


def test_lds_and_hbm_variants(oracle):
    nc.check_variants(oracle, None, parity.build_hooks())


def test_repeated_solves_give_one_digest(oracle):
    """As many solves as tests/test_gpu_cursor_nodes.py makes on one handle: class ids are drawn from an atomic counter and differ
    from solve to solve, the rows of the stage are computed with every solve's classes."""
    nc.check_repeated(oracle, None, 100)


def test_solve_many(oracle):
    nc.check_solve_many(oracle, None)


def test_seeded_fuzz(oracle):
    """Every fourth seed of test_cursor_engine_pod_operators_nodes.test_seeded_fuzz, under its conditions (four of five on the cursor
    engine, as tests/test_gpu_cursor_pod_operators.py asks of its share)."""
    on_cursor, rest, negative_on_nodes = nc.run_fuzz(oracle, None, nc.GPU_FUZZ_SEEDS)
    assert on_cursor * 5 >= len(nc.GPU_FUZZ_SEEDS) * 4, (on_cursor, rest)
    assert negative_on_nodes * 2 >= len(nc.GPU_FUZZ_SEEDS), negative_on_nodes
