"""GPU tests of the cursor engine's existing-node stage (ksolve_pack_nodes, csrc/node_stage.h) on the device library: the cases of
tests/test_cursor_engine_nodes.py that exercise the kernel's paths, against the oracle."""
import pytest

import engine_checks as ec
import existing_node_cases as en
import parity
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_nodes", en.BLOCK_EDGES)
def test_block_edges(oracle, n_nodes):
    got, want = en.check_engine(oracle, None, en.block_edge_problem(n_nodes), variant=1)
    assert en.on_nodes(got) >= 2 and got["newNodeClaims"]


def test_extremes_and_negative_remaining(oracle):
    got, _ = en.check_engine(oracle, None, en.all_on_nodes_problem())
    assert not got["newNodeClaims"] and en.on_nodes(got) == 12
    got, _ = en.check_engine(oracle, None, en.none_on_nodes_problem())
    assert en.on_nodes(got) == 0 and got["newNodeClaims"]
    en.check_engine(oracle, None, en.negative_remaining_problem())


@pytest.fixture(scope="module")
def big():
    return fx.with_daemonsets(fx.config2(pods=20000, n_types=500, seed=7), "c")


@pytest.mark.parametrize("n_nodes,variant,fill", [(300, 1, (0.2, 0.9)), (3100, 2, (0.9, 1.0))])
def test_production_like_both_memory_variants(oracle, big, n_nodes, variant, fill):
    """config2(pods=20000, n_types=500) with DaemonSets and 300 nodes (remaining resources in LDS); and with 3,100 nearly full
    small nodes, past kNodeStageLdsRem (3,072 nodes at four resource dimensions): the HBM variant."""
    prob = fx.with_existing_nodes(big, n_nodes, seed=5, fill=fill, small=variant == 2)
    got, _ = en.check_engine(oracle, None, prob, variant=variant)
    assert en.on_nodes(got) > 300 and got["newNodeClaims"] and not got["podErrors"]


def test_fuzz_seeds(oracle):
    ran, placed, _ = en.run_fuzz(oracle, None, range(16))
    assert ran >= 12 and placed > 0


def test_hundred_solves_one_digest(oracle):
    prob = fx.with_daemonsets(fx.with_existing_nodes(fx.config2(pods=3000, n_types=144, seed=8), 100, seed=4), "b")
    s = NewScheduler(dict(prob, options=dict(prob["options"], engine="cursor-nodes")))
    digests = set()
    for _ in range(100):
        r = s.Solve()
        digests.add(parity.results_digest(r)[0])
    s.close()
    assert r["counters"]["engine"] == "cursor" and len(digests) == 1
    ec.same(r, oracle.solve(prob), prob)
