"""GPU tests of the spread engine's existing-node path (ksolve_pack_topo_nodes, csrc/topo_nodes.h) on the device library: the cases
of tests/test_spread_engine_nodes.py that cross a 64-node block and a claim window, against the oracle."""
import pytest

import engine_checks as ec
import parity
import spread_node_cases as sn
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler

pytestmark = pytest.mark.gpu


def test_the_benchmark_mix_with_nodes_and_daemonsets(oracle):
    cfg, n_nodes, _, with_ds = sn.MIX[1]
    got, want = sn.check_engine(oracle, None, sn.mix_problem(cfg, n_nodes, daemonsets=True))
    assert (sn.on_nodes(want), len(want["newNodeClaims"])) == with_ds and not want["podErrors"]
    assert sn.on_nodes(got) > 0 and got["newNodeClaims"]


@pytest.mark.parametrize("n_nodes", sn.BLOCK_EDGES)
def test_block_edges(oracle, n_nodes):
    got, want = sn.check_engine(oracle, None, sn.block_edge_problem(n_nodes))
    assert f"node-{n_nodes - 1:04d}" in {e["name"] for e in got["existingNodes"] if e["pods"]} and got["newNodeClaims"]


def test_a_node_refuses_and_later_accepts(oracle):
    prob = sn.refuse_then_accept_problem()
    got, want = sn.check_engine(oracle, None, prob)
    assert sn.node_then_claim_then_node(want, prob)


def test_fuzz_seeds(oracle):
    cands, ran, placed, _ = sn.run_fuzz(oracle, None, range(24))
    assert cands >= 8, cands
    assert ran * 3 >= cands * 2 and placed > 0, (ran, cands)


def test_hundred_solves_one_digest(oracle):
    prob = fx.with_existing_nodes(fx.config3(pods=3000, n_types=144, seed=8), 100, seed=4)
    s = NewScheduler(dict(prob, options=dict(prob["options"], engine="spread-nodes")))
    digests = set()
    for _ in range(100):
        r = s.Solve()
        digests.add(parity.results_digest(r)[0])
    s.close()
    assert r["counters"]["engine"] == "spread" and r["counters"]["engineFallbackReason"] == 0 and len(digests) == 1
    assert sn.on_nodes(r) > 0
    assert digests == {parity.results_digest(oracle.solve(prob))[0]}
    ec.same(r, oracle.solve(prob), prob)
