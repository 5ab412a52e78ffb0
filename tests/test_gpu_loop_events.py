"""GPU tests of the tail behind the cursor engine's fast loop (fast_engine.h fast_hot_run): the shapes of tests/test_loop_events.py
on the device against the oracle, with the same caps on the one-pod loop's calls (5,638 and 1,534 before the tail), a 16-NodePool
batch, and four problems in one batched launch (ksolve_pack_fast_batch)."""
import pytest

import parity
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler, SolveBatch

pytestmark = pytest.mark.gpu


def same(got, want):
    assert got["counters"]["engine"] == "cursor"
    assert parity.results_digest(got)[0] == parity.results_digest(want)[0]
    assert got["counters"]["referenceBinEvaluations"] == want["counters"]["binEvaluations"]


# pods, types, NodeClaims, fullEvaluations as reported before the tail, the cap on the one-pod loop's calls (None: the claim count)
@pytest.mark.parametrize("pods,types,claims,full,cap", [(20000, 500, 57, 20000, 1500), (3000, 16, 525, 7005, None)])
def test_events_leave_the_one_pod_loop_on_the_device(oracle, pods, types, claims, full, cap):
    prob = fx.config2(pods=pods, n_types=types, seed=42)
    got = NewScheduler(prob).Solve()
    same(got, oracle.solve(prob))
    c = got["counters"]
    assert len(got["newNodeClaims"]) == claims and c["phaseCycles"][21] == full
    print(f"config2({pods}, {types}): one-pod loop calls {c['onePodLoopCalls']}")
    assert c["onePodLoopCalls"] < (claims if cap is None else cap)


def test_sixteen_nodepools_four_rows_on_the_device(oracle):
    """More than 64 classes live at once: ksolve_pack_fast_g0r4. The engine reports its rows where limits are set (phaseCycles[23]):
    the same problem with limits that never bind, under the setting that takes them."""
    prob = fx.config4(pods=8000, n_types=200, n_pools=16, seed=42)
    limited = dict(prob, nodePools=[dict(p, limits={"cpu": "100000000"}) for p in prob["nodePools"]], options=dict(prob["options"], engine="cursor-limits"))
    word = NewScheduler(limited).Solve()["counters"]["phaseCycles"][23]
    assert (word >> 16) & 0xFFFF == 4
    got = NewScheduler(prob).Solve()
    same(got, oracle.solve(prob))
    assert got["counters"]["phaseCycles"][21] == 8161        # fullEvaluations, as reported before the tail
    assert got["counters"]["onePodLoopCalls"] < 1000         # 5,574 before the tail


def test_events_in_a_batched_launch(oracle):
    """The unit of bench.py's batched leg (ksolve_pack_fast_batch, one wavefront per problem, maxClaims 1024), four of them."""
    probs = [dict(p, options=dict(p["options"], maxClaims=1024)) for p in (fx.config2(pods=20000, n_types=500, seed=1000 + i) for i in range(4))]
    for got, prob in zip(SolveBatch([NewScheduler(p) for p in probs]), probs):
        same(got, oracle.solve(prob))
        assert got["counters"]["onePodLoopCalls"] < 1500
