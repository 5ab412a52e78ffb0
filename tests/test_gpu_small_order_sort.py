"""GPU tests of the cursor engine's slow sort on small claim orders (pdq_emul.h RegOrder: at most 64 claims sorted in two vector
registers; above that the LDS-resident order is scanned 512 positions per step): solves that spend their whole life, or most of it,
with 13 to 64 claims in flight, against the oracle. The CPU run of the same code is tests/test_small_order_sort.py; orders of
512 claims and more are held by test_gpu_parity.py::test_full_size_digest."""
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


# 57 NodeClaims (every slow sort at n < 58), and 73 (across the hand-over from registers to LDS at 64 / 65)
@pytest.mark.parametrize("pods,claims", [(20000, 57), (26000, 73)])
def test_small_orders_on_the_device(oracle, pods, claims):
    prob = fx.config2(pods=pods, n_types=500, seed=42)
    want = oracle.solve(prob)
    got = NewScheduler(prob).Solve()
    assert len(got["newNodeClaims"]) == claims and got["counters"]["slowSorts"] >= 3000
    same(got, want)


def test_small_orders_in_a_batched_launch(oracle):
    """The unit of bench.py's batched leg (ksolve_pack_fast_batch, one wavefront per problem, maxClaims 1024), four of them."""
    probs = [dict(p, options=dict(p["options"], maxClaims=1024)) for p in (fx.config2(pods=20000, n_types=500, seed=1000 + i) for i in range(4))]
    for got, prob in zip(SolveBatch([NewScheduler(p) for p in probs]), probs):
        same(got, oracle.solve(prob))
