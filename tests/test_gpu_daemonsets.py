"""GPU tests (run with -m gpu on an MI355X) of DaemonSet overhead on the cursor and spread engines: the product library
karpenter_amd/libksolve.so through the C ABI against the oracle on the same seeded inputs. Every case asserts the engine that ran and
fallback reason 0, so none can pass by falling back to the general engine. The emulation run is tests/test_fast_engines_daemonsets.py."""
import pytest

import daemonset_cases as dc
import engine_checks as ec
import parity
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd import fixtures as fx
from karpenter_amd.scheduling import NewScheduler
from test_fast_engines_daemonsets import CURSOR_SEEDS, SPREAD_SEEDS

pytestmark = pytest.mark.gpu


def test_known_answers_on_the_device(oracle):
    for name, prob in dc.known_answers():
        got, _ = dc.check_engine(oracle, None, prob, "cursor", ("cursor-wide", "cursor-hbm"))
        if name == "one-group":
            req = got["newNodeClaims"][0]["requests"]
            assert int(req["cpu"]) == 2 * 10**9 and int(req["pods"]) == 2 * 10**9


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_config2_with_daemonsets_on_the_cursor_engine(oracle, kind):
    got, _ = dc.check_engine(oracle, None, fx.with_daemonsets(fx.config2(pods=20000, n_types=500, seed=42), kind), "cursor", ("cursor-wide", "cursor-hbm"))
    assert got["scheduledPods"] == 20000


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_config3_with_daemonsets_on_the_spread_engine(oracle, kind):
    got, _ = dc.check_engine(oracle, None, fx.with_daemonsets(fx.config3(pods=20000, n_types=500, seed=42), kind), "spread")
    assert not got["podErrors"]


def test_fuzz_on_the_device(oracle):
    ran, _ = dc.run_fuzz(oracle, None, dc.cursor_fuzz_problem, CURSOR_SEEDS[:16], "cursor")
    assert ran >= 12, ran
    ran, _ = dc.run_fuzz(oracle, None, dc.spread_fuzz_problem, SPREAD_SEEDS[:16], "spread")
    assert ran >= 12, ran


def test_one_hundred_solves_of_one_handle(oracle):
    prob = fx.with_daemonsets(fx.config2(pods=6000, n_types=144, seed=3), "c")
    s = NewScheduler(prob)
    digests = set()
    for _ in range(100):
        r = s.Solve()
        assert r["counters"]["engine"] == "cursor" and r["counters"]["engineFallbackReason"] == 0
        digests.add(parity.results_digest(r)[0])
    s.close()
    assert len(digests) == 1
    ec.same(r, oracle.solve(prob), prob)
