"""GPU tests (run with -m gpu on an MI355X) of the spread engine's limit stages (csrc/topo_engine.h TopoEngine::limit_stage,
engines "auto-limits-spread" / "spread-limits"): the product library through the C ABI against the oracle, on the problems of
tests/spread_limit_cases.py — the ones tests/test_spread_engine_limits.py runs on the emulation, at the same small shapes."""
import pytest

import engine_checks as ec
import limit_cases as lc
import parity
import spread_limit_cases as sl
import spread_node_cases as sn
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd.scheduling import Unsupported

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cfg,limits,n_limited,n_open", sl.MIX)
def test_the_benchmark_mix_with_a_cpu_limit(oracle, cfg, limits, n_limited, n_open):
    got, want = sl.check_engine(oracle, None, sl.mix_problem(cfg, limits))
    assert (sl.pool_of(want).count("limited"), sl.pool_of(want).count("open")) == (n_limited, n_open) and not want["podErrors"]
    assert sl.stages(got)[0] >= 1 and sl.stages(got)[1] is not None


def test_node_limit(oracle):
    got, want = sl.check_engine(oracle, None, sl.mix_problem((300, 144, 1), {"nodes": "0"}))
    assert sl.pool_of(want) == ["open"] * 60 and sl.stages(got) == (0, None)
    loose = sl.mix_problem((300, 144, 1), {"nodes": "20"})
    want = oracle.solve(loose)
    digests = set()
    for engine in ("auto", "spread-limits"):
        r = ec.solve(loose, engine, None)
        assert r["counters"]["engine"] == "spread" and r["counters"]["engineFallbackReason"] == 0, (engine, r["counters"])
        ec.same(r, want, loose)
        digests.add(parity.results_digest(r)[0])
    assert len(digests) == 1 and sl.stages(r) == (0, None)


def test_zonal_chain(oracle):
    got, want = sl.check_engine(oracle, None, sl.zonal_chain_problem())
    assert (sl.pool_of(want).count("first"), sl.pool_of(want).count("second")) == (5, 10)
    assert sl.stages(got) == (0, 5)


def test_early_stage_claims_keep_accepting(oracle):
    prob = sl.early_stage_problem()
    got, want = sl.check_engine(oracle, None, prob)
    assert (sl.pool_of(want).count("first"), sl.pool_of(want).count("second")) == (5, 5)
    assert sl.early_claim_holds_a_small_pod(prob, want) and sl.stages(got) == (1, 4)


def test_stage_exhaustion(oracle):
    got, want = sl.check_engine(oracle, None, sl.stage_chain_problem(3))
    assert all(sl.pool_of(want).count(f"pool-{i}") == 7 for i in range(3)) and sl.stages(got)[0] == 21
    sl.check_declined(oracle, None, sl.stage_chain_problem(4), 29)


def test_with_existing_nodes_and_daemonsets(oracle):
    got, want = sl.check_engine(oracle, None, sl.mix_nodes_problem(), base="auto-nodes-spread")
    assert sn.on_nodes(want) == 129 and (sl.pool_of(want).count("limited"), sl.pool_of(want).count("open")) == (4, 52)
    assert sl.stages(got) == (4, 0)


def test_repeated_solves_on_one_handle(oracle):
    prob = sl.zonal_chain_problem()
    digests, words, last = sl.repeated_solves(None, prob, "auto-limits-spread", 100)
    assert len(digests) == 1 and words == {(0, 5)}
    ec.same(last, oracle.solve(prob), prob)
    prob = sl.stage_chain_problem(3)
    digests, words, last = sl.repeated_solves(None, prob, "spread-limits", 20)
    assert len(digests) == 1 and {w[0] for w in words} == {21}
    ec.same(last, oracle.solve(prob), prob)


def test_seeded_fuzz(oracle):
    """The first eight of the fifteen seeds test_spread_engine_limits.test_seeded_fuzz keeps on the spread engine."""
    assert sl.run_fuzz(oracle, None, sl.FUZZ_ON_SPREAD[:8]) > 0


def test_engines_0_to_12_are_unchanged(oracle):
    for prob in (sl.mix_problem(*sl.MIX[0][:2]), sl.zonal_chain_problem()):
        for engine in ("auto", "auto-limits"):
            c = ec.solve(prob, engine, None)["counters"]
            assert (c["engine"], c["engineFallbackReason"]) == ("general", 24), (engine, c)
        with pytest.raises(Unsupported, match=r"spread engine declined the problem \(reason 24\)"):
            ec.solve(prob, "spread", None)
    prob = lc.cpu_chain_problem(True)
    got = ec.solve(prob, "auto-limits-spread", None)
    assert got["counters"]["engine"] == "cursor" and got["counters"]["engineFallbackReason"] == 0 and lc.stages(got) == (0, 5)
    ec.same(got, oracle.solve(prob), prob)
