"""CPU tests of the spread engine's limit stages (csrc/topo_engine.h TopoEngine::limit_stage over csrc/fast_engine.h
limit_stage_id, engines "auto-limits-spread" / "spread-limits"): through the host emulation of the device code (tests/emu, test
infrastructure only), the real C ABI and the real flattener, against the oracle in claims, nodes, instance-type lists, pod
assignment and the reference-equivalent evaluation count. The problems are tests/spread_limit_cases.py's; the device run is
tests/test_gpu_spread_limits.py."""
import pytest

import engine_checks as ec
import limit_cases as lc
import spread_limit_cases as sl
import spread_node_cases as sn
from karpenter_amd.scheduling import Unsupported
from test_device_algorithm import emu  # noqa: F401  (fixture)


@pytest.mark.parametrize("cfg,limits,n_limited,n_open", sl.MIX)
def test_the_benchmark_mix_with_a_cpu_limit(oracle, emu, cfg, limits, n_limited, n_open):
    got, want = sl.check_engine(oracle, emu, sl.mix_problem(cfg, limits))
    assert (sl.pool_of(want).count("limited"), sl.pool_of(want).count("open")) == (n_limited, n_open) and not want["podErrors"]
    assert sl.stages(got)[0] >= 1 and sl.stages(got)[1] is not None


def test_node_limit(oracle, emu):
    got, want = sl.check_engine(oracle, emu, sl.mix_problem((300, 144, 1), {"nodes": "0"}))
    assert sl.pool_of(want) == ["open"] * 60
    assert sl.stages(got) == (0, None)
    assert ec.solve(sl.mix_problem((300, 144, 1), {"nodes": "0"}), "auto", emu)["counters"]["engineFallbackReason"] == 23
    # a limit that never binds: the spread engine under every setting, one digest
    loose = sl.mix_problem((300, 144, 1), {"nodes": "20"})
    want = oracle.solve(loose)
    digests = set()
    for engine in ("auto", "spread", "spread-limits", "auto-limits-spread"):
        r = ec.solve(loose, engine, emu)
        assert r["counters"]["engine"] == "spread" and r["counters"]["engineFallbackReason"] == 0, (engine, r["counters"])
        ec.same(r, want, loose)
        digests.add(sl.parity.results_digest(r)[0])
    assert len(digests) == 1 and sl.stages(r) == (0, None)


def test_zonal_chain(oracle, emu):
    got, want = sl.check_engine(oracle, emu, sl.zonal_chain_problem())
    assert (sl.pool_of(want).count("first"), sl.pool_of(want).count("second")) == (5, 10) and not want["podErrors"]
    assert sl.stages(got) == (0, 5)       # no list between "every type" and "none": no stage; the first exclusion with five claims open


def test_early_stage_claims_keep_accepting(oracle, emu):
    prob = sl.early_stage_problem()
    got, want = sl.check_engine(oracle, emu, prob)
    assert (sl.pool_of(want).count("first"), sl.pool_of(want).count("second")) == (5, 5) and not want["podErrors"]
    assert sl.early_claim_holds_a_small_pod(prob, want)
    assert sl.stages(got) == (1, 4)       # 36 -> 28 -> 20 -> 12 -> 4: the types above 4 cpu leave the list with four claims open


def test_stage_exhaustion(oracle, emu):
    got, want = sl.check_engine(oracle, emu, sl.stage_chain_problem(3))
    assert all(sl.pool_of(want).count(f"pool-{i}") == 7 for i in range(3)) and sl.pool_of(want).count("catch-all") == 6
    assert sl.stages(got)[0] == 21
    sl.check_declined(oracle, emu, sl.stage_chain_problem(4), 29)


def test_with_existing_nodes_and_daemonsets(oracle, emu):
    prob = sl.mix_nodes_problem()
    got, want = sl.check_engine(oracle, emu, prob, base="auto-nodes-spread")
    assert sn.on_nodes(want) == 129 and (sl.pool_of(want).count("limited"), sl.pool_of(want).count("open")) == (4, 52) and not want["podErrors"]
    assert sl.stages(got) == (4, 0)       # limits.cpu = 100 is less than the largest types hold: the first claim already opens under a narrowed list


def test_repeated_solves_on_one_handle(oracle, emu):
    prob = sl.zonal_chain_problem()
    digests, words, last = sl.repeated_solves(emu, prob, "auto-limits-spread", 100)
    assert len(digests) == 1 and words == {(0, 5)}
    ec.same(last, oracle.solve(prob), prob)
    # ... and with stages to forget
    prob = sl.stage_chain_problem(3)
    digests, words, last = sl.repeated_solves(emu, prob, "spread-limits", 20)
    assert len(digests) == 1 and {w[0] for w in words} == {21}
    ec.same(last, oracle.solve(prob), prob)


def test_seeded_fuzz(oracle, emu):
    assert sl.run_fuzz(oracle, emu, sl.FUZZ_SEEDS) > 0


def test_engines_0_to_12_are_unchanged(oracle, emu):
    """The parent's behaviour: "auto" and "auto-limits" end on the general engine with the limit's reason, "spread" refuses and
    names it; a topology-free problem under 13 runs on the cursor engine with its stages."""
    for prob in (sl.mix_problem(*sl.MIX[0][:2]), sl.zonal_chain_problem()):
        for engine in ("auto", "auto-limits"):
            c = ec.solve(prob, engine, emu)["counters"]
            assert (c["engine"], c["engineFallbackReason"]) == ("general", 24), (engine, c)
        with pytest.raises(Unsupported, match=r"spread engine declined the problem \(reason 24\)"):
            ec.solve(prob, "spread", emu)
    prob = lc.cpu_chain_problem(True)
    got = ec.solve(prob, "auto-limits-spread", emu)
    assert got["counters"]["engine"] == "cursor" and got["counters"]["engineFallbackReason"] == 0 and lc.stages(got) == (0, 5)
    ec.same(got, oracle.solve(prob), prob)
