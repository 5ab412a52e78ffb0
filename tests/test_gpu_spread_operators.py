"""GPU tests (run with -m gpu on an MI355X) of the spread engine's complement templates (csrc/topo_engine.h "Complement templates on
the spread engine", csrc/fast_engine.h FastCold::setup, ksolve_fast_records; engines "auto-operators-spread" / "spread-operators"):
the product library through the C ABI against the oracle, on the problems of tests/spread_operator_cases.py — the ones
tests/test_spread_engine_operators.py runs on the emulation, at the same small shapes."""
import pytest

import engine_checks as ec
import limit_cases as lc
import operator_cases as oc
import spread_limit_cases as sl
import spread_node_cases as sn
import spread_operator_cases as so
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd import fixtures as fx

pytestmark = pytest.mark.gpu


def test_notin_on_the_spread_key(oracle):
    got, want = so.check_engine(oracle, None, oc.spread_problem(), 3)
    assert {so.zone_of(c) for c in so.claims_of(got, "not-zone-1")} >= {("In", ("test-zone-2",)), ("In", ("test-zone-3",))}
    assert all("test-zone-1" not in so.zone_of(c)[1] or so.zone_of(c)[0] == "NotIn" for c in so.claims_of(got, "not-zone-1"))
    assert any(so.zone_of(c) == ("In", ("test-zone-1",)) for c in so.claims_of(got, "open"))


def test_counted_but_not_narrowed(oracle):
    prob = so.counted_problem()
    got, want = so.check_engine(oracle, None, prob, 3)
    kept = [c for c in so.claims_of(got, "only-3") if so.zone_of(c) == ("NotIn", ("test-zone-1", "test-zone-2"))]
    assert len(kept) == 3 and all(len(c["pods"]) == 1 for c in kept)
    assert so.pods_by_zone(got, so.spread_uids(prob)) == {"test-zone-1": 2, "test-zone-2": 2, "test-zone-3": 2}
    concrete = so.counted_problem("In")
    other = ec.solve(concrete, so.ONLY, None)
    ec.same(other, oracle.solve(concrete), concrete)
    assert so.pods_by_zone(other, so.spread_uids(concrete)) == {"test-zone-1": 3, "test-zone-2": 3}


def test_bounds(oracle):
    got, want = so.check_engine(oracle, None, so.bounds_problem(), 0)
    above = so.claims_of(got, "above")
    assert above
    for c in above:
        r = so.integer_req(c)
        assert (r["operator"], r["complement"], r["values"], r["gte"], r["lte"]) == ("Exists", True, [], 3, None)


def test_two_dictionary_key_groups(oracle):
    got, want = so.check_engine(oracle, None, so.two_keys_problem(), 3)
    assert so.claims_of(got, "both")


def test_zonal_anti_affinity_and_affinity(oracle):
    got, want = so.check_engine(oracle, None, so.affinity_problem(), 3)
    assert so.claims_of(got, "not-zone-1") and so.claims_of(got, "open")


def test_does_not_exist_on_the_spread_key(oracle):
    got, want = so.check_engine(oracle, None, so.does_not_exist_problem(), 3)
    assert not so.claims_of(got, "nowhere") and so.claims_of(got, "open")


def test_limit_stages(oracle):
    for prob, bare in ((so.limit_mix_problem(), sl.mix_problem(*sl.MIX[0][:2])), (so.limit_chain_problem(), sl.zonal_chain_problem())):
        got, want = so.check_engine(oracle, None, prob, 0)
        assert sl.stages(got) == sl.stages(ec.solve(bare, "auto-limits-spread", None)) and sl.stages(got)[1] is not None
        assert all((fx.FAKE_INTEGER_LABEL, "Exists", 1, None) in so.complement_kinds(c) for c in got["newNodeClaims"])
    prob = so.limit_notin_problem()
    got, want = so.check_engine(oracle, None, prob, 3)
    cpus = lc.cpu_of(prob)
    assert sl.stages(got)[0] >= 1
    assert any(so.zone_of(c) == ("NotIn", ("test-zone-1",)) for c in so.claims_of(got, "not-zone-1") if lc.max_cpu(c, cpus) < 8)


def test_existing_nodes(oracle):
    for prob in (so.nodes_mix_problem(), so.nodes_limit_problem()):
        want = oracle.solve(prob)
        assert not want["podErrors"] and sn.on_nodes(want) > 0
        plain = ec.solve(prob, "auto-nodes-spread", None)
        assert (plain["counters"]["engine"], plain["counters"]["engineFallbackReason"]) == ("general", 34), plain["counters"]
        got = ec.solve(prob, so.AUTO, None)
        assert (got["counters"]["engine"], got["counters"]["engineFallbackReason"]) == ("spread", 0), got["counters"]
        ec.same(got, want, prob)
        assert sn.on_nodes(got) == sn.on_nodes(want)


def test_daemonset_overhead(oracle):
    so.check_engine(oracle, None, so.daemonset_problem(), 3)


def test_still_outside_the_shape(oracle):
    so.check_declined(oracle, None, so.pod_notin_problem(), 4)
    so.check_declined(oracle, None, so.pod_gt_problem(), 1)
    so.check_declined(oracle, None, so.min_values_problem(), 1)
    so.check_declined(oracle, None, so.node_filter_problem(), 43)


def test_cursor_side_of_auto_operators_spread():
    for prob in (oc.notin_problem(), oc.bounds_problem()):
        cell = so.lone_cell(None, prob, so.AUTO)
        assert cell[:2] == ("cursor", 0) and cell == so.lone_cell(None, prob, "auto-operators")


def test_repeated_solves():
    for prob in (oc.spread_problem(), so.limit_mix_problem()):
        digests, words, _ = sl.repeated_solves(None, prob, so.ONLY, 50)
        assert len(digests) == 1 and len(words) == 1


def test_in_a_batch():
    probs = [oc.spread_problem(), so.counted_problem(), so.bounds_problem()]
    for engine in (so.AUTO, so.ONLY):
        cells = so.batch_cells(None, probs, engine)
        assert [c[:2] for c in cells] == [("spread", 0)] * 3
        assert cells == [so.lone_cell(None, p, engine) for p in probs]


def test_old_settings_stay_as_they_are():
    prob = oc.spread_problem()
    for engine in ("auto", "auto-operators"):
        assert so.lone_cell(None, prob, engine)[:2] == ("general", 3)
    for engine in ("spread", "spread-limits"):
        assert "spread engine declined the problem (reason 3)" in ec.refusal(prob, engine, None)
    prob = so.bounds_problem()
    for engine in ("auto", "auto-operators"):
        assert so.lone_cell(None, prob, engine)[:2] == ("general", 0)
    assert "spread engine requested for a problem outside its shape" in ec.refusal(prob, "spread", None)


def test_seeded_fuzz(oracle):
    """Thirty of the 120 seeds of test_spread_engine_operators.test_seeded_fuzz (every fourth), under its conditions: each equals the
    oracle, reason 27 and nothing else off the spread engine, three in four on it, more than half of those over a pool that is not In."""
    on_spread, non_in, rest = so.run_fuzz(oracle, None, so.GPU_FUZZ_SEEDS)
    assert on_spread * 4 >= len(so.GPU_FUZZ_SEEDS) * 3, (on_spread, rest)
    assert non_in * 2 > on_spread, (non_in, on_spread)
