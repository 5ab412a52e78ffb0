"""GPU tests (run with -m gpu on an MI355X) of the spread engine's topology node filters (csrc/topo_engine.h "Topology node filters";
kernels ksolve_pack_topo_f / ksolve_pack_topo_nodes_f; engines "auto-filters-spread" / "spread-filters"): the product library
through the C ABI against the oracle, on the problems of tests/spread_filter_cases.py — the ones
tests/test_spread_engine_filters.py runs on the emulation, at the same small shapes."""
import pytest

import engine_checks as ec
import spread_filter_cases as sf
import spread_limit_cases as sl
import spread_node_cases as sn
import spread_operator_cases as so
import test_spread_engine_filters as cpu
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd import fixtures as fx

pytestmark = pytest.mark.gpu


def test_owner_only(oracle):
    sf.check_engine(oracle, None, so.node_filter_problem())


def test_never_counted(oracle):
    assert cpu.pair(oracle, None, sf.never_problem(), sf.never_problem("Ignore"), False) == (sf.NOT_COUNTED, sf.COUNTED)


def test_dynamic_by_template(oracle):
    assert cpu.pair(oracle, None, sf.by_template_problem(sf.SPOT), sf.by_template_problem(sf.ON_DEMAND)) == (sf.NOT_COUNTED, sf.COUNTED)


def test_undefined_against_defined(oracle):
    assert cpu.pair(oracle, None, sf.undefined_problem(), sf.undefined_problem("Ignore"), False) == (sf.NOT_COUNTED, sf.COUNTED)


def test_undefined_then_concrete(oracle):
    z1, z2, z3 = sf.ZONES
    assert cpu.pair(oracle, None, sf.then_concrete_problem(), sf.then_concrete_problem(False)) == ({z2: 2, z3: 2}, {z1: 1, z2: 2, z3: 1})


def test_complement_template(oracle):
    assert cpu.pair(oracle, None, sf.complement_problem(sf.ON_DEMAND), sf.complement_problem(sf.SPOT)) == (sf.NOT_COUNTED, sf.COUNTED)


def test_custom_key(oracle):
    assert cpu.pair(oracle, None, sf.custom_key_problem("b"), sf.custom_key_problem("a")) == (sf.NOT_COUNTED, sf.COUNTED)


def test_hostname_spread_with_a_filter(oracle):
    got, want = sf.check_engine(oracle, None, sf.hostname_problem())
    other, want2 = sf.check_open(oracle, None, sf.hostname_problem("Ignore"))
    assert (len(got["newNodeClaims"]), len(other["newNodeClaims"])) == (3, 4)


def test_two_keys_in_one_selector(oracle):
    assert cpu.pair(oracle, None, sf.two_keys_problem("b"), sf.two_keys_problem("a")) == (sf.NOT_COUNTED, sf.COUNTED)


def test_taint_policy(oracle):
    assert cpu.pair(oracle, None, sf.taint_problem("Honor"), sf.taint_problem(None), False) == (sf.NOT_COUNTED, sf.COUNTED)


def test_limit_stage(oracle):
    prob = sf.limit_stage_problem("Honor")
    got, want = sf.check_engine(oracle, None, prob)
    assert sl.stages(got)[0] >= 1 and len(so.claims_of(got, "tainted")) >= 3
    other = sf.limit_stage_problem(None)
    got2, want2 = sf.check_open(oracle, None, other)
    assert (sf.owners_by_zone(got, prob), sf.owners_by_zone(got2, other)) == (sf.NOT_COUNTED, sf.COUNTED)


def test_existing_nodes(oracle):
    z1, z2, z3 = sf.ZONES
    assert cpu.pair(oracle, None, sf.node_problem(), sf.node_problem(capacity_type=sf.ON_DEMAND)) == ({z1: 2, z2: 2, z3: 1}, {z2: 2, z3: 3})
    got, want = sf.check_engine(oracle, None, sf.node_problem(fx.HOSTNAME))
    assert sn.on_nodes(got) == sn.on_nodes(want) == 3
    assert cpu.pair(oracle, None, sf.tainted_node_problem("Honor"), sf.tainted_node_problem(None), False) == ({z1: 2, z2: 2, z3: 1}, {z2: 2, z3: 3})


def test_set_aside_pods(oracle):
    prob = sf.set_aside_problem()
    want = oracle.solve(prob)
    assert len(want["podErrors"]) >= 2 and want["counters"]["pops"] > len(prob["pods"])
    sf.check_engine(oracle, None, prob, want)


def test_still_outside_the_shape(oracle):
    sf.check_declined(oracle, None, sf.pod_notin_problem(), 4)
    sf.check_declined(oracle, None, sf.too_many_slots_problem(), 43)
    sf.check_engine(oracle, None, sf.too_many_slots_problem(16))
    sf.check_declined(oracle, None, sf.preference_problem(), 41)


def test_old_settings_stay_as_they_are():
    """Cases 1 and 10 under the settings that exist: ("general", 43), and the refusal of "spread-unschedulable" names 43. One cell
    cannot read 43: case 1 is spread_operator_cases.node_filter_problem() as it stands, over a NodePool with zone NotIn, and "auto"
    — which takes no complement template — stops at reason 3 before it looks at a filter, as
    test_spread_engine_operators.test_old_settings_stay_as_they_are pins for that pool. The cell is asserted as it is, and the
    same pods over the open pool alone give "auto" its 43."""
    for prob in (so.node_filter_problem(), sf.taint_problem("Honor")):
        for engine in ("auto", "auto-operators-spread", "auto-unschedulable-spread"):
            complement = engine == "auto" and so.has_non_in_pool(prob)
            assert sf.lone_cell(None, prob, engine)[:2] == ("general", 3 if complement else 43), engine
        assert "spread engine declined the problem (reason 43)" in ec.refusal(prob, "spread-unschedulable", None)
    prob = so.node_filter_problem()
    positive = dict(prob, nodePools=[p for p in prob["nodePools"] if p["name"] == "open"])
    assert not so.has_non_in_pool(positive) and sf.lone_cell(None, positive, "auto")[:2] == ("general", 43)


def test_repeated_solves():
    for prob in (sf.then_concrete_problem(), sf.limit_stage_problem("Honor")):
        digests, words, _ = sf.repeated_solves(None, prob, sf.ONLY, 50)
        assert len(digests) == 1 and len(words) == 1


def test_in_a_batch():
    probs = [sf.by_template_problem(), sf.complement_problem(), sf.node_problem()]
    for engine in (sf.AUTO, sf.ONLY):
        cells = sf.batch_cells(None, probs, engine)
        assert [c[:2] for c in cells] == [("spread", 0)] * 3
        assert cells == [sf.lone_cell(None, p, engine) for p in probs]


def test_seeded_fuzz(oracle):
    """Every fourth of the 120 seeds of test_spread_engine_filters.test_seeded_fuzz, under its conditions."""
    on_spread, disc, rest = sf.run_fuzz(oracle, None, sf.GPU_FUZZ_SEEDS)
    assert on_spread * 4 >= len(sf.GPU_FUZZ_SEEDS) * 3, (on_spread, rest)
    assert disc * 2 >= on_spread, (disc, on_spread)
