"""CPU tests of the spread engine's topology node filters (csrc/topo_engine.h "Topology node filters": setup_filters, claim_cut, the
five Record sites; csrc/topo_nodes.h topo_node_filter_cut; engines "auto-filters-spread" / "spread-filters"): through the host
emulation of the device code (tests/emu, test infrastructure only), the real C ABI and the real flattener, against the oracle in
claims, instance-type lists, claim requirements, pod assignment, pod errors, queue pops and the reference-equivalent evaluation count.
The problems are tests/spread_filter_cases.py's; the device run is tests/test_gpu_spread_filters.py."""
import engine_checks as ec
import spread_filter_cases as sf
import spread_limit_cases as sl
import spread_node_cases as sn
import spread_operator_cases as so
from karpenter_amd import fixtures as fx
from test_device_algorithm import emu  # noqa: F401  (fixture)


def pair(oracle, lib, filtered, other, other_filtered=True):
    """Both problems of a pair through the common check (the other one through check_open when it has no filter that can say no);
    -> the oracle's owners per zone of each, and the engine's equal them (the results are equal)."""
    got, want = sf.check_engine(oracle, lib, filtered)
    got2, want2 = (sf.check_engine if other_filtered else sf.check_open)(oracle, lib, other)
    return sf.owners_by_zone(want, filtered), sf.owners_by_zone(want2, other)


def test_owner_only(oracle, emu):
    """The owner's own pods always match its filter: resolved ALWAYS at set-up, no slot."""
    sf.check_engine(oracle, emu, so.node_filter_problem())


def test_never_counted(oracle, emu):
    assert pair(oracle, emu, sf.never_problem(), sf.never_problem("Ignore"), False) == (sf.NOT_COUNTED, sf.COUNTED)


def test_dynamic_by_template(oracle, emu):
    assert pair(oracle, emu, sf.by_template_problem(sf.SPOT), sf.by_template_problem(sf.ON_DEMAND)) == (sf.NOT_COUNTED, sf.COUNTED)


def test_undefined_against_defined(oracle, emu):
    """capacity-type is well known; the strict Compatible of the filter fails it all the same on a claim that does not define it."""
    assert pair(oracle, emu, sf.undefined_problem(), sf.undefined_problem("Ignore"), False) == (sf.NOT_COUNTED, sf.COUNTED)


def test_undefined_then_concrete(oracle, emu):
    z1, z2, z3 = sf.ZONES
    assert pair(oracle, emu, sf.then_concrete_problem(), sf.then_concrete_problem(False)) == ({z2: 2, z3: 2}, {z1: 1, z2: 2, z3: 1})


def test_complement_template(oracle, emu):
    assert pair(oracle, emu, sf.complement_problem(sf.ON_DEMAND), sf.complement_problem(sf.SPOT)) == (sf.NOT_COUNTED, sf.COUNTED)


def test_custom_key(oracle, emu):
    assert pair(oracle, emu, sf.custom_key_problem("b"), sf.custom_key_problem("a")) == (sf.NOT_COUNTED, sf.COUNTED)


def test_hostname_spread_with_a_filter(oracle, emu):
    """The uncounted pod does not use up the owner's maxSkew on its claim: three claims; with Ignore it does: four."""
    got, want = sf.check_engine(oracle, emu, sf.hostname_problem())
    other, want2 = sf.check_open(oracle, emu, sf.hostname_problem("Ignore"))
    assert (len(want["newNodeClaims"]), len(want2["newNodeClaims"])) == (3, 4)
    assert (len(got["newNodeClaims"]), len(other["newNodeClaims"])) == (3, 4)


def test_two_keys_in_one_selector(oracle, emu):
    assert pair(oracle, emu, sf.two_keys_problem("b"), sf.two_keys_problem("a")) == (sf.NOT_COUNTED, sf.COUNTED)


def test_taint_policy(oracle, emu):
    assert pair(oracle, emu, sf.taint_problem("Honor"), sf.taint_problem(None), False) == (sf.NOT_COUNTED, sf.COUNTED)


def test_limit_stage(oracle, emu):
    """The claims of the tainted pool's limit stage carry the stage's id: it resolves to the tainted template, and they are not counted."""
    prob = sf.limit_stage_problem("Honor")
    got, want = sf.check_engine(oracle, emu, prob)
    assert sl.stages(got)[0] >= 1 and len(so.claims_of(got, "tainted")) >= 3
    other = sf.limit_stage_problem(None)
    got2, want2 = sf.check_open(oracle, emu, other)
    assert (sf.owners_by_zone(want, prob), sf.owners_by_zone(want2, other)) == (sf.NOT_COUNTED, sf.COUNTED)


def test_existing_nodes(oracle, emu):
    z1, z2, z3 = sf.ZONES
    spot, on_demand = sf.node_problem(), sf.node_problem(capacity_type=sf.ON_DEMAND)
    assert pair(oracle, emu, spot, on_demand) == ({z1: 2, z2: 2, z3: 1}, {z2: 2, z3: 3})
    got, want = sf.check_engine(oracle, emu, sf.node_problem(fx.HOSTNAME))
    assert sn.on_nodes(got) == sn.on_nodes(want) == 3
    # a tainted node under Honor: reason 43 from create() under 22, a filter slot under 24 / 25
    tainted, plain = sf.tainted_node_problem("Honor"), sf.tainted_node_problem(None)
    assert pair(oracle, emu, tainted, plain, False) == ({z1: 2, z2: 2, z3: 1}, {z2: 2, z3: 3})


def test_set_aside_pods(oracle, emu):
    """Unschedulable pods in the same batch — one too big, the others out of limit: errors and pops as the oracle's second round leaves them."""
    prob = sf.set_aside_problem()
    want = oracle.solve(prob)
    assert len(want["podErrors"]) >= 2 and want["counters"]["pops"] > len(prob["pods"])
    sf.check_engine(oracle, emu, prob, want)


def test_still_outside_the_shape(oracle, emu):
    sf.check_declined(oracle, emu, sf.pod_notin_problem(), 4)
    sf.check_declined(oracle, emu, sf.too_many_slots_problem(), 43)
    sf.check_engine(oracle, emu, sf.too_many_slots_problem(16))   # (sixteen fit)
    sf.check_declined(oracle, emu, sf.preference_problem(), 41)


def test_old_settings_stay_as_they_are(emu):
    """Cases 1 and 10 under the settings that exist: ("general", 43), and the refusal of "spread-unschedulable" names 43. One cell
    cannot read 43: case 1 is spread_operator_cases.node_filter_problem() as it stands, over a NodePool with zone NotIn, and "auto"
    — which takes no complement template — stops at reason 3 before it looks at a filter, as
    test_spread_engine_operators.test_old_settings_stay_as_they_are pins for that pool. The cell is asserted as it is, and the
    same pods over the open pool alone give "auto" its 43."""
    for prob in (so.node_filter_problem(), sf.taint_problem("Honor")):
        for engine in ("auto", "auto-operators-spread", "auto-unschedulable-spread"):
            complement = engine == "auto" and so.has_non_in_pool(prob)
            assert sf.lone_cell(emu, prob, engine)[:2] == ("general", 3 if complement else 43), engine
        assert "spread engine declined the problem (reason 43)" in ec.refusal(prob, "spread-unschedulable", emu)
    prob = so.node_filter_problem()
    positive = dict(prob, nodePools=[p for p in prob["nodePools"] if p["name"] == "open"])
    assert not so.has_non_in_pool(positive) and sf.lone_cell(emu, positive, "auto")[:2] == ("general", 43)


def test_repeated_solves(emu):
    for prob in (sf.then_concrete_problem(), sf.limit_stage_problem("Honor")):
        digests, words, _ = sf.repeated_solves(emu, prob, sf.ONLY, 50)
        assert len(digests) == 1 and len(words) == 1


def test_in_a_batch(emu):
    probs = [sf.by_template_problem(), sf.complement_problem(), sf.node_problem()]
    for engine in (sf.AUTO, sf.ONLY):
        cells = sf.batch_cells(emu, probs, engine)
        assert [c[:2] for c in cells] == [("spread", 0)] * 3
        assert cells == [sf.lone_cell(emu, p, engine) for p in probs]


def test_seeded_fuzz(oracle, emu):
    """120 seeds of sf.fuzz_problem: each equals the oracle under "auto-filters-spread"; at least three quarters end on the spread
    engine with reason 0, the others leave it with a reason of sf.FUZZ_REASONS; at least half of the seeds on the spread engine are
    discriminating — the oracle's own result changes when every constraint's two policies are set to Ignore."""
    on_spread, disc, rest = sf.run_fuzz(oracle, emu, sf.FUZZ_SEEDS)
    assert on_spread * 4 >= len(sf.FUZZ_SEEDS) * 3, (on_spread, rest)
    assert disc * 2 >= on_spread, (disc, on_spread)
