"""CPU tests of the spread engine's complement templates (csrc/topo_engine.h "Complement templates on the spread engine",
csrc/fast_engine.h FastCold::setup, the records of ksolve_fast_records; engines "auto-operators-spread" / "spread-operators"): through
the host emulation of the device code (tests/emu, test infrastructure only), the real C ABI and the real flattener, against the
oracle in claims, instance-type lists, claim requirements, pod assignment and the reference-equivalent evaluation count. The problems
are tests/spread_operator_cases.py's; the device run is tests/test_gpu_spread_operators.py."""
import engine_checks as ec
import limit_cases as lc
import operator_cases as oc
import spread_limit_cases as sl
import spread_node_cases as sn
import spread_operator_cases as so
from karpenter_amd import fixtures as fx
from test_device_algorithm import emu  # noqa: F401  (fixture)


def test_notin_on_the_spread_key(oracle, emu):
    """test-zone-1 appears only on claims of the open pool; the claims of `not-zone-1` are narrowed to test-zone-2 and to test-zone-3."""
    got, want = so.check_engine(oracle, emu, oc.spread_problem(), 3)
    for res in (want, got):
        assert {so.zone_of(c) for c in so.claims_of(res, "not-zone-1")} >= {("In", ("test-zone-2",)), ("In", ("test-zone-3",))}
        assert all("test-zone-1" not in so.zone_of(c)[1] or so.zone_of(c)[0] == "NotIn" for c in so.claims_of(res, "not-zone-1"))
        assert any(so.zone_of(c) == ("In", ("test-zone-1",)) for c in so.claims_of(res, "open"))


def test_counted_but_not_narrowed(oracle, emu):
    """A field with ONE value is not a concrete claim: three claims keep NotIn [test-zone-1, test-zone-2] and count for nothing, the
    six spread pods land 2 / 2 / 2. Written In [test-zone-3] the same pool counts them, and the six land 3 / 3 on zones 1 and 2."""
    prob = so.counted_problem()
    got, want = so.check_engine(oracle, emu, prob, 3)
    for res in (want, got):
        kept = [c for c in so.claims_of(res, "only-3") if so.zone_of(c) == ("NotIn", ("test-zone-1", "test-zone-2"))]
        assert len(kept) == 3 and all(len(c["pods"]) == 1 for c in kept)
        assert so.pods_by_zone(res, so.spread_uids(prob)) == {"test-zone-1": 2, "test-zone-2": 2, "test-zone-3": 2}
        narrowed = sorted((c["nodePool"],) + so.zone_of(c) for c in res["newNodeClaims"] if c not in kept)
        assert narrowed == [("only-3", "In", ("test-zone-3",)), ("open", "In", ("test-zone-1",)), ("open", "In", ("test-zone-2",))]
    concrete = so.counted_problem("In")
    other = oracle.solve(concrete)
    assert not other["podErrors"]
    assert so.pods_by_zone(other, so.spread_uids(concrete)) == {"test-zone-1": 3, "test-zone-2": 3}   # the comparison pins the guard-bit rule only because the two differ
    ec.same(ec.solve(concrete, so.ONLY, emu), other, concrete)


def test_bounds(oracle, emu):
    prob = so.bounds_problem()
    got, want = so.check_engine(oracle, emu, prob, 0)
    integer = oc.integer_of(prob)
    for res in (want, got):
        above = so.claims_of(res, "above")
        assert above and all(integer[t] > 2 for c in above for t in c["instanceTypes"])
        # no pod selects on `integer`: every claim of the pool prints Gt 2 as the reference holds it — Exists with the bound
        for c in above:
            r = so.integer_req(c)
            assert (r["operator"], r["complement"], r["values"], r["gte"], r["lte"]) == ("Exists", True, [], 3, None)


def test_two_dictionary_key_groups(oracle, emu):
    got, want = so.check_engine(oracle, emu, so.two_keys_problem(), 3)
    both = so.claims_of(got, "both")
    assert both and all("test-zone-3" not in so.zone_of(c)[1] or so.zone_of(c)[0] == "NotIn" for c in both)
    assert {so.req_of(c, fx.CAPACITY_TYPE)[0] for c in both} >= {"In"}


def test_zonal_anti_affinity_and_affinity(oracle, emu):
    got, want = so.check_engine(oracle, emu, so.affinity_problem(), 3)
    assert so.claims_of(want, "not-zone-1") and so.claims_of(want, "open")


def test_does_not_exist_on_the_spread_key(oracle, emu):
    """The spread engine solves it: the pool's field is empty and its guard bit clear, no instance type meets it, the template is
    never active and every pod goes to the open pool."""
    got, want = so.check_engine(oracle, emu, so.does_not_exist_problem(), 3)
    assert not so.claims_of(got, "nowhere") and so.claims_of(got, "open")


def test_limit_stages(oracle, emu):
    """The stages are the unmodified problem's, and a stage claim still carries the pool's complement requirements. In the mix and
    the chain every claim's zone is concrete — the mix's pools also carry zone In [three zones], which meets NotIn [test-zone-9] as
    an In set, and every pod of the chain has a zonal spread — so there the complement that survives on a stage claim is integer
    Gt 0; so.limit_notin_problem() is the case whose stage claims print NotIn itself."""
    for prob, bare in ((so.limit_mix_problem(), sl.mix_problem(*sl.MIX[0][:2])), (so.limit_chain_problem(), sl.zonal_chain_problem())):
        got, want = so.check_engine(oracle, emu, prob, 0)
        assert sl.stages(got) == sl.stages(ec.solve(bare, "auto-limits-spread", emu)) and sl.stages(got)[1] is not None   # (a limit bound)
        assert all((fx.FAKE_INTEGER_LABEL, "Exists", 1, None) in so.complement_kinds(c) for c in got["newNodeClaims"])
    chain = so.claims_of(got, "second")
    assert chain and all(so.zone_of(c)[0] == "In" for c in chain)
    prob = so.limit_notin_problem()
    got, want = so.check_engine(oracle, emu, prob, 3)
    assert sl.stages(got)[0] >= 1
    cpus = lc.cpu_of(prob)
    staged = [c for c in so.claims_of(got, "not-zone-1") if lc.max_cpu(c, cpus) < 8]
    assert staged and any(so.zone_of(c) == ("NotIn", ("test-zone-1",)) for c in staged)


def test_existing_nodes(oracle, emu):
    """Engines 9-17 name the existing nodes' reason for such a batch (34)."""
    for prob in (so.nodes_mix_problem(), so.nodes_limit_problem()):
        want = oracle.solve(prob)
        assert not want["podErrors"] and sn.on_nodes(want) > 0
        plain = ec.solve(prob, "auto-nodes-spread", emu)
        assert (plain["counters"]["engine"], plain["counters"]["engineFallbackReason"]) == ("general", 34), plain["counters"]
        got = ec.solve(prob, so.AUTO, emu)
        assert (got["counters"]["engine"], got["counters"]["engineFallbackReason"]) == ("spread", 0), got["counters"]
        ec.same(got, want, prob)
        assert sn.on_nodes(got) == sn.on_nodes(want)


def test_daemonset_overhead(oracle, emu):
    so.check_engine(oracle, emu, so.daemonset_problem(), 3)


def test_still_outside_the_shape(oracle, emu):
    so.check_declined(oracle, emu, so.pod_notin_problem(), 4)
    so.check_declined(oracle, emu, so.pod_gt_problem(), 1)
    so.check_declined(oracle, emu, so.min_values_problem(), 1)
    so.check_declined(oracle, emu, so.node_filter_problem(), 43)


def test_cursor_side_of_auto_operators_spread(emu):
    for prob in (oc.notin_problem(), oc.bounds_problem()):
        cell = so.lone_cell(emu, prob, so.AUTO)
        assert cell[:2] == ("cursor", 0) and cell == so.lone_cell(emu, prob, "auto-operators")


def test_repeated_solves(emu):
    for prob in (oc.spread_problem(), so.limit_mix_problem()):
        digests, words, _ = sl.repeated_solves(emu, prob, so.ONLY, 50)
        assert len(digests) == 1 and len(words) == 1


def test_in_a_batch(emu):
    probs = [oc.spread_problem(), so.counted_problem(), so.bounds_problem()]
    for engine in (so.AUTO, so.ONLY):
        cells = so.batch_cells(emu, probs, engine)
        assert [c[:2] for c in cells] == [("spread", 0)] * 3
        assert cells == [so.lone_cell(emu, p, engine) for p in probs]


def test_old_settings_stay_as_they_are(emu):
    prob = oc.spread_problem()
    for engine in ("auto", "auto-operators"):
        assert so.lone_cell(emu, prob, engine)[:2] == ("general", 3)
    for engine in ("spread", "spread-limits"):
        assert "spread engine declined the problem (reason 3)" in ec.refusal(prob, engine, emu)
    prob = so.bounds_problem()
    for engine in ("auto", "auto-nodes-spread", "auto-limits-spread", "auto-operators"):
        assert so.lone_cell(emu, prob, engine)[:2] == ("general", 0)
    assert "spread engine requested for a problem outside its shape" in ec.refusal(prob, "spread", emu)
    # ... and 17 is still the cursor engine alone, without a name: the new names do not decode to it
    assert "cursor engine requested for a problem outside its shape" in ec.refusal(oc.spread_problem(), 17, emu)


def test_seeded_fuzz(oracle, emu):
    """120 seeds of so.fuzz_problem, a contiguous range: each equals the oracle under "auto-operators-spread"; a seed that leaves the
    spread engine reports reason 27 and nothing else; at least 90 end on the spread engine with reason 0 (measured: 95, the other 25
    with reason 27), and more than half of those have a NodePool with a requirement that is not an In set (measured: see
    profiles/spread_operators/README.md)."""
    on_spread, non_in, rest = so.run_fuzz(oracle, emu, so.FUZZ_SEEDS)
    assert on_spread >= 90, (on_spread, rest)
    assert non_in * 2 > on_spread, (non_in, on_spread)
