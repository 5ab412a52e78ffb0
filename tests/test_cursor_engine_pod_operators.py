"""CPU tests of the cursor engine's pod operators (csrc/fast_engine.h "The cursor engine's pod operators", the records of
ksolve_fast_records; engines "auto-pod-operators" / "cursor-pod-operators"): through the host emulation of the device code (tests/emu,
test infrastructure only), the real C ABI and the real flattener, against the oracle in claims, instance-type lists, claim
requirements (operator and values), pod assignment and the reference-equivalent evaluation count. The problems are
tests/pod_operator_cases.py's; the device run is tests/test_gpu_cursor_pod_operators.py."""
import engine_checks as ec
import limit_cases as lc
import operator_cases as oc
import pod_operator_cases as pc
from karpenter_amd import fixtures as fx
from test_device_algorithm import emu  # noqa: F401  (fixture)


def test_zone_notin_over_an_open_pool(oracle, emu):
    """The three kinds of requirement a claim can end with: the pods' NotIn as it stands, the union of two pods' NotIn sets, and the
    concrete In set a positive pod leaves."""
    got, want = pc.check_engine(oracle, emu, pc.zone_notin_problem())
    assert pc.kinds(want, fx.ZONE) == pc.ZONE_NOTIN_KINDS
    assert pc.kinds(got, fx.ZONE) == pc.ZONE_NOTIN_KINDS


def test_capacity_type_notin_over_an_in_pool(oracle, emu):
    prob = pc.capacity_type_problem()
    got, want = pc.check_engine(oracle, emu, prob)
    picky = {p["uid"] for p in prob["pods"] if pc.pod_reqs(p)}
    with_picky = [c for c in pc.claims_of(want, "both") if picky & set(c["pods"])]
    assert with_picky and all(pc.req_of(c, fx.CAPACITY_TYPE) == ("In", ["on-demand"]) for c in with_picky)
    assert any(pc.req_of(c, fx.CAPACITY_TYPE) == ("In", ["on-demand", "spot"]) for c in pc.claims_of(want, "both"))
    assert pc.kinds(got, fx.CAPACITY_TYPE, "both") == pc.kinds(want, fx.CAPACITY_TYPE, "both")


def test_complement_meets_complement_with_the_dictionary_exhausted(oracle, emu):
    prob = pc.exhausted_problem()
    got, want = pc.check_engine(oracle, emu, prob)
    assert pc.kinds(want, pc.K, "not-a") == {("NotIn", ("a", "b"))}
    pinned = {p["uid"] for p in prob["pods"] if pc.pod_reqs(p)[0]["operator"] == "In"}
    assert pinned and all(pinned >= set(c["pods"]) for c in pc.claims_of(want, "open")) and pc.kinds(want, pc.K, "open") == {("In", ("a",))}
    assert pc.kinds(got, pc.K, "not-a") == {("NotIn", ("a", "b"))} and pc.kinds(got, pc.K, "open") == {("In", ("a",))}


def test_special_does_not_exist(oracle, emu):
    prob = pc.dne_problem()
    got, want = pc.check_engine(oracle, emu, prob, 8)
    integer = oc.integer_of(prob)
    dne = {p["uid"] for p in prob["pods"] if pc.pod_reqs(p)}
    opened, without, with_ = pc.claims_of(want, "open"), pc.claims_of(want, "without"), pc.claims_of(want, "with")
    assert opened and without and with_
    assert not any(dne & set(c["pods"]) for c in with_)                      # the Exists pool refuses them
    assert all(dne >= set(c["pods"]) for c in without)                       # the DoesNotExist pool takes those that tolerate it
    assert pc.kinds(want, fx.FAKE_EXOTIC_LABEL, "open") == {("DoesNotExist", ())} and pc.kinds(got, fx.FAKE_EXOTIC_LABEL, "open") == {("DoesNotExist", ())}
    assert all(integer[t] <= 4 for c in opened for t in c["instanceTypes"]) and all(integer[t] <= 4 for c in pc.claims_of(got, "open") for t in c["instanceTypes"])


def test_static_verdicts_on_a_key_no_type_defines(oracle, emu):
    prob = pc.static_verdict_problem()
    got, want = pc.check_engine(oracle, emu, prob, 4)   # (the Exists class is met first: 4, not the DoesNotExist class's 8)
    ops = {p["uid"]: (pc.pod_reqs(p) or [{"operator": None}])[0]["operator"] for p in prob["pods"]}
    assert not pc.claims_of(want, "exists-first")                                                   # DoesNotExist against the pool's Exists
    assert {ops[u] for c in pc.claims_of(want, "absent") for u in c["pods"]} == {"DoesNotExist", None}   # Exists against the pool's DoesNotExist
    assert {ops[u] for c in pc.claims_of(want, "exists") for u in c["pods"]} == {"Exists"}
    assert pc.kinds(got, pc.K, "absent") == {("DoesNotExist", ())} and pc.kinds(got, pc.K, "exists") == {("Exists", ())}


def test_integer_notin(oracle, emu):
    prob = pc.integer_problem()
    got, want = pc.check_engine(oracle, emu, prob)
    integer = oc.integer_of(prob)
    two = [c for c in want["newNodeClaims"] if pc.req_of(c, fx.FAKE_INTEGER_LABEL) == ("NotIn", ["7", "8"])]
    holders = {i for t, i in integer.items() if lc.cpu_of(prob)[t] - 0.1 >= 5.5}   # (capacity less the types' 100m overhead)
    assert holders == {6, 7, 8} and len(two) == 2 and all({integer[t] for t in c["instanceTypes"]} == holders - {7, 8} for c in two)
    narrowed = [c for c in want["newNodeClaims"] if pc.req_of(c, fx.FAKE_INTEGER_LABEL) == ("In", ["4", "6"])]
    assert len(narrowed) == 1 and len(narrowed[0]["pods"]) == 3 and [integer[t] for t in narrowed[0]["instanceTypes"]] == [6]
    assert pc.kinds(got, fx.FAKE_INTEGER_LABEL) == pc.kinds(want, fx.FAKE_INTEGER_LABEL)


def test_exists_on_a_key_the_pools_define(oracle, emu):
    got, want = pc.check_engine(oracle, emu, pc.exists_problem())
    assert pc.kinds(want, fx.ZONE, "two") == {("In", ("test-zone-1", "test-zone-2"))}
    assert pc.kinds(want, fx.ZONE, "not-one") == {("NotIn", ("test-zone-1",)), ("In", ("test-zone-3",))}
    assert pc.kinds(got, fx.ZONE, "not-one") == pc.kinds(want, fx.ZONE, "not-one")


def test_limit_stage(oracle, emu):
    prob = pc.limit_problem()
    got, want = pc.check_engine(oracle, emu, prob)
    assert lc.stages(got)[0] >= 1
    cpus = lc.cpu_of(prob)
    staged = [c for c in pc.claims_of(got, "not-zone-1") if lc.max_cpu(c, cpus) < 8]
    assert staged and any(pc.req_of(c, fx.ZONE) == ("NotIn", ["test-zone-1", "test-zone-2"]) for c in staged)
    assert "open" in lc.pool_of(want)


def test_a_pod_that_excludes_every_zone(oracle, emu):
    got, want = pc.check_unschedulable(oracle, emu, pc.no_zone_problem())
    assert len(want["podErrors"]) == 2 and got["podErrors"] == want["podErrors"]


def test_incompatible_pods_keep_the_oracles_error(oracle, emu):
    got, want = pc.check_unschedulable(oracle, emu, pc.incompatible_problem())
    assert sorted(e["code"] for e in want["podErrors"].values()) == [2, 2, 2, 2] and got["podErrors"] == want["podErrors"]


def test_still_declined(oracle, emu):
    pc.check_declined(oracle, emu, pc.pod_gt_problem(), 1)
    pc.check_declined(oracle, emu, pc.nodes_problem(), 4)        # the existing-node stage
    pc.check_declined(oracle, emu, pc.definedness_problem(), 9)
    pc.check_declined(oracle, emu, pc.dne_mixed_problem(), 10)
    pc.check_declined(oracle, emu, pc.notin_bounds_problem(), 11)
    pc.check_declined(oracle, emu, pc.exists_undefined_problem(), 12)
    prob = pc.spread_problem()                                   # the spread engine: 4 under every setting
    auto = ec.solve(prob, pc.AUTO, emu)
    assert (auto["counters"]["engine"], auto["counters"]["engineFallbackReason"]) == ("general", 4), auto["counters"]
    ec.same(auto, oracle.solve(prob), prob)
    plain = ec.solve(oc.pod_notin_problem(), pc.BASE, emu)["counters"]
    assert (plain["engine"], plain["engineFallbackReason"]) == ("general", 4)


def test_positive_batches_count_the_same_work(emu):
    """A problem without such pods does the same work under the new names as under "auto"."""
    a = ec.solve(fx.config1(), "auto", emu)["counters"]
    for engine in (pc.AUTO, pc.ENGINE):
        c = ec.solve(fx.config1(), engine, emu)["counters"]
        assert c["engine"] == "cursor"
        assert (c["binEvaluations"], c["slowSorts"], c["referenceBinEvaluations"], c["pops"]) == (a["binEvaluations"], a["slowSorts"], a["referenceBinEvaluations"], a["pops"])


def test_seeded_fuzz(oracle, emu):
    """Forty seeds of pc.fuzz_problem, a contiguous range: each equals the oracle under "auto-pod-operators", the oracle reports no pod
    error for any, at least 32 end on the cursor engine with reason 0, the others name a by-design decline (pc.FUZZ_REASONS), and at
    least half carry a pod requirement that is not an In set (the generator does what it is for: a shape is turned one time in three,
    and many shapes select on nothing)."""
    on_cursor, rest, turned = pc.run_fuzz(oracle, emu, pc.FUZZ_SEEDS)
    assert on_cursor >= 32, (on_cursor, rest)
    assert turned * 2 >= len(pc.FUZZ_SEEDS), turned
