"""CPU tests of the cursor engine's complement templates (csrc/fast_engine.h FastCold::setup "Complement templates", the records of
ksolve_fast_records; engines "auto-operators" / "cursor-operators"): through the host emulation of the device code (tests/emu, test
infrastructure only), the real C ABI and the real flattener, against the oracle in claims, instance-type lists, claim requirements
(operator and values), pod assignment and the reference-equivalent evaluation count. The problems are tests/operator_cases.py's; the
device run is tests/test_gpu_cursor_operators.py."""
import engine_checks as ec
import limit_cases as lc
import operator_cases as oc
from karpenter_amd import fixtures as fx
from test_device_algorithm import emu  # noqa: F401  (fixture)


def test_bounds_on_a_key_no_pod_selects_on(oracle, emu):
    prob = oc.bounds_problem()
    got, want = oc.check_engine(oracle, emu, prob, 1)
    integer = oc.integer_of(prob)
    assert oc.claims_of(want, "above") and oc.claims_of(want, "below") and oc.claims_of(want, "open")
    assert all(integer[t] > 2 for c in oc.claims_of(want, "above") for t in c["instanceTypes"])
    assert all(integer[t] < 3 for c in oc.claims_of(want, "below") for t in c["instanceTypes"])
    # the claim carries the pool's requirement as it stands: Exists with a bound
    r = next(r for r in oc.claims_of(got, "above")[0]["requirements"] if r["key"] == fx.FAKE_INTEGER_LABEL)
    assert (r["operator"], r["complement"], r["values"], r["gte"], r["lte"]) == ("Exists", True, [], 3, None)


def test_notin_on_a_key_pods_select_on(oracle, emu):
    """The two states of the guard bit: a claim that holds only unselecting pods still prints the pool's NotIn [test-zone-1]; one that
    took a pod admitting all three zones holds the same two values as a concrete In set; a test-zone-2 pod narrows it further."""
    got, want = oc.check_engine(oracle, emu, oc.notin_problem(), 3)
    assert oc.zone_kinds(want) == oc.NOTIN_KINDS
    assert oc.zone_kinds(got) == oc.NOTIN_KINDS
    assert all(oc.req_of(c, fx.ZONE) == ("In", ["test-zone-1"]) for c in oc.claims_of(want, "open")) and oc.claims_of(want, "open")


def test_does_not_exist_and_exists(oracle, emu):
    prob = oc.exists_problem()
    got, want = oc.check_engine(oracle, emu, prob, 3)
    integer = oc.integer_of(prob)
    without, with_ = oc.claims_of(want, "without"), oc.claims_of(want, "with")
    assert without and with_
    assert all(integer[t] <= 4 for c in without for t in c["instanceTypes"]) and all(integer[t] > 4 for c in with_ for t in c["instanceTypes"])
    selecting = {p["uid"] for p in prob["pods"] if p.get("nodeSelector")}
    assert not any(selecting & set(c["pods"]) for c in without)
    assert {oc.req_of(c, fx.FAKE_EXOTIC_LABEL)[0] for c in with_} == {"Exists", "In"}
    assert {oc.req_of(c, fx.FAKE_EXOTIC_LABEL)[0] for c in without} == {"DoesNotExist"}


def test_escape_rule(oracle, emu):
    got, want = oc.check_engine(oracle, emu, oc.escape_problem(), 1)
    lists = {p: sorted(oc.claims_of(want, p)[0]["instanceTypes"]) for p in ("not-y", "exists", "positive")}
    assert lists == {"not-y": ["k-absent", "k-not-x"], "exists": ["k-is-y", "k-not-x"], "positive": ["k-not-x"]}
    assert {p: sorted(oc.claims_of(got, p)[0]["instanceTypes"]) for p in lists} == lists


def test_escape_rule_without_bounds(oracle, emu):
    """The same three types under the NotIn and Exists pools alone: engines 0-14 decline in setup() (3), not on the host (1)."""
    prob = oc.escape_problem()
    prob["nodePools"] = [p for p in prob["nodePools"] if p["name"] != "positive"]
    oc.check_engine(oracle, emu, prob, 3)


def test_gt_on_a_key_pods_select_on(oracle, emu):
    prob = oc.kwok_problem()
    got, want = oc.check_engine(oracle, emu, prob, 1)
    only_two = {p["uid"] for p in prob["pods"] if p.get("nodeSelector")}
    assert only_two and all(only_two & set(c["pods"]) for c in oc.claims_of(want, "open")) and not any(only_two & set(c["pods"]) for c in oc.claims_of(want, "big"))
    assert all(not t.startswith("c-") for c in oc.claims_of(want, "big") for t in c["instanceTypes"])
    kinds = {oc.req_of(c, fx.KWOK_CPU) and (oc.req_of(c, fx.KWOK_CPU)[0], tuple(oc.req_of(c, fx.KWOK_CPU)[1])) for c in oc.claims_of(want, "big")}
    assert ("In", ("4", "8")) in kinds      # In [2, 4, 8] met Gt 3: concrete, the bound dropped


def test_limit_stage(oracle, emu):
    prob = oc.limit_problem()
    got, want = oc.check_engine(oracle, emu, prob, 3)
    assert lc.stages(got)[0] >= 1
    cpus = lc.cpu_of(prob)
    staged = [c for c in oc.claims_of(got, "not-zone-1") if lc.max_cpu(c, cpus) < 8]
    assert staged and any(oc.req_of(c, fx.ZONE) == ("NotIn", ["test-zone-1"]) for c in staged)
    assert "open" in lc.pool_of(want)


def test_existing_nodes_and_a_daemonset(oracle, emu):
    """Engines 7-14 name the existing nodes' reason for a batch with bounds (34); "auto" does not try a batch with nodes at all."""
    prob = oc.nodes_problem()
    got, want = oc.check_engine(oracle, emu, prob, 34, base="auto-nodes", base_cursor="cursor-nodes")
    assert sum(len(e["pods"]) for e in want.get("existingNodes", [])) > 0 and oc.claims_of(want, "above")
    plain = ec.solve(prob, "auto", emu)["counters"]
    assert (plain["engine"], plain["engineFallbackReason"]) == ("general", 0)


def test_still_declined(oracle, emu):
    oc.check_declined(oracle, emu, oc.pod_notin_problem(), 4)
    oc.check_declined(oracle, emu, oc.min_values_problem(), 1)
    oc.check_declined(oracle, emu, oc.pod_gt_problem(), 1)
    prob = oc.spread_problem()
    auto = ec.solve(prob, "auto-operators", emu)
    assert auto["counters"]["engine"] == "general", auto["counters"]
    ec.same(auto, oracle.solve(prob), prob)


def test_in_only_pools_count_the_same_work(emu):
    """A problem without such pools does the same work under the new names as under "auto"."""
    a = ec.solve(fx.config1(), "auto", emu)["counters"]
    for engine in ("auto-operators", "cursor-operators"):
        c = ec.solve(fx.config1(), engine, emu)["counters"]
        assert c["engine"] == "cursor"
        assert (c["binEvaluations"], c["slowSorts"], c["referenceBinEvaluations"], c["pops"]) == (a["binEvaluations"], a["slowSorts"], a["referenceBinEvaluations"], a["pops"])


def test_seeded_fuzz(oracle, emu):
    """Forty seeds of oc.fuzz_problem, a contiguous range: each equals the oracle under "auto-operators", the oracle reports no pod
    error for any, and at least 32 end on the cursor engine with reason 0. Measured: all 40 do; no seed leaves the cursor engine."""
    on_cursor, rest = oc.run_fuzz(oracle, emu, oc.FUZZ_SEEDS)
    assert on_cursor >= 32, (on_cursor, rest)
