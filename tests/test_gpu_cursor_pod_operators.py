"""GPU tests (run with -m gpu on an MI355X) of the cursor engine's pod operators (csrc/fast_engine.h "The cursor engine's pod
operators", ksolve_fast_records; engines "auto-pod-operators" / "cursor-pod-operators"; the kernels of
csrc/ksolve_pack_fast.hip compiled for the PodOps flavour of csrc/pack_flavours.h): the product library through the C ABI against the oracle, on the problems of
tests/pod_operator_cases.py — the ones tests/test_cursor_engine_pod_operators.py runs on the emulation, at the same small shapes."""
import pytest

import engine_checks as ec
import limit_cases as lc
import operator_cases as oc
import pod_operator_cases as pc
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd import fixtures as fx

pytestmark = pytest.mark.gpu


def test_zone_notin_over_an_open_pool(oracle):
    got, want = pc.check_engine(oracle, None, pc.zone_notin_problem())
    assert pc.kinds(want, fx.ZONE) == pc.ZONE_NOTIN_KINDS and pc.kinds(got, fx.ZONE) == pc.ZONE_NOTIN_KINDS


def test_capacity_type_notin_over_an_in_pool(oracle):
    got, want = pc.check_engine(oracle, None, pc.capacity_type_problem())
    assert pc.kinds(want, fx.CAPACITY_TYPE, "both") == {("In", ("on-demand",)), ("In", ("on-demand", "spot"))}
    assert pc.kinds(got, fx.CAPACITY_TYPE, "both") == pc.kinds(want, fx.CAPACITY_TYPE, "both")


def test_complement_meets_complement_with_the_dictionary_exhausted(oracle):
    got, want = pc.check_engine(oracle, None, pc.exhausted_problem())
    assert pc.kinds(want, pc.K, "not-a") == {("NotIn", ("a", "b"))} and pc.kinds(want, pc.K, "open") == {("In", ("a",))}
    assert pc.kinds(got, pc.K, "not-a") == {("NotIn", ("a", "b"))} and pc.kinds(got, pc.K, "open") == {("In", ("a",))}


def test_special_does_not_exist(oracle):
    prob = pc.dne_problem()
    got, want = pc.check_engine(oracle, None, prob, 8)
    integer = oc.integer_of(prob)
    assert pc.claims_of(want, "open") and pc.claims_of(want, "without") and pc.claims_of(want, "with")
    assert pc.kinds(got, fx.FAKE_EXOTIC_LABEL, "open") == {("DoesNotExist", ())}
    assert all(integer[t] <= 4 for c in pc.claims_of(got, "open") for t in c["instanceTypes"])


def test_static_verdicts_on_a_key_no_type_defines(oracle):
    got, want = pc.check_engine(oracle, None, pc.static_verdict_problem(), 4)
    assert not pc.claims_of(want, "exists-first") and pc.claims_of(want, "absent") and pc.claims_of(want, "exists")
    assert pc.kinds(got, pc.K, "absent") == {("DoesNotExist", ())} and pc.kinds(got, pc.K, "exists") == {("Exists", ())}


def test_integer_notin(oracle):
    got, want = pc.check_engine(oracle, None, pc.integer_problem())
    assert {("NotIn", ("7", "8")), ("In", ("4", "6"))} <= pc.kinds(want, fx.FAKE_INTEGER_LABEL)
    assert pc.kinds(got, fx.FAKE_INTEGER_LABEL) == pc.kinds(want, fx.FAKE_INTEGER_LABEL)


def test_exists_on_a_key_the_pools_define(oracle):
    got, want = pc.check_engine(oracle, None, pc.exists_problem())
    assert pc.kinds(want, fx.ZONE, "not-one") == {("NotIn", ("test-zone-1",)), ("In", ("test-zone-3",))}
    assert pc.kinds(got, fx.ZONE, "not-one") == pc.kinds(want, fx.ZONE, "not-one")


def test_limit_stage(oracle):
    prob = pc.limit_problem()
    got, want = pc.check_engine(oracle, None, prob)
    cpus = lc.cpu_of(prob)
    assert lc.stages(got)[0] >= 1
    assert any(pc.req_of(c, fx.ZONE) == ("NotIn", ["test-zone-1", "test-zone-2"]) for c in pc.claims_of(got, "not-zone-1") if lc.max_cpu(c, cpus) < 8)


def test_a_pod_that_excludes_every_zone(oracle):
    got, want = pc.check_unschedulable(oracle, None, pc.no_zone_problem())
    assert len(want["podErrors"]) == 2 and got["podErrors"] == want["podErrors"]


def test_incompatible_pods_keep_the_oracles_error(oracle):
    got, want = pc.check_unschedulable(oracle, None, pc.incompatible_problem())
    assert sorted(e["code"] for e in want["podErrors"].values()) == [2, 2, 2, 2] and got["podErrors"] == want["podErrors"]


def test_still_declined(oracle):
    pc.check_declined(oracle, None, pc.pod_gt_problem(), 1)
    pc.check_declined(oracle, None, pc.nodes_problem(), 4)
    pc.check_declined(oracle, None, pc.definedness_problem(), 9)
    pc.check_declined(oracle, None, pc.dne_mixed_problem(), 10)
    pc.check_declined(oracle, None, pc.notin_bounds_problem(), 11)
    pc.check_declined(oracle, None, pc.exists_undefined_problem(), 12)
    prob = pc.spread_problem()
    auto = ec.solve(prob, pc.AUTO, None)
    assert (auto["counters"]["engine"], auto["counters"]["engineFallbackReason"]) == ("general", 4), auto["counters"]
    ec.same(auto, oracle.solve(prob), prob)
    plain = ec.solve(oc.pod_notin_problem(), pc.BASE, None)["counters"]
    assert (plain["engine"], plain["engineFallbackReason"]) == ("general", 4)


def test_seeded_fuzz(oracle):
    """Ten of the forty seeds of test_cursor_engine_pod_operators.test_seeded_fuzz, under its conditions."""
    on_cursor, rest, turned = pc.run_fuzz(oracle, None, pc.GPU_FUZZ_SEEDS)
    assert on_cursor * 5 >= len(pc.GPU_FUZZ_SEEDS) * 4, (on_cursor, rest)
    assert turned * 2 >= len(pc.GPU_FUZZ_SEEDS), turned
