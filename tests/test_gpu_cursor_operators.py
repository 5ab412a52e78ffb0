"""GPU tests (run with -m gpu on an MI355X) of the cursor engine's complement templates (csrc/fast_engine.h FastCold::setup
"Complement templates", ksolve_fast_records; engines "auto-operators" / "cursor-operators"): the product library through the C ABI
against the oracle, on the problems of tests/operator_cases.py — the ones tests/test_cursor_engine_operators.py runs on the
emulation, at the same small shapes."""
import pytest

import limit_cases as lc
import operator_cases as oc
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd import fixtures as fx

pytestmark = pytest.mark.gpu


def test_bounds_on_a_key_no_pod_selects_on(oracle):
    prob = oc.bounds_problem()
    got, want = oc.check_engine(oracle, None, prob, 1)
    integer = oc.integer_of(prob)
    assert oc.claims_of(want, "above") and oc.claims_of(want, "below")
    assert all(integer[t] > 2 for c in oc.claims_of(got, "above") for t in c["instanceTypes"])


def test_notin_on_a_key_pods_select_on(oracle):
    got, want = oc.check_engine(oracle, None, oc.notin_problem(), 3)
    assert oc.zone_kinds(want) == oc.NOTIN_KINDS and oc.zone_kinds(got) == oc.NOTIN_KINDS


def test_does_not_exist_and_exists(oracle):
    got, want = oc.check_engine(oracle, None, oc.exists_problem(), 3)
    assert oc.claims_of(want, "without") and oc.claims_of(want, "with")
    assert {oc.req_of(c, fx.FAKE_EXOTIC_LABEL)[0] for c in oc.claims_of(got, "with")} == {"Exists", "In"}


def test_escape_rule(oracle):
    got, want = oc.check_engine(oracle, None, oc.escape_problem(), 1)
    lists = {p: sorted(oc.claims_of(got, p)[0]["instanceTypes"]) for p in ("not-y", "exists", "positive")}
    assert lists == {"not-y": ["k-absent", "k-not-x"], "exists": ["k-is-y", "k-not-x"], "positive": ["k-not-x"]}


def test_gt_on_a_key_pods_select_on(oracle):
    got, want = oc.check_engine(oracle, None, oc.kwok_problem(), 1)
    assert oc.claims_of(want, "big") and oc.claims_of(want, "open")


def test_limit_stage(oracle):
    prob = oc.limit_problem()
    got, want = oc.check_engine(oracle, None, prob, 3)
    cpus = lc.cpu_of(prob)
    assert lc.stages(got)[0] >= 1
    assert any(oc.req_of(c, fx.ZONE) == ("NotIn", ["test-zone-1"]) for c in oc.claims_of(got, "not-zone-1") if lc.max_cpu(c, cpus) < 8)


def test_existing_nodes_and_a_daemonset(oracle):
    got, want = oc.check_engine(oracle, None, oc.nodes_problem(), 34, base="auto-nodes", base_cursor="cursor-nodes")
    assert sum(len(e["pods"]) for e in want.get("existingNodes", [])) > 0 and oc.claims_of(want, "above")


def test_seeded_fuzz(oracle):
    """Ten of the forty seeds of test_cursor_engine_operators.test_seeded_fuzz, under its conditions."""
    on_cursor, rest = oc.run_fuzz(oracle, None, oc.GPU_FUZZ_SEEDS)
    assert on_cursor * 5 >= len(oc.GPU_FUZZ_SEEDS) * 4, (on_cursor, rest)
