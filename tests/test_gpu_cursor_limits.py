"""GPU tests (run with -m gpu on an MI355X) of the cursor engine's limit stages (csrc/fast_engine.h FastLimits, engines
"auto-limits" / "cursor-limits"): the product library through the C ABI against the oracle, on the problems of tests/limit_cases.py —
the ones tests/test_cursor_engine_limits.py runs on the emulation, at the same small shapes."""
import pytest

import engine_checks as ec
import limit_cases as lc
import parity
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd import fixtures as fx

pytestmark = pytest.mark.gpu


def test_cpu_chain(oracle):
    lc.check_declined(oracle, None, lc.cpu_chain_problem(False), 27)
    got, want = lc.check_engine(oracle, None, lc.cpu_chain_problem(True))
    assert lc.pool_of(want).count("first") == 5 and lc.pool_of(want).count("second") == 10
    assert lc.stages(got) == (0, 5)


def test_nodes_zero(oracle):
    got, want = lc.check_engine(oracle, None, lc.nodes_zero_problem())
    assert set(lc.pool_of(want)) == {"second"} and lc.stages(got) == (0, None)


def test_two_resources(oracle):
    got, want = lc.check_engine(oracle, None, lc.two_resource_problem())
    assert lc.stages(got)[0] == 2 and set(lc.pool_of(want)) == {"limited", "open"}


def test_daemonsets(oracle):
    got, want = lc.check_engine(oracle, None, lc.daemonset_problem(30))
    assert len(want["newNodeClaims"]) == 5 and not want["podErrors"] and lc.stages(got) == (1, 3)
    got, _ = lc.check_engine(oracle, None, lc.daemonset_overhead_problem())
    assert lc.stages(got)[0] == 1


def test_early_stage_claims_keep_accepting(oracle):
    prob = lc.early_stage_problem()
    got, want = lc.check_engine(oracle, None, prob)
    assert lc.early_claim_took_a_pod_after_a_later_stage(prob, want) and lc.stages(got) == (1, 4)


def test_four_rows_of_class_slots(oracle):
    got, want = lc.check_engine(oracle, None, lc.many_classes_problem())
    assert lc.rows(got) == 4
    assert lc.stages(got)[0] >= 3 and set(lc.pool_of(want)) == {"limited", "catch-all"}


def test_memory_plan_1(oracle):
    got, want = lc.check_engine(oracle, None, lc.escalation_problem(3200))
    assert (got["counters"]["cursorMemoryPlan"], got["counters"]["cursorAttempts"]) == (1, 2)
    assert lc.stages(got)[0] == 1 and lc.pool_of(want).count("first") > 80


def test_memory_plan_2(oracle, monkeypatch):
    """Plan 2 on a small problem needs the -DKSOLVE_TEST_HOOKS build of the device library (it reads KSOLVE_TEST_WIDE_CAP, the
    product does not), as tests/test_gpu_parity.py::test_cursor_engine_moves_its_claim_order_to_hbm_on_the_device."""
    monkeypatch.setenv("KSOLVE_TEST_WIDE_CAP", "1024")
    got, want = lc.check_engine(oracle, parity.build_hooks(), lc.escalation_problem(3200))
    assert (got["counters"]["cursorMemoryPlan"], got["counters"]["cursorAttempts"]) == (2, 2)
    assert lc.stages(got)[0] == 1 and lc.pool_of(want).count("first") > 80


def test_with_existing_nodes(oracle):
    prob = fx.with_existing_nodes(lc.cpu_chain_problem(True), 4, seed=1)
    got, want = lc.check_engine(oracle, None, prob, base="auto-nodes")
    assert sum(len(e["pods"]) for e in want.get("existingNodes", [])) > 0 and lc.stages(got)[1] is not None


def test_stage_exhaustion(oracle):
    got, _ = lc.check_engine(oracle, None, lc.stage_chain_problem(3))
    assert lc.stages(got)[0] == 21
    lc.check_declined(oracle, None, lc.stage_chain_problem(4), 29)


def test_a_hundred_solves_on_one_handle(oracle):
    prob = lc.cpu_chain_problem(True)
    digests, last = ec.digests_of_repeated_solves(None, prob, "auto-limits", 100, "cursor")
    assert len(digests) == 1
    ec.same(last, oracle.solve(prob), prob)
    prob = lc.stage_chain_problem(3)
    digests, last = ec.digests_of_repeated_solves(None, prob, "cursor-limits", 20, "cursor")
    assert len(digests) == 1 and lc.stages(last)[0] == 21
    ec.same(last, oracle.solve(prob), prob)


def test_seeded_fuzz(oracle):
    """Eight of the seeds of test_cursor_engine_limits.test_seeded_fuzz, under its conditions (picked seeds: the shares are a
    property of the selection, see there)."""
    binds, on_cursor, reasons = lc.run_fuzz(oracle, None, lc.GPU_SEEDS)
    assert binds * 2 >= len(lc.GPU_SEEDS), (binds, reasons)
    assert on_cursor * 3 >= binds * 2, (binds, on_cursor, reasons)


def test_seeded_fuzz_with_an_open_pool(oracle):
    lc.run_fuzz(oracle, None, lc.OPEN_SEEDS[:8], open_catch_all=True)
