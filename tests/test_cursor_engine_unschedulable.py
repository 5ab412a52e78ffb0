"""CPU tests of the cursor engine's set-aside list (csrc/fast_engine.h, "Unschedulable pods": FastCold::new_claim's error, set_aside,
retry_unschedulable; engines "auto-unschedulable" / "cursor-unschedulable"): through the host emulation of the device code
(tests/emu, test infrastructure only), the real C ABI and the real flattener, against the oracle in claims and their order,
hostnames, pod errors with their flags, queue pops and the reference-equivalent evaluation count. The problems are
tests/unschedulable_cases.py's; the device run is tests/test_gpu_cursor_unschedulable.py."""
import pytest

import engine_checks as ec
import limit_cases as lc
import parity
import unschedulable_cases as uc
from karpenter_amd import fixtures as fx
from test_device_algorithm import emu  # noqa: F401  (fixture)
from test_device_fuzz_all import emu_reversed  # noqa: F401  (fixture)

HAND = uc.hand_problems()


@pytest.fixture(scope="module")
def wanted(oracle):
    """The oracle's result of every hand problem, computed once."""
    return {name: oracle.solve(prob) for name, prob, _ in HAND}


def test_the_oracle_reports_what_the_cases_say(wanted):
    """Facts about the reference alone: the errors, claims and pops each case was written for, and every error code the cursor
    engine can report — Taints 1, Incompatible 2, InstanceTypes 4 without a flag and with 21, NoTemplates 6, Limits 7."""
    seen = set()
    for name, prob, expect in HAND:
        uc.check_expectation(prob, wanted[name], expect)
        seen |= set(uc.errors_of(wanted[name]))
    assert {(1, 0), (2, 0), (4, 0), (4, 21), (6, 0), (7, 0)} <= seen, seen


@pytest.mark.parametrize("name", [name for name, _, _ in HAND])
def test_hand_problem(oracle, emu, name):
    prob = next(p for n, p, _ in HAND if n == name)
    got, want = uc.check_engine(oracle, emu, prob)
    if name == "escalation":
        assert got["counters"]["cursorMemoryPlan"] >= 1, got["counters"]   # plan 1: the claims' state in HBM
    if name == "many-classes":
        assert lc.rows(got) == 4


@pytest.mark.parametrize("name", [name for name, _, _ in HAND if name != "escalation"])
def test_hand_problem_lanes_reversed(oracle, emu_reversed, name):
    prob = next(p for n, p, _ in HAND if n == name)
    uc.check_engine(oracle, emu_reversed, prob)


def test_error_changes_at_the_retry(oracle, emu):
    """The 100-cpu pod fails with InstanceTypes (4, 21) at its first attempt — what a step limit right behind it shows — and with
    Limits (7) at its second, once the pool has run into its limit: the reported error is that of the LAST attempt."""
    prob = uc.error_changes_problem()
    big = next(p["uid"] for p in prob["pods"] if p["requests"]["cpu"] == "100")
    early = ec.solve(dict(prob, options=dict(prob.get("options", {}), maxSteps=1)), "cursor-unschedulable", emu)
    assert early["timedOut"] and (early["podErrors"][big]["code"], early["podErrors"][big]["diag"]) == (4, 21)
    got, want = uc.check_engine(oracle, emu, prob)
    assert (got["podErrors"][big]["code"], got["podErrors"][big]["diag"]) == (7, 0)


def test_plain_batches_count_the_same_work(emu):
    """A batch without such pods does the same work under the new names as under "auto"."""
    a = ec.solve(fx.config1(), "auto", emu)["counters"]
    for engine in ("auto-unschedulable", "cursor-unschedulable"):
        c = ec.solve(fx.config1(), engine, emu)["counters"]
        assert c["engine"] == "cursor"
        assert (c["binEvaluations"], c["slowSorts"], c["referenceBinEvaluations"], c["pops"]) == (a["binEvaluations"], a["slowSorts"], a["referenceBinEvaluations"], a["pops"])


def test_repeated_solves(oracle, emu):
    """Twenty solves of one handle: the set-aside list starts empty every time (setup())."""
    for prob in (uc.tail_run_problem(), fx.with_existing_nodes(uc.tail_run_problem(), 4, seed=1), uc.error_changes_problem()):
        digests, last = ec.digests_of_repeated_solves(emu, prob, "cursor-unschedulable", 20, "cursor")
        assert len(digests) == 1
        want = oracle.solve(prob)
        ec.same(last, want, mode=ec.SETS)
        assert last["counters"]["pops"] == want["counters"]["pops"]


@pytest.mark.parametrize("nodes", [False, True], ids=["plain", "nodes"])
def test_step_limit(emu, nodes):
    """maxSteps from two before the queue's end to one past the last pop of the second round: the cursor engine equals the general
    engine stopped at the same step — status, pops, Results (the errors recorded so far included)."""
    prob = uc.tail_run_problem()
    if nodes:
        prob = fx.with_existing_nodes(prob, 4, seed=1)
    pods, pops = uc.n_pods(prob), uc.n_pods(prob) + 1
    for steps in range(pods - 2, pops + 2):
        limited = dict(prob, options=dict(prob.get("options", {}), maxSteps=steps))
        c = ec.solve(limited, "cursor-unschedulable", emu)
        g = ec.solve(limited, "general", emu)
        assert c["counters"]["engine"] == "cursor" and c["counters"]["engineFallbackReason"] == 0, (steps, c["counters"])
        assert c["timedOut"] == g["timedOut"] == (steps < pops), (steps, c["timedOut"], g["timedOut"])
        parity.assert_same_results(c, g)
        assert c["counters"]["pops"] == g["counters"]["pops"] == min(steps, pops), (steps, c["counters"]["pops"], g["counters"]["pops"])
        assert c["counters"]["referenceBinEvaluations"] == g["counters"]["referenceBinEvaluations"], steps


def test_still_declined(oracle, emu):
    """The spread engine declines a batch with such a pod as before (27: there a retry can succeed). A failing pod with a preference
    makes a relaxation row, and such a batch is not offered to a fast engine at all (reason 0, "outside its shape"). A pod with a
    NotIn, Gt or Lt requirement of its own keeps its reason (4, 1, 1), and so does a NodePool with minValues (1)."""
    prob = uc.spread_problem()
    auto = ec.solve(prob, "auto-unschedulable", emu)
    assert (auto["counters"]["engine"], auto["counters"]["engineFallbackReason"]) == ("general", 27), auto["counters"]
    ec.same(auto, oracle.solve(prob), prob)
    uc.check_declined(oracle, emu, uc.preference_problem(), 0)
    for _, prob, reason in uc.pod_operator_problems():
        uc.check_declined(oracle, emu, prob, reason)


def test_seeded_fuzz(oracle, emu):
    """lc.fuzz_problem for the seeds 0-47 under "auto-unschedulable": each equals the oracle (pops included); the oracle reports pod
    errors in 47 of them; at least 40 end on the cursor engine with reason 0, and none leaves it with 27. Measured: all 48 stay on
    the cursor engine."""
    with_errors, on_cursor, rest = uc.run_fuzz(oracle, emu, uc.FUZZ_SEEDS)
    assert with_errors == 47, with_errors
    assert on_cursor >= 40, (on_cursor, rest)
