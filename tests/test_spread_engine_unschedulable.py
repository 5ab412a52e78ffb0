"""CPU tests of the spread engine's set-aside list and its second round (csrc/topo_engine.h, "The spread engine's unschedulable pods":
new_claim's error, set_aside, attempt, retry_unschedulable, the verdicts kept per class; engines "auto-unschedulable-spread" /
"spread-unschedulable"): through the host emulation of the device code (tests/emu, test infrastructure only), the real C ABI and the
real flattener, against the oracle in claims and their order, hostnames, pod errors with their flags, queue pops and the
reference-equivalent evaluation count. The problems are tests/spread_unschedulable_cases.py's; the device run is
tests/test_gpu_spread_unschedulable.py."""
import json
import os

import pytest

import engine_checks as ec
import mix_cases
import parity
import spread_limit_cases as slc
import spread_unschedulable_cases as suc
from test_device_algorithm import emu  # noqa: F401  (fixture)
from test_device_fuzz_all import emu_reversed  # noqa: F401  (fixture)

HAND = suc.hand_problems()
FURTHER = suc.further_problems()
NAMES = [name for name, _, _ in HAND] + [name for name, _ in FURTHER]
PROBLEMS = dict([(name, prob) for name, prob, _ in HAND] + FURTHER)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spread_unschedulable_parent.json")


@pytest.fixture(scope="module")
def wanted(oracle):
    """The oracle's result of every problem, computed once."""
    return {name: oracle.solve(prob) for name, prob in PROBLEMS.items()}


def test_the_oracle_reports_what_the_cases_say(wanted):
    """Facts about the reference alone: pops, claims and errors of the issue's table; the further cases leave pod errors; every
    error code the engine can report occurs — Taints 1, Topology 3, InstanceTypes 4 with 21, NoTemplates 6, Limits 7."""
    seen = set()
    for name, prob, expect in HAND:
        suc.check_expectation(prob, wanted[name], expect)
    for name in NAMES:
        seen |= set(suc.errors_of(wanted[name]))
    for name, _ in FURTHER:
        assert wanted[name]["podErrors"], name
    assert {(1, 0), (3, 0), (4, 21), (6, 0), (7, 0)} <= seen, seen
    # the second round places pods: more pops than pods + pods that end unschedulable
    for name in ("chain", "chain+web", "chain-nodes", "chain+tail40"):
        assert wanted[name]["counters"]["pops"] > suc.n_pods(PROBLEMS[name]) + len(wanted[name]["podErrors"]), name


@pytest.mark.parametrize("name", NAMES)
def test_hand_problem(oracle, emu, wanted, name):
    suc.check_engine(oracle, emu, PROBLEMS[name], wanted[name])


@pytest.mark.parametrize("name", NAMES)
def test_hand_problem_lanes_reversed(oracle, emu_reversed, wanted, name):
    suc.check_engine(oracle, emu_reversed, PROBLEMS[name], wanted[name])


def test_error_changes_at_the_retry(oracle, emu, wanted):
    """The 100-cpu pod of `limits` fails with InstanceTypes (4, 21) at its first attempt — what a step limit right behind it shows —
    and with Limits (7) at its second, once the pool has run into its limit: the reported error is that of the LAST attempt."""
    prob = PROBLEMS["limits"]
    big = next(p["uid"] for p in prob["pods"] if p["requests"]["cpu"] == "100")
    early = ec.solve(dict(prob, options=dict(prob.get("options", {}), maxSteps=1)), suc.ONLY, emu)
    assert ec.where(early) == ("spread", 0), early["counters"]
    assert early["timedOut"] and (early["podErrors"][big]["code"], early["podErrors"][big]["diag"]) == (4, 21)
    got = ec.solve(prob, suc.ONLY, emu)
    assert (got["podErrors"][big]["code"], got["podErrors"][big]["diag"]) == (7, 0)
    assert (wanted["limits"]["podErrors"][big]["code"], wanted["limits"]["podErrors"][big]["diag"]) == (7, 0)


def test_step_limit_inside_the_second_round(emu):
    """chain+web has 12 pods and 18 pops: maxSteps = 14 ends the solve inside the second round. The spread engine equals the general
    engine stopped at the same step in claims, assignments and pod errors."""
    prob = PROBLEMS["chain+web"]
    limited = dict(prob, options=dict(prob.get("options", {}), maxSteps=14))
    s = ec.solve(limited, suc.ONLY, emu)
    g = ec.solve(limited, "general", emu)
    assert ec.where(s) == ("spread", 0), s["counters"]
    assert s["timedOut"] and g["timedOut"]
    parity.assert_same_results(s, g)
    assert s["counters"]["pops"] == g["counters"]["pops"] == 14
    assert s["counters"]["referenceBinEvaluations"] == g["counters"]["referenceBinEvaluations"]


def test_repeated_solves(emu, wanted):
    """Twenty solves of one handle: the set-aside list and the kept verdicts start empty every time."""
    for name in ("chain-nodes", "chain+limits"):
        digests, last = ec.digests_of_repeated_solves(emu, PROBLEMS[name], suc.ONLY, 20, "spread")
        assert len(digests) == 1, name
        ec.same(last, wanted[name], mode=ec.SETS)
        assert last["counters"]["pops"] == wanted[name]["counters"]["pops"]


@pytest.mark.parametrize("family", sorted(suc.FAMILIES))
def test_seeded_fuzz(oracle, emu, family):
    """The three fuzz families under "auto-unschedulable-spread": every seed equals the oracle, pops included, and no seed reports
    reason 27 (run_fuzz asserts both). Seeds that leave the spread engine do so with a shape reason and are printed with it."""
    fn, seeds = suc.FAMILIES[family]
    with_errors, on_spread, rest = suc.run_fuzz(oracle, emu, fn, seeds)
    assert with_errors > 0
    if family == "limits":
        assert slc.FUZZ_UNSCHEDULABLE[0] not in rest, rest   # seed 27 ends on the spread engine


def test_the_unschedulable_fuzz_seed_ends_on_the_spread_engine(oracle, emu):
    prob = mix_cases.fuzz_problem(slc.FUZZ_UNSCHEDULABLE[0])
    want = oracle.solve(prob)
    assert len(want["podErrors"]) == 1
    got = ec.solve(prob, suc.AUTO, emu)
    assert ec.where(got) == ("spread", 0), got["counters"]
    ec.same(got, want, mode=ec.SETS)
    assert got["counters"]["pops"] == want["counters"]["pops"]


def test_settings_0_to_21_are_unchanged(emu):
    """spread+big, chain and limits under every name of rows 0-21 of kEngineSettings: the (engine, reason, digest) — or the refusal's
    text — recorded at the parent commit (tests/tools/spread_unschedulable_engines.py --record-parent)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import spread_unschedulable_engines as tool
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(tool.PARENT_CASES)
    for case in tool.PARENT_CASES:
        assert len(golden[case]) == 21, case   # rows 0-21 without the nameless 17
        assert tool.settings_table(emu, PROBLEMS[case], list(golden[case])) == golden[case], case


@pytest.mark.parametrize("name,reason", [(n, r) for n, _, r in suc.declined_problems()])
def test_still_declined(oracle, emu, name, reason):
    prob = next(p for n, p, _ in suc.declined_problems() if n == name)
    suc.check_declined(oracle, emu, prob, reason)


def test_the_cursor_engine_under_22_behaves_as_under_20(oracle, emu):
    """"auto-unschedulable-spread" carries every switch of 20: a batch without topology that leaves pods unschedulable stays on the
    cursor engine, with the digest 20 gives."""
    import unschedulable_cases as uc
    for prob in (uc.tail_run_problem(), uc.error_changes_problem()):
        a, b = ec.solve(prob, suc.BASE, emu), ec.solve(prob, suc.AUTO, emu)
        assert ec.where(a) == ec.where(b) == ("cursor", 0)
        assert parity.results_digest(a)[0] == parity.results_digest(b)[0]
        assert a["counters"]["pops"] == b["counters"]["pops"]
