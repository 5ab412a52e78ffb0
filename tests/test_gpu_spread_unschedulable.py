"""GPU tests (run with -m gpu on an MI355X) of the spread engine's set-aside list and its second round (csrc/topo_engine.h, "The spread
engine's unschedulable pods"; kernels ksolve_pack_topo_u / ksolve_pack_topo_nodes_u; engines "auto-unschedulable-spread" /
"spread-unschedulable"): the product library through the C ABI against the oracle, on the problems of
tests/spread_unschedulable_cases.py — the ones tests/test_spread_engine_unschedulable.py runs on the emulation, at the same small
shapes (tens of pods)."""
import pytest

import engine_checks as ec
import limit_cases as lc
import parity
import spread_operator_cases as soc
import spread_unschedulable_cases as suc
from gpu_support import built  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

HAND = suc.hand_problems()
FURTHER = suc.further_problems()
NAMES = [name for name, _, _ in HAND] + [name for name, _ in FURTHER]
PROBLEMS = dict([(name, prob) for name, prob, _ in HAND] + FURTHER)


@pytest.mark.parametrize("name", NAMES)
def test_hand_problem(oracle, name):
    got, want = suc.check_engine(oracle, None, PROBLEMS[name])
    expect = next((e for n, _, e in HAND if n == name), None)
    if expect:
        suc.check_expectation(PROBLEMS[name], want, expect)
    else:
        assert want["podErrors"]


def test_repeated_solves(oracle):
    for name in ("chain-nodes", "chain+limits"):
        digests, last = ec.digests_of_repeated_solves(None, PROBLEMS[name], suc.ONLY, 20, "spread")
        assert len(digests) == 1, name
        want = oracle.solve(PROBLEMS[name])
        ec.same(last, want, mode=ec.SETS)
        assert last["counters"]["pops"] == want["counters"]["pops"]


def test_seeded_fuzz(oracle):
    """Every fourth of the 120 seeds of spread_operator_cases.fuzz_problem under "auto-unschedulable-spread": each equals the oracle,
    pops included, none reports 27."""
    with_errors, on_spread, rest = suc.run_fuzz(oracle, None, soc.fuzz_problem, soc.GPU_FUZZ_SEEDS)
    assert on_spread + len(rest) == len(soc.GPU_FUZZ_SEEDS)


def test_the_device_counts_what_the_emulation_counts(oracle):
    """chain+tail40 — 138 pops, kept verdicts replayed and invalidated by the successes between them — on the device and on the
    host emulation of the same source: every counter both report agrees (pops, evaluations, windows read, limit stages)."""
    prob = PROBLEMS["chain+tail40"]
    dev = ec.solve(prob, suc.ONLY, None)
    emu = ec.solve(prob, suc.ONLY, parity.build_emu())
    assert ec.where(dev) == ec.where(emu) == ("spread", 0)
    assert parity.results_digest(dev)[0] == parity.results_digest(emu)[0]
    skip = {"cursorClaimStateInHBM", "cursorMemoryPlan", "cursorAttempts"}
    keys = [k for k, v in emu["counters"].items() if isinstance(v, (int, str, bool)) and k not in skip and not k.lower().endswith(("ms", "cycles", "seconds"))]
    assert "pops" in keys and "referenceBinEvaluations" in keys and "binEvaluations" in keys
    differ = {k: (dev["counters"].get(k), emu["counters"][k]) for k in keys if dev["counters"].get(k) != emu["counters"][k]}
    assert not differ, differ
    assert lc.stages(dev) == lc.stages(emu)
