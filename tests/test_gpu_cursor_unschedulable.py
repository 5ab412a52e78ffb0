"""GPU tests (run with -m gpu on an MI355X) of the cursor engine's set-aside list (csrc/fast_engine.h, "Unschedulable pods"; engines
"auto-unschedulable" / "cursor-unschedulable"): the product library through the C ABI against the oracle, on the problems of
tests/unschedulable_cases.py — the ones tests/test_cursor_engine_unschedulable.py runs on the emulation, at the same small shapes
(the 3,600-claim plan escalation stays on the emulation)."""
import pytest

import engine_checks as ec
import limit_cases as lc
import unschedulable_cases as uc
from gpu_support import built  # noqa: F401  (fixture)
from karpenter_amd import fixtures as fx

pytestmark = pytest.mark.gpu

HAND = uc.hand_problems(with_escalation=False)


@pytest.mark.parametrize("name", [name for name, _, _ in HAND])
def test_hand_problem(oracle, name):
    prob, expect = next((p, e) for n, p, e in HAND if n == name)
    got, want = uc.check_engine(oracle, None, prob)
    uc.check_expectation(prob, want, expect)
    if name == "many-classes":
        assert lc.rows(got) == 4


def test_repeated_solves(oracle):
    prob = fx.with_existing_nodes(uc.tail_run_problem(), 4, seed=1)
    digests, last = ec.digests_of_repeated_solves(None, prob, "cursor-unschedulable", 20, "cursor")
    assert len(digests) == 1
    ec.same(last, oracle.solve(prob), prob)


def test_seeded_fuzz(oracle):
    """Every fourth of the 48 seeds of test_cursor_engine_unschedulable.test_seeded_fuzz, under its conditions."""
    with_errors, on_cursor, rest = uc.run_fuzz(oracle, None, uc.GPU_FUZZ_SEEDS)
    assert with_errors >= len(uc.GPU_FUZZ_SEEDS) - 1
    assert on_cursor * 6 >= len(uc.GPU_FUZZ_SEEDS) * 5, (on_cursor, rest)
