"""GPU tests (run with -m gpu on an MI355X) of the spread engine's pod operators (csrc/topo_engine.h "The spread engine's pod
operators"; kernels ksolve_pack_topo_p / ksolve_pack_topo_nodes_p; engines "auto-pod-operators-spread" / "spread-pod-operators"): the
product library through the C ABI against the oracle, on the problems of tests/spread_pod_operator_cases.py — the ones
tests/test_spread_engine_pod_operators.py runs on the emulation, at the same small shapes."""
import pytest

import engine_checks as ec
import pod_operator_cases as pc
import spread_filter_cases as sf
import spread_pod_operator_cases as sp
import test_spread_engine_pod_operators as cpu
from gpu_support import built  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
Z1, Z2, Z3 = sp.ZONES


def test_lone_notin_pod_beside_a_spread(oracle):
    sp.check_engine(oracle, None, pc.spread_problem())


def test_spread_pods_carry_the_notin(oracle):
    cpu.test_spread_pods_carry_the_notin(oracle, None)


def test_counted_but_not_concrete(oracle):
    assert cpu.pair(oracle, None, sp.counted_problem(), sp.counted_problem("In")) == ({Z1: 2, Z2: 2, Z3: 2}, {Z1: 3, Z2: 3})


def test_notin_term_on_an_undefined_key(oracle):
    assert cpu.pair(oracle, None, sp.undefined_term_problem(), sp.undefined_term_problem("In")) == (sf.COUNTED, sf.NOT_COUNTED)


def test_notin_pod_defines_the_key(oracle):
    cpu.test_notin_pod_defines_the_key(oracle, None)


def test_two_dictionary_key_groups(oracle):
    cpu.test_two_dictionary_key_groups(oracle, None)


def test_affinity_and_anti_affinity(oracle):
    sp.check_engine(oracle, None, sp.affinity_problem())


def test_does_not_exist_beside_a_spread(oracle):
    cpu.test_does_not_exist_beside_a_spread(oracle, None)


def test_does_not_exist_term(oracle):
    cpu.test_does_not_exist_term(oracle, None)


def test_zone_exists_over_pools_that_define_the_zone(oracle):
    sp.check_engine(oracle, None, sp.exists_problem())


def test_unschedulable_pods(oracle):
    cpu.test_unschedulable_pods(oracle, None)


def test_limit_stage(oracle):
    cpu.test_limit_stage(oracle, None)


def test_daemonset_overhead(oracle):
    sp.check_engine(oracle, None, sp.daemonset_problem())


def test_still_declined(oracle):
    cpu.test_still_declined(oracle, None)


def test_old_settings_stay_as_they_are():
    cpu.test_old_settings_stay_as_they_are(None)


def test_positive_batches_are_unchanged():
    cpu.test_positive_batches_are_unchanged(None)


def test_repeated_solves():
    cpu.test_repeated_solves(None)


def test_members_of_one_solve_many(oracle):
    cpu.test_members_of_one_solve_many(oracle, None)


def test_seeded_fuzz(oracle):
    """Every fourth of the 120 seeds of test_spread_engine_pod_operators.test_seeded_fuzz, under its conditions."""
    on_spread, rest, errors = sp.run_fuzz(oracle, None, sp.GPU_FUZZ_SEEDS)
    assert on_spread * 5 >= len(sp.GPU_FUZZ_SEEDS) * 4, (on_spread, rest)
    assert errors >= 1, errors
