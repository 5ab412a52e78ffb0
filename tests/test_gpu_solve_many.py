"""scheduling.SolveMany / ksolve_solve_many on the device (tests/test_solve_many.py on the host emulation, same shapes): every member
of the call gets the result Solve() gives it on a fresh handle, and members of the spread engine's shape share launches of the
ksolve_pack_topo*_many kernels. The member lists and the checks are tests/solve_many_cases.py."""
import time

import pytest

import solve_many_cases as smc
from gpu_support import built  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def test_the_whole_engine_matrix_as_alone():
    """Every problem of the engine matrix under every setting, the fourteen problems of a setting in ONE SolveMany: all seven fields of
    all 252 cells equal the device's recorded cell of the LONE solve (tests/golden/engine_matrix.json, taken before this call
    existed). None is skipped and none is excepted."""
    want = smc.recorded_alone("device")
    assert len(want) == 252
    diff = smc.em.differences(smc.matrix_cells(None), want)
    assert not diff, f"{len(diff)} fields differ (cell, field, got, recorded): {diff[:12]}"


def test_launches_are_shared(oracle):
    smc.check_shared(oracle, None)


@pytest.fixture(scope="module")
def flavours():
    members = smc.flavour_members()
    return (members,) + smc.passes_on_same_handles(None, members)


@pytest.fixture(scope="module")
def handbacks():
    members = smc.handback_members()
    return (members,) + smc.passes_on_same_handles(None, members)


def test_all_six_flavours_in_one_call(oracle, flavours):
    members, want, runs = flavours
    smc.check_flavours(oracle, None, members, runs[0][0], runs[0][1], want)


def test_hand_backs_and_refusals_inside_the_call(oracle, handbacks):
    members, want, runs = handbacks
    smc.check_handbacks(oracle, None, members, runs[0][0], runs[0][1], want)


def test_more_members_than_cus():
    """264 members on 256 CUs: one launch whose last blocks wait for a CU, so the ticket decides who runs first. 24 pods each while
    handle creation plus the SolveMany call (with Results) stay under five seconds — timed here, without the 264 lone solves, and
    printed (profiles/solve_many/gpu_new_tests.log keeps the figure); were it more, the pod count would be halved, not the member
    count. The clock is not asserted: a test that fails on a busy host checks nothing about the solver."""
    members = smc.crowd_members()
    t = time.perf_counter()
    stats, seconds = smc.check_crowd(None, members)
    print(f"264 members: handle creation + SolveMany {seconds:.2f} s; with the 264 lone solves {time.perf_counter() - t:.2f} s; {stats}")


def test_the_same_handles_again(flavours, handbacks):
    smc.check_again(flavours[2])
    smc.check_again(handbacks[2])


def test_seeded_fuzz(oracle):
    smc.check_fuzz(oracle, None, smc.sf.GPU_FUZZ_SEEDS, calls=1)
