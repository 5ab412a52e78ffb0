"""scheduling.SolveMany / ksolve_solve_many through the host emulation (CPU; tests/test_gpu_solve_many.py on the device, same shapes):
every member of the call gets the result Solve() gives it on a fresh handle, and members of the spread engine's shape share launches.
The member lists and the checks are tests/solve_many_cases.py."""
import ctypes
import os

import pytest

import solve_many_cases as smc
from test_device_algorithm import emu  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_whole_engine_matrix_as_alone(emu):
    """Every problem of the engine matrix under every setting, the fourteen problems of a setting in ONE SolveMany: all seven fields of
    all 252 cells equal the recorded cell of the LONE solve (tests/golden/engine_matrix.json, taken before this call existed). None is
    skipped and none is excepted: cursorAttempts and cursorMemoryPlan equal the lone cell's too."""
    want = smc.recorded_alone("emulation")
    assert len(want) == 252
    diff = smc.em.differences(smc.matrix_cells(emu), want)
    assert not diff, f"{len(diff)} fields differ (cell, field, got, recorded): {diff[:12]}"


def test_launches_are_shared(oracle, emu):
    smc.check_shared(oracle, emu)


@pytest.fixture(scope="module")
def flavours(emu):
    members = smc.flavour_members()
    return (members,) + smc.passes_on_same_handles(emu, members)


@pytest.fixture(scope="module")
def handbacks(emu):
    members = smc.handback_members()
    return (members,) + smc.passes_on_same_handles(emu, members)


def test_all_six_flavours_in_one_call(oracle, emu, flavours):
    members, want, runs = flavours
    smc.check_flavours(oracle, emu, members, runs[0][0], runs[0][1], want)


def test_hand_backs_and_refusals_inside_the_call(oracle, emu, handbacks):
    members, want, runs = handbacks
    smc.check_handbacks(oracle, emu, members, runs[0][0], runs[0][1], want)


def test_more_members_than_cus(emu):
    stats, _ = smc.check_crowd(emu, smc.crowd_members())
    assert stats["general_members"] == stats["handed_back"], stats   # (every member has topology groups: whatever ran on the general engine was handed back)


def test_the_same_handles_again(flavours, handbacks):
    smc.check_again(flavours[2])
    smc.check_again(handbacks[2])


def test_seeded_fuzz(oracle, emu):
    smc.check_fuzz(oracle, emu, smc.sf.FUZZ_SEEDS, calls=3)


def test_abi(emu):
    """The product library and the emulation export ksolve_solve_many, the ABI version is still 8, the host library exports
    ksched_solve_many and the Go shim calls the C entry point."""
    import __graft_entry__
    __graft_entry__.build()
    product = ctypes.CDLL(os.path.join(ROOT, "karpenter_amd", "libksolve.so"))
    assert hasattr(product, "ksolve_solve_many")
    product.ksolve_abi_version.restype = ctypes.c_uint32
    assert product.ksolve_abi_version() == 8
    emulation = ctypes.CDLL(emu)
    assert hasattr(emulation, "ksolve_solve_many")
    emulation.ksolve_abi_version.restype = ctypes.c_uint32
    assert emulation.ksolve_abi_version() == 8
    assert hasattr(ctypes.CDLL(os.path.join(ROOT, "karpenter_amd", "libksched.so")), "ksched_solve_many")
    with open(os.path.join(ROOT, "go", "ksolve_shim.go")) as f:
        assert "C.ksolve_solve_many(" in f.read()
