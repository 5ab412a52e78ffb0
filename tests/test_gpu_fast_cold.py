"""GPU tests of the cold half of the cursor engine (fast_engine.h FastCold) on the device: the test-only entry point
ksolve_test_fast_cold of tests/emu/libksolve_hooks.so (the gfx950 build with -DKSOLVE_TEST_HOOKS) — one wavefront over the product's
LDS plan, setup() and a script of operations, in every instantiation of FastCold the product's kernels use — on the cases of
tests/fast_cold_cases.py. Every device answer equals the definition and, bit for bit in the same fields, the answer of the host
emulation; every case asserts which instantiation ran. The CPU run of the same cases, which also holds the cases to what they must
contain, is tests/test_fast_cold.py."""
import os
import time

import pytest

import fast_cold_cases as fc
import parity
from gpu_support import built  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
_T0 = time.time()


@pytest.fixture(scope="module")
def hooks():
    return parity.build_hooks()


@pytest.fixture(scope="module")
def emu():
    return parity.build_emu()


@pytest.mark.parametrize("name", list(fc.CASES))
def test_against_definition_and_emulation(hooks, emu, name):
    P, script = fc.load(name)
    want = fc.expected(P, script)
    host = fc.run(emu, P, script, want)
    assert fc.mismatches(host, want, P, script) == [], (name, "the emulation")       # only cases that are green on the emulation go to the device
    got = fc.run(hooks, P, script, want)
    assert got["status"] == 0 and got["kernel"] == fc.kernel_id(P, emulation=False), (name, got["status"], got["kernel"])
    assert fc.mismatches(got, want, P, script) == [], (name, "definition")
    assert fc.device_differs(got, host, P) == [], (name, "emulation")


@pytest.mark.parametrize("name", list(fc.DECLINES))
def test_decline(hooks, emu, name):
    P, reason = fc.DECLINES[name]()
    script = [("CELLS", 0, ())]
    want = fc.expected(P, script)
    assert want["setup_ret"] == reason, name
    got = fc.run(hooks, P, script, want)
    assert got["kernel"] == fc.kernel_id(P, emulation=False) and fc.mismatches(got, want, P, script) == [], name
    if reason == 0:
        assert fc.device_differs(got, fc.run(emu, P, script, want), P) == [], name


@pytest.mark.parametrize("name", list(fc.REFUSED))
def test_hook_refuses_what_is_out_of_range(hooks, name):
    P, script, edit = fc.REFUSED[name]()
    got = fc.run(hooks, P, script, edit=edit)
    assert got["status"] == fc.KSOLVE_ERR_INVALID and bytes(got["scal"]) == b"\xA5" * len(bytes(got["scal"])), name


def test_zz_file_time():
    """how long this file took (read with -s; profiles/fast_cold_tests/ keeps the figure of the recorded run)"""
    took = time.time() - _T0
    print(f"tests/test_gpu_fast_cold.py: {took:.1f} s")
    out = os.environ.get("KSOLVE_FAST_COLD_TIME_FILE")
    if out:
        with open(out, "w") as f:
            f.write(f"tests/test_gpu_fast_cold.py: {took:.1f} s from import to the last test\n")
