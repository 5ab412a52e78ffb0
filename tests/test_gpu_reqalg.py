"""The requirement algebra (csrc/reqalg.h) and the instance-type index (ksolve_it_index) on the MI355X against their definition
(tests/reqalg_cases.py): the lists of tests/test_reqalg.py through the test-only entry points ksolve_test_reqalg and
ksolve_test_it_index of tests/emu/libksolve_hooks.so (the gfx950 build with -DKSOLVE_TEST_HOOKS) — one launch per table and per
shape for the algebra, one per index case. Every comparison is exact. Each case also runs on the host emulation, and the two
answers must agree bit for bit in every field, the ones the definition leaves open included (none is excluded: see
reqalg_cases.py)."""
import pytest

import parity
import reqalg_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hooks():
    from karpenter_amd.scheduling import device_available
    import __graft_entry__
    __graft_entry__.build()
    assert device_available(), "GPU tests need a usable gfx950 device and karpenter_amd/libksolve.so (no CPU fallback)"
    return parity.build_hooks()


@pytest.fixture(scope="module")
def emu():
    return parity.build_emu()


def test_reference_tables(hooks, emu):
    golden = rc.golden_tables()
    dev, host = rc.run_tables(hooks, golden), rc.run_tables(emu, golden)
    assert len(dev) == len(host) == 6
    for i, (d, h) in enumerate(zip(dev, host)):
        assert rc.same_outputs(d, h, rc.REQALG_FIELDS) == [], ("device and emulation differ", i)


@pytest.mark.parametrize("name", list(rc.SHAPES))
def test_generated_pairs(hooks, emu, name):
    dev = rc.run_shape(hooks, name)
    assert rc.same_outputs(dev, rc.run_shape(emu, name), rc.REQALG_FIELDS) == [], "device and emulation differ"


@pytest.mark.parametrize("n_its,n_res", rc.INDEX_SIZES)
def test_it_index(hooks, emu, n_its, n_res):
    dev, _ = rc.run_index(hooks, n_its, n_res, "ordinary")
    assert rc.same_outputs(dev, rc.run_index(emu, n_its, n_res, "ordinary")[0], rc.INDEX_FIELDS + ("error", "it_words")) == []


@pytest.mark.parametrize("n_its", rc.CONTENTION_SIZES)
def test_it_index_contention(hooks, emu, n_its):
    """All types In the same value and undefined on the same key: the 64 threads of a word OR into the same two words, which only
    atomics keep whole (the emulation's serial loop cannot lose such a bit; the device can)."""
    dev, _ = rc.run_index(hooks, n_its, 2, "contention")
    assert rc.same_outputs(dev, rc.run_index(emu, n_its, 2, "contention")[0], rc.INDEX_FIELDS + ("error", "it_words")) == []


@pytest.mark.parametrize("kind", ["wrong-name", "bound"])
def test_it_index_errors(hooks, emu, kind):
    dev, _ = rc.run_index(hooks, 65, 2, kind)
    # (the tables of a problem the error word refuses for a bound are compared between the two builds only)
    assert rc.same_outputs(dev, rc.run_index(emu, 65, 2, kind)[0], rc.INDEX_FIELDS + ("error", "it_words")) == []
