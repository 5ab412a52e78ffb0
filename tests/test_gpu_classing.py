"""Pod classing on the MI355X against its definition (tests/classing_cases.py): every classing kernel the launcher can pick —
the six instantiations of ksolve_row_hash_coop2, the same at 60 rows per block, ksolve_row_hash_coop, and ksolve_row_hash both
forced and reached on its own — through the test-only entry point ksolve_test_classify of tests/emu/libksolve_hooks.so (the gfx950
build with -DKSOLVE_TEST_HOOKS). The library reports which kernel it launched and every case asserts on it, so a case that runs
another variant fails instead of passing for the wrong reason. The CPU run of the same lists is tests/test_classing.py."""
import pytest

import classing_cases as cc
import parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hooks():
    from karpenter_amd.scheduling import device_available
    import __graft_entry__
    __graft_entry__.build()
    assert device_available(), "GPU tests need a usable gfx950 device and karpenter_amd/libksolve.so (no CPU fallback)"
    return parity.build_hooks()


def switches(monkeypatch, variant, extra=()):
    for name in cc.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in list(cc.VARIANTS[variant]["env"].items()) + list(extra):
        monkeypatch.setenv(name, value)


def launched(variant, shape, got, what):
    """The kernel the library reports is the variant's."""
    v = cc.VARIANTS[variant]
    want = v["kernel"] if v["kernel"] is not None else cc.coop2_kernel(shape["minv"], shape["separate"], shape["n_res"])
    assert got["kernel"] == want, (what, "launched", cc.KERNEL_NAMES.get(got["kernel"], got["kernel"]), "expected", cc.KERNEL_NAMES[want])
    if want <= cc.K_COOP2_8:
        assert got["rows_per_block"] == (60 if variant == "coop2_rows60" else 64), (what, got["rows_per_block"])


def partition_and_tables(hooks, monkeypatch, variant):
    """Test A (see tests/test_classing.py) on one kernel variant."""
    switches(monkeypatch, variant)
    n = 0
    for shape in cc.shapes(variant):
        case = cc.make_case(shape)
        got = cc.run(hooks, case)
        launched(variant, shape, got, shape)
        cc.check_full(case, got, shape)
        n += 1
    # the kernels without the shared-table form on a SHARED strict table (the launcher's KSOLVE_TEST_NO_SHARED_STRICT)
    if cc.VARIANTS[variant]["separate"] and variant != "plain_lds":
        switches(monkeypatch, variant, [("KSOLVE_TEST_NO_SHARED_STRICT", "1")])
        for shape in cc.shapes(variant)[-3:]:
            case = cc.make_case(dict(shape, separate=False))
            got = cc.run(hooks, case)
            launched(variant, shape, got, shape)
            cc.check_full(case, got, shape)
            n += 1
    print(f"test A, {variant}: {n} launches of {cc.KERNEL_NAMES.get(cc.VARIANTS[variant]['kernel'], 'coop2, 60 rows per block')}")


def single_field_differences(hooks, monkeypatch, variant):
    """Test B (see tests/test_classing.py) on one kernel variant."""
    switches(monkeypatch, variant)
    shape = cc.b_shape(variant)
    n = 0
    for name, counted, rows, at, case in cc.b_cases(shape):
        what = (variant, name, rows, at)
        forced = cc.run(hooks, case, hash_keep=0)
        launched(variant, shape, forced, what)
        cc.check_forced(case, forced, counted, what)
        full = cc.run(hooks, case)
        launched(variant, shape, full, what)
        assert full["n_classes"] == (2 if counted else 1), what
        cc.check_full(case, full, what)
        n += 2
    print(f"test B, {variant}: {n} launches, req_words {shape['rw']}, n_keys {shape['nk']}, n_res {shape['n_res']}")


COOP2 = ["coop2_minv_same", "coop2_minv", "coop2_same_4", "coop2_same_8", "coop2_4", "coop2_8", "coop2_rows60"]
OLDER = ["coop1", "plain_forced", "plain_lds"]


def test_every_variant_has_its_cases():
    assert sorted(COOP2 + OLDER) == sorted(cc.VARIANTS) and len(cc.VARIANTS) == 10


@pytest.mark.parametrize("variant", COOP2)
def test_coop2_partition_and_class_tables(hooks, monkeypatch, variant):
    partition_and_tables(hooks, monkeypatch, variant)


@pytest.mark.parametrize("variant", COOP2)
def test_coop2_single_field_differences(hooks, monkeypatch, variant):
    single_field_differences(hooks, monkeypatch, variant)


@pytest.mark.parametrize("variant", OLDER)
def test_older_kernels_partition_and_class_tables(hooks, monkeypatch, variant):
    partition_and_tables(hooks, monkeypatch, variant)


@pytest.mark.parametrize("variant", OLDER)
def test_older_kernels_single_field_differences(hooks, monkeypatch, variant):
    single_field_differences(hooks, monkeypatch, variant)
