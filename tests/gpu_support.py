"""What every test file of the device has in common (TEST INFRASTRUCTURE): `from gpu_support import built  # noqa: F401` makes the
fixture below the importing module's own — autouse, once per module — the way the CPU files import `emu`."""
import pytest

from karpenter_amd.scheduling import device_available


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__
    __graft_entry__.build()
    assert device_available(), "GPU tests need a usable gfx950 device and karpenter_amd/libksolve.so (no CPU fallback)"
