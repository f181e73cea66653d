"""Host side of pm_hellinger_topk (no GPU): workspace sizes, argument checks before anything is enqueued, the error bound, and
the main kernel's resources as the product's flags compile it."""
import ctypes
import os
import sys

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from platymatch_amd import _native
    from platymatch_amd.build import build_native
    build_native()
    return _native.load()


def test_workspace_is_monotone_and_zero_for_zeros(lib):
    size = lib.pm_hellinger_topk_workspace
    assert size(0, 0, 0, 0) == 0 and size(100, 100, 5, 16) == 0 and size(100, 100, 1, 65) == 0
    base = (1000, 2000, 2, 16)
    for arg, bigger in enumerate((40000, 50000, 4, 64)):
        grown = list(base)
        grown[arg] = bigger
        assert size(*grown) > size(*base) > 0, arg
    assert all(size(n + 1, 77, 1, 8) >= size(n, 77, 1, 8) for n in range(1, 40000, 61))      # also across the split regimes


@pytest.mark.parametrize("k,frames,ws_bytes,want", [(16, 4, 64, -2), (0, 4, 1 << 40, -1), (65, 4, 1 << 40, -1), (16, 5, 1 << 40, -1)])
def test_argument_errors_come_before_any_launch(lib, k, frames, ws_bytes, want):
    fake = ctypes.c_void_p(0x1000)               # never dereferenced
    assert lib.pm_hellinger_topk(fake, 10, fake, 10, 3600, frames, k, 0, fake, fake, fake, fake, ws_bytes, None) == want
    assert lib.pm_hellinger_topk(fake, 10, fake, 10, 3600, 4, 16, 0, fake, fake, fake, None, 0, None) == -2


def test_delta(lib):
    d = ctypes.c_double(0.0)
    assert lib.pm_hellinger_delta(ctypes.addressof(d)) == 0 and 0.0 < d.value < 1e-4
    assert d.value >= 722 * 2.0 ** -24           # the derivation in csrc/pm_hellinger.hip


def test_main_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = {r["name"].split("::")[-1]: r for r in kernel_resources.census(["pm_hellinger.hip"])}
    main = rows["hl_topk_kernel"]
    assert main["scratch"] == 0 and main["spills"] == 0
    assert main["workgroups"] >= 1 and main["waves"] >= 1 and main["lds"] <= 160 * 1024      # one workgroup per CU, one wave per SIMD
    assert all(r["scratch"] == 0 and r["spills"] == 0 for r in rows.values())
