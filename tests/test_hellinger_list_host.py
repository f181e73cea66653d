"""Host side of pm_hellinger_list (no GPU): workspace sizes, argument checks before anything is enqueued, and hl_list_kernel's
resources as the product's flags compile it."""
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
    size = lib.pm_hellinger_list_workspace
    assert size(0, 0, 0) == 0 and size(100, 100, 5) == 0 and size(100, 0, 1) == 0 and size(-1, 100, 1) == 0
    assert size(40000, 2000, 2) > size(1000, 2000, 2) > 0 and size(1000, 50000, 2) > size(1000, 2000, 2) < size(1000, 2000, 4)
    assert all(size(n + 1, 77, 1) >= size(n, 77, 1) for n in range(1, 40000, 61))


# (scA, u, frames, cap, workspace bytes) -> code: a short and a missing workspace, NULL arguments, bad frame counts, cap <= 0
@pytest.mark.parametrize("sc_a,u,frames,cap,ws_bytes,want", [
    (0x1000, 0x1000, 4, 640, 64, -2), (0x1000, 0x1000, 4, 640, 0, -2), (None, 0x1000, 4, 640, 1 << 40, -1), (0x1000, None, 4, 640, 1 << 40, -1),
    (0x1000, 0x1000, 0, 640, 1 << 40, -1), (0x1000, 0x1000, 5, 640, 1 << 40, -1), (0x1000, 0x1000, 4, 0, 1 << 40, -1), (0x1000, 0x1000, 4, -5, 1 << 40, -1)])
def test_argument_errors_come_before_any_launch(lib, sc_a, u, frames, cap, ws_bytes, want):
    fake = ctypes.c_void_p(0x1000)               # never dereferenced
    ws = fake if ws_bytes else None
    assert lib.pm_hellinger_list(sc_a, 10, fake, 10, 3600, frames, u, fake, None, 0.0, 0, fake, fake, cap, fake, fake, ws, ws_bytes, None) == want


def test_list_kernel_resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    rows = {r["name"].split("::")[-1]: r for r in kernel_resources.census(["pm_hellinger.hip"])}
    k = rows["hl_list_kernel"]
    assert k["scratch"] == 0 and k["spills"] == 0
    assert k["lds"] <= 80 * 1024 and k["workgroups"] >= 2 and k["waves"] >= 2      # two workgroups per CU, two waves per SIMD
