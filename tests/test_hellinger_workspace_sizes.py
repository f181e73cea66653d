"""Workspace sizes of the four Hellinger entry points (no GPU): literal values recorded from the build that still had one layout
function per entry point, so that the shared layout (csrc/pm_hellinger.h: hl_layout) cannot move a byte unnoticed."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from platymatch_amd import _native
    from platymatch_amd.build import build_native
    build_native()
    return _native.load()


# (nA, nB, F, k) -> (topk, select, select_bf16, list); the bf16 query serves k <= 32 and is asked with k = 32 at the last shape
SIZES = {
    (1, 1, 1, 1): (381952, 763904, 1379328, 370944),
    (64, 64, 1, 16): (3331072, 6662144, 13175808, 370944),
    (65, 129, 1, 16): (6754816, 6847488, 13373440, 556288),
    (129, 257, 4, 17): (28870144, 56072192, 56244224, 2595072),
    (5, 3000, 4, 32): (42680832, 68310016, 120031232, 17978624),
    (20000, 20000, 4, 16): (170197504, 195826688, 256002048, 145495296),
    (50000, 50000, 4, 64): (463010816, 563674112, 587894784, 362347776),
}


@pytest.mark.parametrize("shape", sorted(SIZES))
def test_workspace_sizes(lib, shape):
    nA, nB, F, k = shape
    got = (lib.pm_hellinger_topk_workspace(nA, nB, F, k), lib.pm_hellinger_select_workspace(nA, nB, F, k),
           lib.pm_hellinger_select_bf16_workspace(nA, nB, F, min(k, 32)), lib.pm_hellinger_list_workspace(nA, nB, F))
    assert got == SIZES[shape]
