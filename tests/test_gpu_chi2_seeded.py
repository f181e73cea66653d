"""Seeded division in the half-cost chi-square kernel (csrc/pm_chi2.hip: NSP, pm_common.h: div_seeded).  When both clouds have one
common total T, a shell whose two launch-wide maxima sum below NSEED = 94^2 may take its reciprocals from the count-sum table
R[s] = fl(T/s) that a tile lays over its term table from its switch shell g_sw on.  Statements: whatever a tile does, all eight
matrices carry the bits of the general four-frame kernel; eligibility is as pm_chi2_sym_seed_info reports it; and the per-tile
report (pm_chi2_sym_ws_report) counts a shell as tabled only where it really came from the term table.

40 x 150 descriptors, nine tiles, ragged in both directions, integer counts over a common total, frames by the phi
permutations — as tests/test_gpu_chi2_tile_table.py.  Every case runs with all four pairings of a row seeded and with two
(PM_CHI2_SEED, read per launch), whichever of them the product ships."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NA, NB, TOTAL, TL, NSEED = 40, 150, 20000, 94, 94 * 94
TILES, PER_TILE_ROW = 9, 3
Q = np.arange(12)
OUTER = slice(12 * 12, 360)          # rings 2..4: shells 12..29


@pytest.fixture(scope="module")
def g():
    import torch
    from platymatch_amd import _kernels as K, _native as nat
    from platymatch_amd._pairings import PAIRINGS
    nat.load()
    assert torch.cuda.is_available(), "gpu-marked tests need a ROCm device"

    class G_:
        pass
    G_.K, G_.nat, G_.t, G_.PAIRINGS = K, nat, torch, PAIRINGS
    return G_


@pytest.fixture(params=["4", "2"])
def seeded_pairings(request, monkeypatch):
    monkeypatch.setenv("PM_CHI2_SEED", request.param)
    monkeypatch.delenv("PM_CHI2_MAX_BLOCKS", raising=False)
    return request.param


def base_counts(seed=8836):
    """Rings 0 and 1: counts 0..40 (tabled everywhere); rings 2..4: counts 100..4000 (far above the term table's side and above
    the count bytes' 255); a singly occupied bin in each cloud, from which the kernel reads the total."""
    rng = np.random.default_rng(seed)
    ca, cb = rng.integers(0, 41, (NA, 360)), rng.integers(0, 41, (NB, 360))
    ca[:, OUTER], cb[:, OUTER] = rng.integers(100, 4001, (NA, 216)), rng.integers(100, 4001, (NB, 216))
    ca[:, 0], cb[:, 0] = 1, 1
    return ca, cb


def frames(f1):
    s = f1.reshape(-1, 30, 12)
    return np.stack([s, s[:, :, (Q + 6) % 12], s[:, :, 11 - Q], s[:, :, (17 - Q) % 12]]).reshape(4, -1, 360)


def run(g, a, b, pairing=-1):
    """-> (the kernel's matrices, the general kernel's, tiles per shell that tabled it, launch-wide seed eligibility)"""
    da, db = g.nat.to_dev(np.ascontiguousarray(frames(a)[:2])), g.nat.to_dev(np.ascontiguousarray(frames(b)))
    want = g.K.chi2_cost8(da, db, path="general")
    got, tabled, tiles = g.K.chi2_frame1_tile_report(da[0], db[0], pairing)
    seeded, nseed = g.K.chi2_frame1_seed_info(da[0], db[0])
    assert tiles == TILES and nseed == NSEED
    return got, want, tabled.cpu().numpy().tolist(), seeded


def same_bits(g, x, y):
    return g.t.equal(x.contiguous().view(g.t.int64), y.contiguous().view(g.t.int64))


def test_outer_rings_are_seeded_and_the_bits_stay(g, seeded_pairings):
    ca, cb = base_counts()
    got, want, tabled, seeded = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    assert seeded == [1] * 30                      # (every shell's maxima sum to at most 8 000)
    assert tabled == [TILES] * 12 + [0] * 18       # switch shell 12 in every tile


@pytest.mark.parametrize("top,eligible", [(NSEED - 1 - 4000, 1), (NSEED - 4000, 0)])
def test_a_shell_is_eligible_up_to_a_maxima_sum_of_nseed_minus_one(g, seeded_pairings, top, eligible):
    ca, cb = base_counts()
    ca[7, 20 * 12 + 2] = 4000                      # the moving cloud's maximum in shell 20
    cb[149, 20 * 12 + 9] = top                     # the fixed cloud's: the sum is NSEED - 1 or NSEED
    got, want, tabled, seeded = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    expect = [1] * 30
    expect[20] = eligible
    assert seeded == expect and tabled == [TILES] * 12 + [0] * 18


def test_a_count_above_65535_is_not_wrapped_into_eligibility(g, seeded_pairings):
    """Total 200 000; shell 25 holds 70 000 in one moving row and at most 40 in the fixed cloud: 70 000 mod 65 536 + 40 would be
    below NSEED.  Counts above 255 are in every outer shell."""
    ca, cb = base_counts()
    cb[:, 25 * 12:26 * 12] = np.random.default_rng(1).integers(0, 41, (NB, 12))
    ca[5, 25 * 12 + 3] = 70000
    got, want, tabled, seeded = run(g, ca / 200000, cb / 200000)
    assert same_bits(g, got, want)
    expect = [1] * 30
    expect[25] = 0
    assert seeded == expect and tabled == [TILES] * 12 + [0] * 18


def test_zero_counts_on_either_side_and_on_both(g, seeded_pairings):
    rng = np.random.default_rng(2)
    ca, cb = base_counts()
    ca[:, OUTER] *= rng.integers(0, 2, (NA, 216))
    cb[:, OUTER] *= rng.integers(0, 2, (NB, 216))
    ca[:, 15 * 12:16 * 12] = 0                     # a seeded shell that is empty in the whole moving cloud
    cb[64:128, 15 * 12:16 * 12] = 0                # ... and in one column tile of the fixed cloud: s = 0 throughout
    got, want, tabled, seeded = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    assert seeded == [1] * 30 and tabled[:12] == [TILES] * 12


def test_unequal_totals_seed_nothing(g, seeded_pairings):
    ca, cb = base_counts()
    got, want, tabled, seeded = run(g, ca / TOTAL, cb / (TOTAL - 1))
    assert same_bits(g, got, want)
    assert seeded == [0] * 30 and tabled == [TILES] * 12 + [0] * 18


def late_tabled_counts():
    """Only the moving rows 0..15 hold large counts, in shells 12..28; shell 29 is small everywhere.  The three tiles of tile row 0
    have the mask {0..11, 29}: switching at 12 (12 tabled, 18 seeded: 12 * 85 + 18 * 216 = 4 908) beats keeping the table (13 tabled, 17
    computed: 5 185), so shell 29 is seeded there.  The six tiles below table all thirty shells and keep their table."""
    rng = np.random.default_rng(3)
    ca, cb = rng.integers(0, 41, (NA, 360)), rng.integers(0, 41, (NB, 360))
    ca[:16, 12 * 12:29 * 12] = rng.integers(100, 4001, (16, 17 * 12))
    ca[:, 0], cb[:, 0] = 1, 1
    return ca, cb


def test_a_tabled_shell_after_the_switch_is_seeded_and_reported_as_not_tabled(g, seeded_pairings):
    ca, cb = late_tabled_counts()
    got, want, tabled, seeded = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    assert seeded == [1] * 30
    assert tabled == [TILES] * 12 + [TILES - PER_TILE_ROW] * 18


def test_without_seeds_the_late_shell_is_tabled_in_every_tile(g, monkeypatch):
    monkeypatch.setenv("PM_CHI2_SEED", "0")
    ca, cb = late_tabled_counts()
    got, want, tabled, _ = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    assert tabled == [TILES] * 12 + [TILES - PER_TILE_ROW] * 17 + [TILES]


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_one_pairing_alone_is_seeded_too(g, seeded_pairings, t):
    ca, cb = base_counts()
    ca[:, 14 * 12:15 * 12] *= np.random.default_rng(4).integers(0, 2, (NA, 12))
    got, want, tabled, seeded = run(g, ca / TOTAL, cb / TOTAL, pairing=t)
    h, twin = g.PAIRINGS[t]
    assert same_bits(g, got[0], want[h]) and same_bits(g, got[1], want[twin])
    assert seeded == [1] * 30 and tabled == [TILES] * 12 + [0] * 18


@pytest.mark.parametrize("cap", [3, 6])
def test_banded_launches(g, seeded_pairings, monkeypatch, cap):
    ca, cb = late_tabled_counts()
    ca[39, 20 * 12 + 1] = 3000                     # the ragged tile row switches too (shells 12..19 stay tabled there: see below)
    a, b = ca / TOTAL, cb / TOTAL
    whole, want, tabled_whole, _ = run(g, a, b)
    monkeypatch.setenv("PM_CHI2_MAX_BLOCKS", str(cap))
    banded, _, tabled, seeded = run(g, a, b)
    pair, _, tabled_pair, _ = run(g, a, b, pairing=1)
    g.t.cuda.synchronize()
    assert same_bits(g, whole, want) and same_bits(g, banded, want)
    h, twin = g.PAIRINGS[1]
    assert same_bits(g, pair[0], want[h]) and same_bits(g, pair[1], want[twin])
    # tile row 2 (rows 32..39): mask = all but shell 20.  Keeping the table costs 29 * 85 + 240 = 2 705; switching at 20 costs
    # 20 * 85 + 10 * 216 = 3 860: it keeps the table and computes shell 20
    expect = [TILES] * 12 + [TILES - PER_TILE_ROW] * 18
    expect[20] = TILES - 2 * PER_TILE_ROW
    assert seeded == [1] * 30
    assert tabled_whole == expect and tabled == expect and tabled_pair == expect
