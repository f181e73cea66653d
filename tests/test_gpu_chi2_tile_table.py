"""The half-cost kernel decides PER TILE (16 moving rows x 64 fixed columns) which (ring, theta) shells it serves from the term
table (csrc/pm_chi2.hip: tabmask): a shell is tabled in a tile iff every count of the shell in the tile's 16 + 64 descriptors is
below the table's side, 94.  Statements: whatever the tiles choose, all eight matrices carry the bits of the general four-frame
kernel (the reference's, shape_context.py:88-99); and the tiles choose exactly as stated (pm_chi2_sym_ws_report's per-shell tile
counts).  Descriptors are integer counts over one common total, as the existing term-table tests build them, so the table is live.

40 x 150 descriptors: row tiles 0..15, 16..31, 32..39 (ragged: the kernel's clamped indices repeat row 39), column tiles 0..63,
64..127, 128..149 (ragged) — nine tiles.

One case of the issue's list cannot exist and is absent: "a shell where every tile qualifies although the launch-wide maximum
does not".  The launch-wide maximum of a shell is a count in some row (or column), every row belongs to a tile row, so the
tiles of that tile row (column) do not qualify.  What the rule buys is the converse, which the first test pins: ONE offending row
costs its own tile row the shell and no other."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NA, NB, TOTAL, TL, G = 40, 150, 1000, 94, 13
TILES, PER_TILE_ROW, PER_TILE_COL = 9, 3, 3
Q = np.arange(12)


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


def base_counts():
    """Counts 0..40 everywhere (every shell below the table's side in every row), a singly occupied bin in each cloud (the
    kernel reads the common total off the smallest positive value), shell G filled up to 93."""
    rng = np.random.default_rng(94)
    ca, cb = rng.integers(0, 41, (NA, 360)), rng.integers(0, 41, (NB, 360))
    ca[:, 0], cb[:, 0] = 1, 1
    ca[:, G * 12:G * 12 + 12] = rng.integers(80, 94, (NA, 12))
    cb[:, G * 12:G * 12 + 12] = rng.integers(80, 94, (NB, 12))
    ca[1, G * 12 + 3] = ca[20, G * 12] = ca[39, G * 12 + 11] = 93
    cb[2, G * 12 + 5] = cb[100, G * 12 + 7] = cb[149, G * 12] = 93
    return ca, cb


def frames(f1):
    """Frames 2..4 as the phi permutations of frame 1 (shape_context.py:172-181 away from sector edges)."""
    s = f1.reshape(-1, 30, 12)
    return np.stack([s, s[:, :, (Q + 6) % 12], s[:, :, 11 - Q], s[:, :, (17 - Q) % 12]]).reshape(4, -1, 360)


def run(g, a, b, pairing=-1):
    """-> (the kernel's matrices, the general kernel's on the expanded frames, tiles per shell)"""
    da, db = g.nat.to_dev(np.ascontiguousarray(frames(a)[:2])), g.nat.to_dev(np.ascontiguousarray(frames(b)))
    want = g.K.chi2_cost8(da, db, path="general")
    got, tabled, tiles = g.K.chi2_frame1_tile_report(da[0], db[0], pairing)
    assert tiles == TILES
    return got, want, tabled.cpu().numpy()


def same_bits(g, x, y):
    return g.t.equal(x.contiguous().view(g.t.int64), y.contiguous().view(g.t.int64))


def test_all_shells_below_the_side_are_tabled_in_every_tile(g):
    ca, cb = base_counts()
    got, want, tabled = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    assert tabled.tolist() == [TILES] * 30


@pytest.mark.parametrize("which,index", [("row", 5), ("row", 20), ("row", NA - 1), ("column", 70), ("column", 0), ("column", NB - 1)])
def test_one_count_of_94_costs_only_its_own_tiles_the_shell(g, which, index):
    """A single descriptor with a count of exactly 94 in shell G (93 elsewhere, in every tile): the three tiles of its tile row
    (column) compute the shell, the six others table it; row 39 is the row the ragged tile's clamped indices repeat, column 149
    the last of the ragged column tile."""
    ca, cb = base_counts()
    (ca if which == "row" else cb)[index, G * 12 + 4] = TL
    got, want, tabled = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    expect = [TILES] * 30
    expect[G] = TILES - (PER_TILE_ROW if which == "row" else PER_TILE_COL)
    assert tabled.tolist() == expect


def test_a_row_and_a_column_of_94_leave_the_four_tiles_off_both(g):
    ca, cb = base_counts()
    ca[17, G * 12 + 1] = TL
    cb[140, G * 12 + 9] = TL + 20
    got, want, tabled = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    assert tabled[G] == 4 and tabled.sum() == 29 * TILES + 4


def test_a_tile_with_no_eligible_shell_skips_the_table_beside_neighbours_that_use_it(g):
    """Row 3 holds a 94 in EVERY shell: the tiles of tile row 0 have an empty mask (no table fill, every term computed), the six
    tiles below table all thirty shells."""
    ca, cb = base_counts()
    ca[3, 2::12] = TL
    got, want, tabled = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    assert tabled.tolist() == [TILES - PER_TILE_ROW] * 30


def test_a_value_that_is_not_count_over_total_rules_the_table_out_in_every_tile(g):
    ca, cb = base_counts()
    cb[77, 200] = 7
    a, b = ca / TOTAL, cb / TOTAL
    b[77, 200] = np.nextafter(b[77, 200], 1.0)
    got, want, tabled = run(g, a, b)
    assert same_bits(g, got, want)
    assert tabled.tolist() == [0] * 30


def test_saturated_counts_are_never_tabled(g):
    """Counts are kept as bytes saturated at 255: a shell that holds 255, 300 or 999 somewhere in every tile row is computed
    everywhere (and 999 / 1000 still verifies as count / total)."""
    ca, cb = base_counts()
    ca[0, 20 * 12], ca[16, 20 * 12 + 5], ca[NA - 1, 20 * 12 + 11] = 255, 300, 999
    got, want, tabled = run(g, ca / TOTAL, cb / TOTAL)
    assert same_bits(g, got, want)
    expect = [TILES] * 30
    expect[20] = 0
    assert tabled.tolist() == expect


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_one_pairing_alone_chooses_the_same_tiles(g, t):
    ca, cb = base_counts()
    ca[NA - 1, G * 12 + 4] = TL
    cb[70, (G + 1) * 12] = TL
    got, want, tabled = run(g, ca / TOTAL, cb / TOTAL, pairing=t)
    h, twin = g.PAIRINGS[t]
    assert same_bits(g, got[0], want[h]) and same_bits(g, got[1], want[twin])
    expect = [TILES] * 30
    expect[G], expect[G + 1] = TILES - PER_TILE_ROW, TILES - PER_TILE_COL
    assert tabled.tolist() == expect


@pytest.mark.parametrize("cap", [3, 6])
def test_banded_launches_read_the_counts_of_their_own_rows(g, monkeypatch, cap):
    """PM_CHI2_MAX_BLOCKS cuts the nine tiles into bands of one or two tile rows, each launched on offset pointers: the offending
    rows 20 and 39 must cost the tile rows they are in, in whichever band, and the report adds up over the bands."""
    ca, cb = base_counts()
    ca[20, G * 12 + 4] = TL
    ca[NA - 1, (G + 1) * 12] = TL
    a, b = ca / TOTAL, cb / TOTAL
    monkeypatch.delenv("PM_CHI2_MAX_BLOCKS", raising=False)
    whole, want, tabled_whole = run(g, a, b)
    monkeypatch.setenv("PM_CHI2_MAX_BLOCKS", str(cap))
    banded, _, tabled = run(g, a, b)
    pair, _, tabled_pair = run(g, a, b, pairing=2)
    g.t.cuda.synchronize()
    assert same_bits(g, whole, want) and same_bits(g, banded, want)
    h, twin = g.PAIRINGS[2]
    assert same_bits(g, pair[0], want[h]) and same_bits(g, pair[1], want[twin])
    expect = [TILES] * 30
    expect[G] = expect[G + 1] = TILES - PER_TILE_ROW
    assert tabled_whole.tolist() == expect and tabled.tolist() == expect and tabled_pair.tolist() == expect
