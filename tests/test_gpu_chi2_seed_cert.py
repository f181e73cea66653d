"""The per-launch certificate of the short seeded division (csrc/pm_chi2.hip: seed_cert_kernel, pm_seed_short.h:
div_seeded_short).  The product's half-cost kernel divides its seeded terms WITHOUT the Newton step, after a kernel has checked,
for the launch's own total and every count pair the launch can meet, that this gives div_pos's bits; where the certificate reads 0
(PM_CHI2_SEED_CERT=0 forces that) the launch seeds nothing and runs as under PM_CHI2_SEED=0.  Statements: either way all eight
matrices carry the bits of the general four-frame kernel; pm_chi2_sym_seed_info reports the eligible shells with the certificate
and none without it; and a shell whose maxima sum reaches NSEED = 94^2 stays computed.

37 x 150 descriptors (nine 16 x 64 tiles, ragged in both directions), integer counts over a common total T in {999, 49 999},
frames by the phi permutations, as tests/test_gpu_chi2_seeded.py.  A descriptor value is at most 1, so with T = 999 the counts stop
at 999 and no shell can reach NSEED; with T = 49 999 shell 20's maxima sum to NSEED - 1 and shell 21's to NSEED."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NA, NB, NSEED = 37, 150, 94 * 94
TILES = 9
TOTALS = [999, 49999]
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
    G_.cases = {}
    return G_


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for name in ("PM_CHI2_SEED", "PM_CHI2_SEED_CERT", "PM_CHI2_MAX_BLOCKS"):
        monkeypatch.delenv(name, raising=False)


def shell(g0, g1=None):
    return slice(12 * g0, 12 * (g0 + 1 if g1 is None else g1))


def counts(total):
    """shells 0..7: zeros and counts up to 40; 8..11: every count below the term table's side; 12..19: mid-range counts, a third of
    them zero on either side; 20: maxima summing to NSEED - 1 (or to 2 T where that is less); 21: to NSEED (T = 49 999);
    22..29: mid-range with whole rows and columns of zeros.  Bin 0 holds count 1 in both clouds: the kernel reads T from it."""
    rng = np.random.default_rng(total)
    hi_a, hi_b = min(total, 4400), min(total, NSEED - 1 - 4400)
    ca, cb = rng.integers(0, 41, (NA, 360)), rng.integers(0, 41, (NB, 360))
    ca[:, shell(0, 8)] *= rng.integers(0, 2, (NA, 96))
    cb[:, shell(0, 8)] *= rng.integers(0, 2, (NB, 96))
    ca[:, shell(8, 12)], cb[:, shell(8, 12)] = rng.integers(0, 94, (NA, 48)), rng.integers(0, 94, (NB, 48))
    ca[:, shell(12, 30)] = rng.integers(94, hi_a + 1, (NA, 216)) * (rng.integers(0, 3, (NA, 216)) > 0)
    cb[:, shell(12, 30)] = rng.integers(94, hi_b + 1, (NB, 216)) * (rng.integers(0, 3, (NB, 216)) > 0)
    ca[3, 20 * 12 + 2], cb[149, 20 * 12 + 9] = hi_a, hi_b                  # 4 400 + 4 435 = NSEED - 1
    if total >= NSEED:
        ca[36, 21 * 12 + 11], cb[64, 21 * 12] = hi_a, hi_b + 1             # NSEED: shell 21 stays computed
    ca[16:32, shell(22, 30)] = 0
    cb[64:128, shell(26, 30)] = 0
    ca[:, 0], cb[:, 0] = 1, 1
    return ca, cb


def frames(f1):
    s = f1.reshape(-1, 30, 12)
    return np.stack([s, s[:, :, (Q + 6) % 12], s[:, :, 11 - Q], s[:, :, (17 - Q) % 12]]).reshape(4, -1, 360)


def case(g, total, fixed_total=None):
    """the descriptors on the device and the general kernel's eight matrices, computed once per (T, fixed cloud's T)"""
    key = (total, fixed_total or total)
    if key not in g.cases:
        ca, cb = counts(total)
        da = g.nat.to_dev(np.ascontiguousarray(frames(ca / key[0])[:2]))
        db = g.nat.to_dev(np.ascontiguousarray(frames(cb / key[1])))
        g.cases[key] = (da, db, g.K.chi2_cost8(da, db, path="general"))
    return g.cases[key]


def run(g, da, db, pairing=-1):
    got, tabled, tiles = g.K.chi2_frame1_tile_report(da[0], db[0], pairing)
    seeded, nseed = g.K.chi2_frame1_seed_info(da[0], db[0])
    assert tiles == TILES and nseed == NSEED
    return got, tabled.cpu().numpy().tolist(), seeded


def same_bits(g, x, y):
    return g.t.equal(x.contiguous().view(g.t.int64), y.contiguous().view(g.t.int64))


def eligible(total):
    e = [1] * 30
    if total >= NSEED:
        e[21] = 0
    return e


@pytest.mark.parametrize("total", TOTALS)
def test_certified_launch_keeps_the_bits_and_the_eligible_shells(g, total):
    da, db, want = case(g, total)
    got, tabled, seeded = run(g, da, db)
    assert same_bits(g, got, want)
    assert seeded == eligible(total)
    assert tabled[:12] == [TILES] * 12 and tabled[21] == 0


@pytest.mark.parametrize("total", TOTALS)
def test_without_the_certificate_nothing_is_seeded_and_the_bits_stay(g, monkeypatch, total):
    da, db, want = case(g, total)
    monkeypatch.setenv("PM_CHI2_SEED", "0")
    _, tabled_unseeded, _ = run(g, da, db)
    monkeypatch.delenv("PM_CHI2_SEED")
    monkeypatch.setenv("PM_CHI2_SEED_CERT", "0")
    got, tabled, seeded = run(g, da, db)
    assert same_bits(g, got, want)
    assert seeded == [0] * 30
    assert tabled == tabled_unseeded               # the tiles do what they do under PM_CHI2_SEED=0
    monkeypatch.delenv("PM_CHI2_SEED_CERT")
    assert run(g, da, db)[2] == eligible(total)    # read per launch: the next launch is certified again


@pytest.mark.parametrize("cert", ["1", "0"])
def test_unequal_totals(g, monkeypatch, cert):
    da, db, want = case(g, 49999, 49998)
    monkeypatch.setenv("PM_CHI2_SEED_CERT", cert)
    got, _, seeded = run(g, da, db)
    assert same_bits(g, got, want)
    assert seeded == [0] * 30


@pytest.mark.parametrize("cert", ["1", "0"])
@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_one_pairing_alone(g, monkeypatch, t, cert):
    da, db, want = case(g, 49999)
    monkeypatch.setenv("PM_CHI2_SEED_CERT", cert)
    got, _, seeded = run(g, da, db, pairing=t)
    h, twin = g.PAIRINGS[t]
    assert same_bits(g, got[0], want[h]) and same_bits(g, got[1], want[twin])
    assert seeded == (eligible(49999) if cert == "1" else [0] * 30)


def test_two_seeded_pairings_per_row(g, monkeypatch):
    """the measurement knob's other seeding kernel (PM_CHI2_SEED=2) goes through the same certificate"""
    da, db, want = case(g, 49999)
    monkeypatch.setenv("PM_CHI2_SEED", "2")
    got, _, seeded = run(g, da, db)
    assert same_bits(g, got, want) and seeded == eligible(49999)
    monkeypatch.setenv("PM_CHI2_SEED_CERT", "0")
    got, _, seeded = run(g, da, db)
    assert same_bits(g, got, want) and seeded == [0] * 30
