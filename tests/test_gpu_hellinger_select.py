"""hellinger_select (csrc/pm_hellinger.hip: hl_select_kernel, the per-row top-k of the Hellinger lower bound under column prices)
against the float64 NumPy keys 0.5 (sum a + sum b) - sqrt a . sqrt b - v, against hellinger_topk's and hellinger_list's bits, the
exact costs of chi2_cost, and through the public call."""
import functools
import types

import numpy as np
import pytest

from test_gpu_hellinger import reference_bound, synthetic_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import torch
    from platymatch_amd import _kernels as K, _native as nat
    nat.load()
    assert torch.cuda.is_available()
    return types.SimpleNamespace(K=K, nat=nat, t=torch, exact={})


@functools.lru_cache(maxsize=None)
def host_case(n, m, frames, seed):
    a, b = synthetic_case(n, m, frames, seed)
    return a, b, np.stack([reference_bound(a, bf) for bf in b])


def prices(kind, frames, m, seed):
    """'ramp': v_j = 2 j, every later column beats every earlier one; else uniform in [0, 0.5], 'nonfinite' with one NaN and one +inf"""
    if kind == "ramp":
        return np.tile(2.0 * np.arange(m), (frames, 1))
    v = np.random.default_rng(1000 + seed).uniform(0.0, 0.5, (frames, m))
    if kind == "nonfinite":
        v[0, 1], v[-1, m // 2] = np.nan, np.inf
    return v


def reference_keys(ref, v):
    """float64 keys [F, N, M], +inf where the price is not finite (never listed), and the number of listable columns per frame"""
    fin = np.isfinite(v)
    return np.where(fin[:, None, :], ref - np.where(fin, v, 0.0)[:, None, :], np.inf), fin.sum(1)


def gap(keys, fin, k):
    """smallest distance between the k-th and the (k+1)-th reference key of a row, over the frames that have more than k columns"""
    order = np.sort(keys[fin > k], axis=2)
    return (order[:, :, k] - order[:, :, k - 1]).min() if order.size else np.inf


def select(g, ta, tb, v, k, split, info=None):
    return tuple(x.cpu().numpy() for x in g.K.hellinger_select(ta, tb, v=None if v is None else g.nat.to_dev(v), k=k, split=split, info=info))


def check_select(g, n, m, frames, k, splits, seed, v):
    """the assertions of test_gpu_hellinger.check_lists with keys in place of bounds; every split against split 1"""
    a, b, ref = host_case(n, m, frames, seed)
    K, dev, delta = g.K, g.nat.to_dev, g.K.hellinger_delta()
    ta, tb = dev(a), dev(b)
    if (n, m, frames, seed) not in g.exact:
        g.exact[n, m, frames, seed] = np.stack([K.chi2_cost(ta, tb[f].contiguous()).cpu().numpy() for f in range(frames)])
    exact = g.exact[n, m, frames, seed]
    keys, fin = reference_keys(ref, v)
    assert gap(keys, fin, k) > 2 * delta, "choose another seed: %g" % gap(keys, fin, k)
    info = {}
    cols, bound = select(g, ta, tb, v, k, 1, info)
    assert info["nonfinite"] == 0
    assert cols.shape == bound.shape == (frames, n, k) and cols.dtype == np.int32 and bound.dtype == np.float64
    listed = np.broadcast_to((np.arange(k) < np.minimum(fin, k)[:, None])[:, None, :], cols.shape)
    assert np.array_equal(cols >= 0, listed) and (cols < m).all() and np.isposinf(bound[~listed]).all()
    idx, v0 = np.where(listed, cols, 0).astype(np.int64), np.where(np.isfinite(v), v, 0.0)
    sel = np.zeros(ref.shape, bool)
    fi, ni, ri = np.nonzero(listed)
    sel[fi, ni, cols[fi, ni, ri]] = True
    assert sel.sum() == listed.sum() and np.isfinite(keys[sel]).all()                    # distinct, no non-finite price
    dev_max = np.abs(bound - np.take_along_axis(ref, idx, axis=2))[listed].max()
    print("n=%d m=%d frames=%d k=%d: largest |bound - L_float64| = %.3g (delta %.3g)" % (n, m, frames, k, dev_max, delta))
    assert dev_max <= delta
    key = np.where(listed, bound - np.take_along_axis(v0[:, None, :], idx, axis=2), np.inf)
    assert (key[:, :, 1:] >= key[:, :, :-1]).all()
    unlisted, kth = np.isfinite(keys) & ~sel, key[:, :, k - 1:k]
    assert (keys >= kth - delta)[unlisted].all()
    full = fin > k                                                                       # the gap determines the listed SET
    assert not full.any() or np.array_equal(np.sort(idx[full], axis=2), np.sort(np.argsort(keys[full], axis=2, kind="stable")[:, :, :k], axis=2))
    red = exact - v0[:, None, :]
    assert (np.take_along_axis(red, idx, axis=2) >= key - delta)[listed].all() and (red >= kth - delta)[unlisted].all()
    for split in splits:
        c2, b2 = select(g, ta, tb, v, k, split)
        assert np.array_equal(c2, cols) and np.array_equal(b2.view(np.int64), bound.view(np.int64)), split
    u = np.where(np.isfinite(kth[:, :, 0]), kth[:, :, 0], 1e300)      # hellinger_list under (u = key_k, v, tau = 0) lists them too
    for f, (rows, lc, lb) in enumerate(K.hellinger_list(ta, tb, dev(u), dev(v0), 0.0)):
        L = np.full((n, m), np.nan)
        L[rows.cpu().numpy(), lc.cpu().numpy()] = lb.cpu().numpy()
        assert np.array_equal(np.take_along_axis(L, idx[f], axis=1)[listed[f]].view(np.int64), bound[f][listed[f]].view(np.int64))
    return cols, bound


# (N, M, frames, k, splits, seed): ragged panel and tile, the first tile overflows CAP = 32; one row past a panel and one column
# past two tiles; k = 1; M < k (tails); the CAP = 80 instance with forced and automatic splits and the merge; the first k of the
# large instance.  The seeds are the first for which the float64 reference separates every row's k-th and (k+1)-th KEY by more
# than 2 delta without prices; PRICE_SEEDS, case by case, the first for which it does under prices('random') and
# prices('nonfinite') on those descriptors (the ramp separates the keys by more than 1).
CASES = [(70, 90, 4, 16, (0,), 10), (129, 257, 1, 16, (0, 2), 16), (33, 65, 2, 1, (0,), 1), (40, 9, 1, 16, (0, 3), 1),
         (5, 3000, 4, 64, (0, 7), 44), (70, 200, 1, 17, (0,), 2)]
PRICE_SEEDS = (67, 6, 1, 1, 5, 1)


@pytest.mark.parametrize("n,m,frames,k,splits,seed", CASES)
def test_unpriced_lists_are_hellinger_topk(g, n, m, frames, k, splits, seed):
    a, b, _ = host_case(n, m, frames, seed)
    ta, tb = g.nat.to_dev(a), g.nat.to_dev(b)
    cols, bound = (x.cpu().numpy() for x in g.K.hellinger_topk(ta, tb, k=k))
    for v in (None, np.zeros((frames, m))):
        for split in (1,) + splits:
            c2, b2 = select(g, ta, tb, v, k, split)
            assert np.array_equal(c2, cols) and np.array_equal(b2.view(np.int64), bound.view(np.int64)), split
    check_select(g, n, m, frames, k, (), seed, np.zeros((frames, m)))


@pytest.mark.parametrize("kind", ["random", "ramp", "nonfinite"])
@pytest.mark.parametrize("n,m,frames,k,splits,seed,price_seed", [c + (p,) for c, p in zip(CASES, PRICE_SEEDS)])
def test_priced_lists_against_the_float64_keys_and_the_exact_costs(g, n, m, frames, k, splits, seed, price_seed, kind):
    v, ref = prices(kind, frames, m, price_seed), host_case(n, m, frames, seed)[2]
    if kind == "random" and m > k:          # on the reference alone: the prices change some row's set, or they test nothing
        top = [np.sort(np.argsort(x, axis=2, kind="stable")[:, :, :k], axis=2) for x in (ref, ref - v[:, None, :])]
        assert (top[0] != top[1]).any()
    cols, _ = check_select(g, n, m, frames, k, splits, seed, v)
    if kind == "ramp":                      # the last k columns, the last one first
        want = np.where(np.arange(k) < m, m - 1 - np.arange(k), -1)
        assert (cols == want).all()
    if kind == "nonfinite":
        assert not (cols[0] == 1).any() and not (cols[-1] == m // 2).any()


def test_the_public_call(g):
    from platymatch_amd.estimate_transform import shape_context as S
    n, m, frames, k, _, seed = CASES[0]
    a, b, _ = host_case(n, m, frames, seed)
    v, delta = prices("random", frames, m, PRICE_SEEDS[0]), g.K.hellinger_delta()
    cols, bound = select(g, g.nat.to_dev(a), g.nat.to_dev(b), v, k, 0)
    pc, lower = S.unary_distance_candidates(a, tuple(b), k=k, col_offsets=v)
    assert isinstance(pc, np.ndarray) and np.array_equal(pc, cols) and np.array_equal(lower, bound - delta)
    tc, tb = (x.cpu().numpy() for x in g.K.hellinger_topk(g.nat.to_dev(a), g.nat.to_dev(b), k=k))
    pc, lower = S.unary_distance_candidates(a, tuple(b), k=k)
    assert np.array_equal(pc, tc) and np.array_equal(lower, tb - delta)


def test_a_tie_across_splits_is_broken_by_column(g):
    """Fixed rows 20 and 100 are bit-identical copies of moving row 7: equal bounds, the smallest of the row.  With 130 fixed rows
    the top-k kernel has three 64-row tiles and split 2 or 3 puts the two columns into different partial lists; the selection has
    two 128-row tiles, so its splits run the merge as well.  One merge (hl_select_merge_kernel, with and without prices) serves
    both: the lists are [20, 100, ...] with equal bounds, and the same bits for every split and from both calls."""
    n, m, k = 70, 130, 4
    a, b = synthetic_case(n, m, 1, 3)
    b = b.copy()
    b[0, 20] = b[0, 100] = a[7]
    assert -(-m // 64) >= 3 and -(-m // 128) >= 2 and 20 // 64 != 100 // 64      # split 2 gives S = 2 in both, and cuts between them
    ta, tb = g.nat.to_dev(a), g.nat.to_dev(b)
    outs = []
    for split in (1, 2, 3):
        outs.append(tuple(x.cpu().numpy() for x in g.K.hellinger_topk(ta, tb, k=k, split=split)))
        for v in (None, np.zeros((1, m))):
            outs.append(select(g, ta, tb, v, k, split))
    cols, bound = outs[0]
    assert cols[0, 7, :2].tolist() == [20, 100] and bound[0, 7, 0].view(np.int64) == bound[0, 7, 1].view(np.int64)
    assert bound[0, 7, 1] < bound[0, 7, 2]
    for c2, b2 in outs[1:]:
        assert np.array_equal(c2, cols) and np.array_equal(b2.view(np.int64), bound.view(np.int64))
