"""hellinger_list (csrc/pm_hellinger.hip: hl_list_kernel, the threshold listing of the Hellinger lower bound under duals) against
the float64 NumPy bound 0.5 (sum a + sum b) - sqrt a . sqrt b, against hellinger_topk's bits, and through the public call."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import torch
    from platymatch_amd import _kernels as K, _native as nat
    nat.load()
    assert torch.cuda.is_available()
    return types.SimpleNamespace(K=K, nat=nat, t=torch)


def descriptors(rng, n, active):
    """count / total rows as get_shape_context normalises them, each row with its own distribution over 40 of the 360 bins"""
    totals, p = rng.integers(5, 401, n), np.zeros((n, 360))
    p[:, active] = rng.dirichlet(0.3 * np.ones(active.size), n)
    return rng.multinomial(totals, p) / totals[:, None]


def make_case(n, m, frames, seed, delta):
    """a [N, 360], b [F, M, 360], the float64 reference bound [F, N, M], duals u, v of the size of the row minima, and a finite tau
    in the middle of the widest gap between the 1 % and the 2 % smallest of the reference's reduced values"""
    rng = np.random.default_rng(seed)
    active = rng.choice(360, 40, replace=False)
    a, b = descriptors(rng, n, active), np.stack([descriptors(rng, m, active) for _ in range(frames)])
    ref = np.stack([0.5 * (a.sum(1)[:, None] + bf.sum(1)[None, :]) - np.sqrt(a) @ np.sqrt(bf).T for bf in b])
    scale = ref.min(axis=2).mean()
    u, v = rng.uniform(0, scale, (frames, n)), rng.uniform(0, scale, (frames, m))
    red = ref - u[:, :, None] - v[:, None, :]
    low = np.sort(red.ravel())[red.size // 100:red.size // 50]
    tau = low[np.argmax(np.diff(low)):][:2].mean()
    assert np.abs(red - tau).min() > 2 * delta, "choose another seed: %g" % np.abs(red - tau).min()
    return a, b, ref, u, v, red, tau


def as_mask(lst, n, m, L=None):
    """one frame's sorted (rows, cols, bound) -> mask [N, M] of the entries (each listed once), bounds; L: the matrix whose bits they carry"""
    rows, cols, bound = (x.cpu().numpy() for x in lst)
    key = rows.astype(np.int64) * m + cols
    assert rows.dtype == cols.dtype == np.int32 and bound.dtype == np.float64 and (np.diff(key) > 0).all()
    assert key.size == 0 or (rows.min() >= 0 and rows.max() < n and cols.min() >= 0 and cols.max() < m)
    mask = np.zeros((n, m), bool)
    mask[rows, cols] = True
    assert L is None or np.array_equal(bound.view(np.int64), L[mask].view(np.int64))
    return mask, bound


# (N, M, frames, forced splits, seed): ragged in both directions inside one tile; one row past a 128-row panel and one column past
# two 128-column tiles; few rows against 24 column tiles with the split automatic (24) and forced to values that do not divide 24
CASES = [(70, 90, 4, (1,), 1), (129, 257, 2, (1, 2), 1), (5, 3000, 1, (1, 7, 5), 1)]


@pytest.mark.parametrize("n,m,frames,splits,seed", CASES)
def test_lists_against_the_float64_bound_and_topk(g, n, m, frames, splits, seed):
    K, dev, delta = g.K, g.nat.to_dev, g.K.hellinger_delta()
    a, b, ref, u, v, red, tau = make_case(n, m, frames, seed, delta)
    ta, tb, tu, tv = dev(a), dev(b), dev(u), dev(v)
    whole, info = K.hellinger_list(ta, tb, tu, tv, np.inf, cap=n * m), {}      # 1. the whole matrix
    L = np.stack([as_mask(whole[f], n, m)[1].reshape(n, m) for f in range(frames)])      # (n * m distinct keys: every entry once)
    assert np.abs(L - ref).max() <= delta
    lists = K.hellinger_list(ta, tb, tu, tv, tau, info=info)      # 2. the listed set at a finite tau, with the whole matrix's bits
    want = red <= tau
    assert info["count"] == [int(w.sum()) for w in want] and sum(info["count"]) > 0
    assert all(np.array_equal(as_mask(lists[f], n, m, L[f])[0], want[f]) for f in range(frames))
    k = 16      # 3. the same bits as hellinger_topk
    idx, kb = (x.cpu().numpy().astype(t) for x, t in zip(K.hellinger_topk(ta, tb, k=k), (np.int64, np.float64)))
    assert np.array_equal(np.take_along_axis(L, idx, axis=2).view(np.int64), kb.view(np.int64))
    top = K.hellinger_list(ta, tb, dev(kb[:, :, k - 1]), dev(np.zeros((frames, m))), 0.0)
    for f in range(frames):
        mask = as_mask(top[f], n, m, L[f])[0]
        assert np.array_equal(mask, L[f] <= kb[f, :, k - 1:k]) and np.take_along_axis(mask, idx[f], axis=1).all()
    for split in splits:      # 4. split independence (the bits are the whole matrix's, which came from the automatic split)
        again = K.hellinger_list(ta, tb, tu, tv, tau, split=split)
        assert all(np.array_equal(as_mask(again[f], n, m, L[f])[0], want[f]) for f in range(frames)), split
    best = ref.argmin(axis=2)      # 5. skip
    skipped = K.hellinger_list(ta, tb, tu, tv, tau, skip=dev(best, dtype=g.t.int32))
    expect = want & (np.arange(m) != best[:, :, None])
    assert all(np.array_equal(as_mask(skipped[f], n, m, L[f])[0], expect[f]) for f in range(frames))


def test_overflow_nonfinite_input_and_the_public_call(g):
    from platymatch_amd.estimate_transform import shape_context as S
    K, dev, t, delta = g.K, g.nat.to_dev, g.t, g.K.hellinger_delta()
    n, m, frames = 70, 90, 2
    a, b, ref, u, v, red, tau = make_case(n, m, frames, 1, delta)
    ta, tb, tu, tv = dev(a), dev(b), dev(u), dev(v)
    want = red <= tau
    true, info = [int(w.sum()) for w in want], {}
    cap, guard = min(true) - 3, 16
    assert K.hellinger_list(ta, tb, tu, tv, tau, cap=cap, info=info) == [None] * frames and info["count"] == true
    rc = t.full((frames, cap + guard, 2), -7, dtype=t.int32, device=ta.device)
    bound = t.full((frames, cap + guard), -7.0, dtype=t.float64, device=ta.device)
    count, flag = t.zeros(frames, dtype=t.int32, device=ta.device), t.zeros(1, dtype=t.int32, device=ta.device)
    K._hellinger_list_raw(ta, tb, tu, tv, None, tau, 0, rc, bound, cap, count, flag)
    rc_h, bound_h = rc.cpu().numpy().reshape(-1, 2), bound.cpu().numpy().ravel()
    assert count.tolist() == true and (rc_h[frames * cap:] == -7).all() and (bound_h[frames * cap:] == -7.0).all()
    for f in range(frames):          # (frame f's list starts at f * cap: the guard is the tail of the flattened buffers)
        r, c = rc_h[f * cap:(f + 1) * cap].T
        assert want[f][r, c].all() and len(set(zip(r.tolist(), c.tolist()))) == cap
        assert (np.abs(bound_h[f * cap:(f + 1) * cap] - ref[f][r, c]) <= delta).all()
    bad_a, bad_b, bad_u = a.copy(), b.copy(), u.copy()          # a NaN and a negative moving row, a NaN fixed row, a NaN dual
    bad_a[9, 0], bad_a[12, 3], bad_b[1, 11, 5], bad_u[0, 20] = np.nan, -1.0, np.nan, np.nan
    lists = K.hellinger_list(dev(bad_a), dev(bad_b), dev(bad_u), tv, np.inf, cap=n * m, info=info)
    assert info["nonfinite"] == 1 and info["count"] == [(n - 3) * m, (n - 2) * (m - 1)]
    for f, lst in enumerate(lists):
        rows, cols = lst[0].cpu().numpy(), lst[1].cpu().numpy()
        assert not np.isin(rows, [9, 12]).any() and not (f == 0 and (rows == 20).any()) and not (f == 1 and (cols == 11).any())
    exact = np.stack([K.chi2_cost(ta, tb[f].contiguous()).cpu().numpy() for f in range(frames)]) - u[:, :, None] - v[:, None, :]
    thr = np.quantile(exact, 0.01)
    below = S.unary_distance_below(a, (b[0], b[1]), thr, row_offsets=u, col_offsets=v)
    whole = K.hellinger_list(ta, tb, tu, tv, np.inf, cap=n * m)
    for f, (rows, cols, lower) in enumerate(below):
        assert all(isinstance(x, np.ndarray) for x in below[f]) and rows.dtype == np.int32 and lower.dtype == np.float64
        assert np.array_equal(lower, whole[f][2].cpu().numpy().reshape(n, m)[rows, cols] - delta)
        assert np.isin(np.flatnonzero(exact[f] <= thr), rows.astype(np.int64) * m + cols).all() and rows.size < n * m
