"""chi2_select_exact (csrc/pm_chi2_select.hip: hellinger_select's lists rescored exactly, ordered by exact reduced cost, with the
number of proven leading entries) against plain NumPy float64: C = 0.5 sum_q d*d/(a+b) accumulated over q = 0..359 as whole-matrix
operations (zeros of b set to 1e-300; IEEE division and index order make that the exact build's bits), the twin the same loop in
rolled order.  The candidates are what hellinger_select returns and T is formed from ITS bound bits: every assertion is an equality."""
import functools
import types

import numpy as np
import pytest

from test_gpu_hellinger import reference_bound, synthetic_case
from test_gpu_hellinger_select import prices

pytestmark = pytest.mark.gpu
bits = lambda x: np.ascontiguousarray(x).view(np.int64)  # noqa: E731
ROLLED = [12 * (q // 12) + (q % 12 + 6) % 12 for q in range(360)]


@pytest.fixture(scope="module")
def g():
    import torch
    from platymatch_amd import _kernels as K, _native as nat
    nat.load()
    assert torch.cuda.is_available()
    return types.SimpleNamespace(K=K, nat=nat, t=torch)


@functools.lru_cache(maxsize=None)
def host_case(n, m, frames, seed):
    """descriptors a [N, 360], b [F, M, 360] and the reference (C, twin) [F, N, M]"""
    a, b = synthetic_case(n, m, frames, seed)
    bb = np.where(b == 0.0, 1e-300, b)

    def total(order):
        s = np.zeros((frames, n, m))
        for q in order:
            d = a[None, :, None, q] - bb[:, None, :, q]
            s = s + d * d / (a[None, :, None, q] + bb[:, None, :, q])
        return 0.5 * s
    return a, b, total(range(360)), total(ROLLED)


def finite_prices(v, frames, m):
    """(prices with 0 where there are none or they are not finite [F, M], which columns can be listed [F, M])"""
    if v is None:
        return np.zeros((frames, m)), np.ones((frames, m), bool)
    return np.where(np.isfinite(v), v, 0.0), np.isfinite(v)


def expected(C, Ct, v, cand, bound, k, delta):
    """what the kernel must return for these candidate lists: (cols, cost, twin, proven)"""
    v0, _ = finite_prices(v, C.shape[0], C.shape[2])
    ok = cand >= 0
    idx = np.where(ok, cand, 0).astype(np.int64)
    vc = np.take_along_axis(v0[:, None, :], idx, axis=2)
    cost, twin = (np.where(ok, np.take_along_axis(X, idx, axis=2), np.inf) for X in (C, Ct))
    key = np.where(ok, cost - vc, np.inf)
    order = np.lexsort((np.where(ok, cand, 2 ** 31 - 1), key), axis=2)[:, :, :k]
    T = np.where(ok[:, :, -1], (bound[:, :, -1] - vc[:, :, -1]) - delta, np.inf)
    proven = (np.take_along_axis(key, order, axis=2) < T[:, :, None]).sum(2)
    return tuple(np.take_along_axis(X, order, axis=2) for X in (np.where(ok, cand, -1), cost, twin)) + (proven,)


def reference_proven(a, b, C, Ct, v, kc, k, delta):
    """the proof counts on the reference alone: the lists of the float64 bound in place of the device's"""
    v0, fin = finite_prices(v, *C.shape[::2])
    L = np.stack([reference_bound(a, bf) for bf in b])
    keys = np.where(fin[:, None, :], L - v0[:, None, :], np.inf)
    cand = np.argsort(keys, axis=2, kind="stable")[:, :, :kc]
    return expected(C, Ct, v, cand, np.take_along_axis(L, cand, axis=2), k, delta)[3]


def run(g, a, b, v, kc, k, cand=None, info=None):
    """-> (candidates, bound, cols, cost, proven, twin) as NumPy arrays"""
    dev = g.nat.to_dev
    ta, tb, tv = dev(a), dev(b), None if v is None else dev(v)
    lists = g.K.hellinger_select(ta, tb, v=tv, k=kc) if cand is None else tuple(dev(x, dtype=t) for x, t in zip(cand, (g.t.int32, g.t.float64)))
    out = g.K.chi2_select_exact(ta, tb, lists[0], lists[1], v=tv, k=k, twin=True, info=info)
    return tuple(x.cpu().numpy() for x in lists + out)


# (N, M, frames, kc, k, seed): four units per wave and a ragged row block; k = kc, one frame, one row past a block; two units per
# wave; one unit per wave; kc below the smallest instance (padded lanes); M < kc (tails, T = +inf); kc = k = 1.  The seeds are
# test_gpu_hellinger_select's; PRICE_SEEDS, case by case, the first for which the first five cases have, on the reference alone
# under prices('random'), a unit with proven > 0 and a unit with proven < k (without prices they have both as they are).
CASES = [(70, 90, 4, 16, 8, 10), (129, 257, 1, 16, 16, 16), (70, 200, 1, 32, 8, 2), (5, 3000, 4, 64, 16, 44), (33, 65, 2, 8, 5, 1),
         (40, 9, 1, 16, 16, 1), (33, 65, 2, 1, 1, 1)]
PRICE_SEEDS = (0, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("kind", [None, "random", "ramp", "nonfinite"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_rescored_lists_against_the_float64_reference(g, case, kind):
    n, m, frames, kc, k, seed = CASES[case]
    a, b, C, Ct = host_case(n, m, frames, seed)
    v, delta = None if kind is None else prices(kind, frames, m, PRICE_SEEDS[case]), g.K.hellinger_delta()
    if case < 5 and kind in (None, "random"):      # on the reference alone: otherwise the proof count is not tested
        pr = reference_proven(a, b, C, Ct, v, kc, k, delta)
        assert (pr > 0).any() and (pr < k).any(), "choose another price seed"
    info = {}
    cand, bound, cols, cost, proven, twin = run(g, a, b, v, kc, k, info=info)
    assert info["status"] == 0 and cols.dtype == proven.dtype == np.int32 and cols.shape == (frames, n, k) and proven.shape == (frames, n)
    want = expected(C, Ct, v, cand, bound, k, delta)
    print("case %d %s: proven %d..%d of k = %d" % (case, kind, proven.min(), proven.max(), k))
    assert np.array_equal(cols, want[0]) and np.array_equal(proven, want[3])
    assert np.array_equal(bits(cost), bits(want[1])) and np.array_equal(bits(twin), bits(want[2]))
    assert np.isposinf(cost[cols < 0]).all() and np.isposinf(twin[cols < 0]).all() and ((cols >= 0).sum(2) >= proven).all()
    # the proven entries are the head of the row of the full exact reduced matrix, ordered by (value, column)
    v0, fin = finite_prices(v, frames, m)
    head = np.argsort(np.where(fin[:, None, :], C - v0[:, None, :], np.inf), axis=2, kind="stable")[:, :, :k]
    kk = head.shape[2]
    assert (cols[:, :, :kk] == head)[np.arange(kk) < proven[:, :, None]].all()
    if m <= kc:
        assert (proven == np.minimum(k, fin.sum(1))[:, None]).all()
    elif kind == "ramp":
        assert (proven == min(k, kc - 1)).all()
    if kind == "nonfinite":
        assert not (cols[0] == 1).any() and not (cols[-1] == m // 2).any()


def test_the_bits_of_the_exact_kernels(g):
    """fixed frames 2..4 as the phi permutations of frame 1: cost = chi2_cost's entries, twin = chi2_entries' rolled output"""
    n, m, _, kc, _, seed = CASES[0]
    a, b1 = synthetic_case(n, m, 1, seed)
    maps = [lambda q: q, lambda q: (q + 6) % 12, lambda q: 11 - q, lambda q: (5 - q) % 12]
    b = np.stack([b1[0][:, [12 * (q // 12) + fn(q % 12) for q in range(360)]] for fn in maps])
    _, _, cols, cost, _, twin = run(g, a, b, None, kc, kc)
    ta, tb = g.nat.to_dev(a), g.nat.to_dev(b)
    rows = np.repeat(np.arange(n), kc)
    for f in range(4):
        full = g.K.chi2_cost(ta, tb[f].contiguous()).cpu().numpy()
        nat, rol = (x.cpu().numpy() for x in g.K.chi2_entries(ta, tb[0].contiguous(), f, rows, cols[f].ravel()))
        assert np.array_equal(bits(cost[f]), bits(full[rows, cols[f].ravel()].reshape(n, kc)))
        assert np.array_equal(bits(cost[f].ravel()), bits(nat)) and np.array_equal(bits(twin[f].ravel()), bits(rol))


def test_python_surfaces_and_error_paths(g):
    from platymatch_amd.estimate_transform import shape_context as S
    n, m, frames, kc, k, seed = CASES[0]
    a, b, C, Ct = host_case(n, m, frames, seed)
    dev, delta = g.nat.to_dev, g.K.hellinger_delta()
    for v in (None, prices("random", frames, m, PRICE_SEEDS[0])):
        _, _, cols, cost, proven, twin = run(g, a, b, v, kc, k)
        near = g.K.chi2_nearest(dev(a), dev(b), v=None if v is None else dev(v), k=k, candidates=kc, twin=True)
        pub = S.unary_distance_nearest(a, tuple(b), k=k, candidates=kc, col_offsets=v, twin=True)
        for got in (tuple(x.cpu().numpy() for x in near), pub):
            assert all(isinstance(x, np.ndarray) for x in got) and len(got) == 4
            assert np.array_equal(got[0], cols) and np.array_equal(got[2], proven)
            assert np.array_equal(bits(got[1]), bits(cost)) and np.array_equal(bits(got[3]), bits(twin))
    # a moving row holding a NaN
    a2, info = a.copy(), {}
    a2[3, 5] = np.nan
    _, _, cols, cost, proven, twin = run(g, a2, b, None, kc, k, info=info)
    assert info["status"] == 1 and (cols[:, 3] == -1).all() and np.isnan(cost[:, 3]).all() and np.isnan(twin[:, 3]).all() and (proven[:, 3] == 0).all()
    # a candidate index of M: status bit 1, treated as absent
    cand, bound = run(g, a, b, None, kc, k)[:2]
    cand[0, 2, 1], cand[1, 5, 0] = m, -7
    got = run(g, a, b, None, kc, k, cand=(cand, bound), info=info)
    want = expected(C, Ct, None, np.where((cand >= 0) & (cand < m), cand, -1), bound, k, delta)
    assert info["status"] == 2 and np.array_equal(got[2], want[0]) and np.array_equal(bits(got[3]), bits(want[1])) and np.array_equal(got[4], want[3])
