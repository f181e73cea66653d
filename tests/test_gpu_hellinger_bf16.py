"""hellinger_select(precision='bf16x3') (csrc/pm_hellinger_bf16.hip: hl_select_bf16_kernel, the priced per-row top-k of the Hellinger
lower bound on the bf16 matrix path) against the float64 NumPy bound, the exact costs of chi2_cost, and through the public calls.
Contract assertions under the path's own delta; panels of P = 256 rows, tiles of T = 128 columns."""
import types

import numpy as np
import pytest

from test_gpu_hellinger import reference_bound, synthetic_case

pytestmark = pytest.mark.gpu
PREC = "bf16x3"


@pytest.fixture(scope="module")
def g():
    import torch
    from platymatch_amd import _kernels as K, _native as nat
    nat.load()
    assert torch.cuda.is_available()
    return types.SimpleNamespace(K=K, nat=nat, delta=K.hellinger_delta(PREC))


def select(g, ta, tb, v, k, split, info=None):
    out = g.K.hellinger_select(ta, tb, v=None if v is None else g.nat.to_dev(v), k=k, split=split, info=info, precision=PREC)
    return tuple(x.cpu().numpy() for x in out)


def exact_costs(g, ta, tb):
    return np.stack([g.K.chi2_cost(ta, tb[f].contiguous()).cpu().numpy() for f in range(tb.shape[0])])


# (N, M, frames, k, prices): N = 1, P + 2, 2P + 1;  M = k - 3 (tails), T + 72, 3T + 5 (ragged last tile);  both CAP instances
@pytest.mark.parametrize("n,m,frames,k,kind", [(1, 200, 1, 16, None), (258, 389, 4, 32, "random"), (513, 13, 1, 16, "nonfinite"),
                                               (258, 200, 4, 1, "random"), (1, 389, 1, 32, "nonfinite"), (513, 29, 4, 32, None)])
def test_contract_against_the_float64_bound_and_the_exact_costs(g, n, m, frames, k, kind):
    a, b = synthetic_case(n, m, frames, 5)
    ref = np.stack([reference_bound(a, bf) for bf in b])
    v = None if kind is None else np.random.default_rng(7).uniform(0.0, 0.5, (frames, m))
    if kind == "nonfinite":
        v[0, 1], v[-1, m // 2] = np.nan, np.inf
    fin = np.ones((frames, m), bool) if v is None else np.isfinite(v)
    v0 = np.zeros((frames, m)) if v is None else np.where(fin, v, 0.0)
    ta, tb, delta, info = g.nat.to_dev(a), g.nat.to_dev(b), g.delta, {}
    exact = exact_costs(g, ta, tb)
    cols, bound = select(g, ta, tb, v, k, 1, info)
    assert info["nonfinite"] == 0 and cols.shape == bound.shape == (frames, n, k)
    listed = np.broadcast_to((np.arange(k) < np.minimum(fin.sum(1), k)[:, None])[:, None, :], cols.shape)
    assert np.array_equal(cols >= 0, listed) and (cols < m).all() and np.isposinf(bound[~listed]).all()
    idx = np.where(listed, cols, 0).astype(np.int64)
    fi, ni, ri = np.nonzero(listed)
    sel = np.zeros(ref.shape, bool)
    sel[fi, ni, cols[fi, ni, ri]] = True
    assert sel.sum() == listed.sum() and fin[fi, cols[fi, ni, ri]].all()                 # distinct, no non-finite price
    err = np.abs(bound - np.take_along_axis(ref, idx, axis=2))[listed].max()
    print("n=%d m=%d frames=%d k=%d %s: largest |bound - L_float64| = %.3g (delta %.3g)" % (n, m, frames, k, kind, err, delta))
    assert err <= delta
    key = np.where(listed, bound - np.take_along_axis(v0[:, None, :], idx, axis=2), np.inf)
    up = key[:, :, 1:] > key[:, :, :-1]
    assert (up | ((key[:, :, 1:] == key[:, :, :-1]) & ((cols[:, :, 1:] > cols[:, :, :-1]) | ~listed[:, :, 1:]))).all()
    unlisted, kth = fin[:, None, :] & ~sel, key[:, :, k - 1:k]
    red = exact - v0[:, None, :]
    assert ((ref - v0[:, None, :]) >= kth - delta)[unlisted].all() and (red >= kth - delta)[unlisted].all()
    assert (np.take_along_axis(red, idx, axis=2) >= key - delta)[listed].all()
    for split in (2, 3):
        c2, b2 = select(g, ta, tb, v, k, split)
        assert np.array_equal(c2, cols) and np.array_equal(b2.view(np.int64), bound.view(np.int64)), split


def test_edge_rows(g):
    a, b = synthetic_case(70, 90, 2, 3)
    b[0, 20] = a[7]                                  # identical rows: bound 0
    a[3], b[0, 33] = np.eye(360)[17], np.eye(360)[17]          # a one-hot pair: sqrt = 1 exactly
    a[9, 0] = np.nan
    b[1, 11, 5] = -1.0
    info = {}
    cols, bound = select(g, g.nat.to_dev(a), g.nat.to_dev(b), None, 4, 0, info)
    assert info["nonfinite"] == 1
    assert (cols[:, 9] == -1).all() and np.isnan(bound[:, 9]).all()
    assert not (cols[1] == 11).any() and np.isfinite(np.delete(bound, 9, axis=1)).all()
    for row, col in ((7, 20), (3, 33)):
        assert cols[0, row, 0] == col and abs(bound[0, row, 0]) <= g.delta


def test_the_public_calls(g):
    from platymatch_amd.estimate_transform import shape_context as S
    a, b = synthetic_case(70, 90, 2, 10)
    v = np.random.default_rng(7).uniform(0.0, 0.5, (2, 90))
    exact = exact_costs(g, g.nat.to_dev(a), g.nat.to_dev(b))
    cols, dist, proven = S.unary_distance_nearest(a, tuple(b), k=8, candidates=32, precision=PREC, col_offsets=v)
    assert isinstance(cols, np.ndarray) and (cols >= 0).all()
    assert np.array_equal(dist.view(np.int64), np.take_along_axis(exact, cols.astype(np.int64), axis=2).view(np.int64))
    first = np.argsort(exact - v[:, None, :], axis=2, kind="stable")[:, :, :8]
    assert (proven >= 0).all() and (proven <= 8).all() and ((cols == first) | (np.arange(8) >= proven[:, :, None])).all()
    cc, lower = S.unary_distance_candidates(a, tuple(b), k=16, precision=PREC)
    idx = cc.astype(np.int64)
    assert (lower <= np.take_along_axis(exact, idx, axis=2)).all()
    rest = np.ones(exact.shape, bool)
    np.put_along_axis(rest, idx, False, axis=2)
    assert (exact >= lower[:, :, -1:])[rest].all()


def test_bad_arguments(g):
    a, b = synthetic_case(4, 40, 1, 1)
    ta, tb = g.nat.to_dev(a), g.nat.to_dev(b)
    assert g.nat.load().pm_hellinger_select_bf16_workspace(4, 40, 1, 33) == 0
    with pytest.raises(ValueError):
        g.K.hellinger_select(ta, tb, k=33, precision=PREC)
    with pytest.raises(ValueError):
        g.K.hellinger_select(ta, tb, k=8, precision="f16")
    with pytest.raises(ValueError):
        g.K.hellinger_delta("f16")
