"""hellinger_topk (csrc/pm_hellinger.hip: the Hellinger lower bound of the chi-square cost on the matrix cores, fused with a
per-row top-k) against the whole bound matrix in float64 NumPy and against the exact costs of chi2_cost."""
import numpy as np
import pytest

from conftest import synth_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import torch
    from platymatch_amd import _kernels as K, _native as nat, pipeline as P
    nat.load()
    assert torch.cuda.is_available()

    class G:
        pass
    G.K, G.nat, G.P, G.t = K, nat, P, torch
    return G


def multinomial_descriptors(rng, n, active):
    """count / total rows as get_shape_context normalises them: totals of 5..400, each row's own distribution over 40 of the 360
    bins (the bounds of a row then spread over most of [0, 1], which leaves gaps of more than 2 delta at its k-th value)"""
    rows = []
    for total in rng.integers(5, 401, n):
        p = np.zeros(360)
        p[active] = rng.dirichlet(0.3 * np.ones(active.size))
        rows.append(rng.multinomial(total, p) / total)
    return np.stack(rows)


def reference_bound(a, b):
    return 0.5 * (a.sum(1)[:, None] + b.sum(1)[None, :]) - np.sqrt(a) @ np.sqrt(b).T


def synthetic_case(n, m, frames, seed):
    rng = np.random.default_rng(seed)
    active = rng.choice(360, 40, replace=False)
    return multinomial_descriptors(rng, n, active), np.stack([multinomial_descriptors(rng, m, active) for _ in range(frames)])


def check_lists(g, a, b, k, splits, delta):
    """assertions (a)-(f) of one case: a [N, 360], b [F, M, 360] host arrays; every split against split 1"""
    n, (frames, m) = a.shape[0], b.shape[:2]
    ta, tb = g.nat.to_dev(a), g.nat.to_dev(b)
    ref = np.stack([reference_bound(a, b[f]) for f in range(frames)])
    exact = np.stack([g.K.chi2_cost(ta, tb[f].contiguous()).cpu().numpy() for f in range(frames)])
    order = np.sort(ref, axis=2)
    if m > k:       # the reference alone separates the k-th from the (k+1)-th value of every row: the listed SET is then determined
        assert (order[:, :, k] - order[:, :, k - 1]).min() > 2 * delta, "choose another seed: %g" % (order[:, :, k] - order[:, :, k - 1]).min()
    cols, bound = (x.cpu().numpy() for x in g.K.hellinger_topk(ta, tb, k=k, split=1))
    assert cols.shape == bound.shape == (frames, n, k) and cols.dtype == np.int32 and bound.dtype == np.float64
    listed = min(k, m)
    idx = cols[:, :, :listed].astype(np.int64)
    assert (idx >= 0).all() and (idx < m).all()                                                                  # (a)
    assert (cols[:, :, listed:] == -1).all() and np.isposinf(bound[:, :, listed:]).all()
    assert all(len(set(idx[f, i])) == listed for f in range(frames) for i in range(n))
    dev = np.abs(bound[:, :, :listed] - np.take_along_axis(ref, idx, axis=2)).max()
    print("n=%d m=%d frames=%d k=%d: largest |bound - L_float64| = %.3g (delta %.3g)" % (n, m, frames, k, dev, delta))
    assert dev <= delta                                                                                          # (b)
    assert (np.diff(bound[:, :, :listed], axis=2) >= 0).all()                                                    # (c)
    unlisted = np.ones(ref.shape, bool)
    np.put_along_axis(unlisted, idx, False, axis=2)
    kth = bound[:, :, listed - 1:listed]
    assert (ref >= kth - delta)[unlisted].all()                                                                  # (d)
    if m > k:
        assert (np.sort(idx, axis=2) == np.sort(np.argsort(ref, axis=2, kind="stable")[:, :, :k], axis=2)).all()
    assert (np.take_along_axis(exact, idx, axis=2) >= bound[:, :, :listed] - delta).all()                        # (f)
    assert (exact >= kth - delta)[unlisted].all()
    for split in splits:                                                                                         # (e)
        c2, b2 = (x.cpu().numpy() for x in g.K.hellinger_topk(ta, tb, k=k, split=split))
        assert np.array_equal(c2, cols) and np.array_equal(b2.view(np.int64), bound.view(np.int64)), split


# (N, M, frames, k, splits, seed): ragged tile edges; k = 1; fewer columns than k; few rows against many columns with the split
# automatic and forced; one row more than a row block and one column more than two tiles.  The seeds are the first for which the
# float64 reference separates every row's k-th and (k+1)-th value by more than 2 delta.
CASES = [(70, 90, 4, 16, (0,), 10), (33, 65, 2, 1, (0,), 1), (40, 9, 1, 16, (0, 3), 1), (5, 3000, 4, 64, (0, 7), 44),
         (65, 129, 1, 16, (0, 2), 1)]


@pytest.mark.parametrize("n,m,frames,k,splits,seed", CASES)
def test_lists_against_the_float64_bound_and_the_exact_costs(g, n, m, frames, k, splits, seed):
    a, b = synthetic_case(n, m, frames, seed)
    check_lists(g, a, b, k, splits, g.K.hellinger_delta())


SYNTH_SEED = 14          # the first seed whose 24 x 4 reference lists keep the 8th and 9th values more than 2 delta apart


def test_lists_of_shape_context_descriptors(g):
    mv, fx, _ = synth_pair(200, SYNTH_SEED)
    be = g.P.GpuBackend()
    sc_m, sc_f, _ = g.P.build_descriptors(be, be.cloud(mv), be.cloud(fx))
    check_lists(g, sc_m[0, :24].cpu().numpy(), sc_f.cpu().numpy(), 8, (0, 2), g.K.hellinger_delta())


def test_ties_nonfinite_rows_and_the_public_call(g):
    from platymatch_amd.estimate_transform import shape_context as S
    a, b = synthetic_case(70, 90, 2, 3)
    b[0, 50] = b[0, 20] = a[7]                      # two bit-identical fixed rows, at bound 0 for moving row 7
    b[1, 11, 5] = np.nan
    a[9, 0] = np.nan
    a[12, 3] = -1.0
    delta, info = g.K.hellinger_delta(), {}
    cols, bound = (x.cpu().numpy() for x in g.K.hellinger_topk(g.nat.to_dev(a), g.nat.to_dev(b), k=4, info=info))
    assert info["nonfinite"] == 1
    assert list(cols[0, 7, :2]) == [20, 50] and bound[0, 7, 0] == bound[0, 7, 1] and abs(bound[0, 7, 0]) <= delta
    for bad in (9, 12):
        assert (cols[:, bad] == -1).all() and np.isnan(bound[:, bad]).all()
    assert not (cols[1] == 11).any() and np.isfinite(bound[:, 8]).all()
    clean = np.delete(a, (9, 12), axis=0)
    g.K.hellinger_topk(g.nat.to_dev(clean), g.nat.to_dev(b[0]), k=4, info=info)
    assert info["nonfinite"] == 0
    pc, lower = S.unary_distance_candidates(a, (b[0], b[1]), k=4)
    assert isinstance(pc, np.ndarray) and isinstance(lower, np.ndarray) and np.array_equal(pc, cols)
    assert np.array_equal(lower, bound - delta, equal_nan=True)
