"""The leaf-wise device grower (csrc/gbdt_lossguide.hip) against its host twin mifx_gbdt_grow_fixed_lossguide_stats:
all six tree arrays, the node count, leaf_of_row, gain and cover bit for bit, for any launch geometry; then
XGB*(device="gpu", grow_policy="lossguide") against the host twin model."""
import numpy as np
import pytest

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, XGBRegressor, xgb

pytestmark = pytest.mark.gpu

NAMES = C.NAMES + ("gain", "cover")


def twin(bins, nbins, g, h, depth, leaves, rows=None, mask=None, mcw=1.0):
    """(feature, split_bin, default_left, left, right, value, leaf_of_row, gain, cover) of the host twin."""
    (f, n), cap, p = bins.shape, 2 * leaves - 1, xgb._p
    fe, sb, le, ri = (np.empty(cap, np.int32) for _ in range(4))
    dl, val, leaf = np.empty(cap, np.uint8), np.empty(cap, np.float64), np.empty(n, np.int32)
    gain, cover = np.empty(cap, np.float64), np.empty(cap, np.float64)
    cnt = xgb._lib().mifx_gbdt_grow_fixed_lossguide_stats(
        p(bins, xgb._U16), n, f, p(nbins, xgb._I), p(g, xgb._F), p(h, xgb._F), depth, leaves, mcw, 1.0, 0.0, 0.3, 1, cap,
        p(fe, xgb._I), p(sb, xgb._I), p(dl, xgb._U8), p(le, xgb._I), p(ri, xgb._I), p(val, xgb._D), p(leaf, xgb._I),
        None if rows is None else p(rows, xgb._I), 0 if rows is None else len(rows),
        None if mask is None else p(mask, xgb._U8), p(gain, xgb._D), p(cover, xgb._D))
    assert cnt > 0
    return tuple(a[:cnt].copy() for a in (fe, sb, dl, le, ri, val)) + (leaf,) + (gain[:cnt].copy(), cover[:cnt].copy())


def same(got, want, what=""):
    assert len(got[0]) == len(want[0]), f"{what}: node count"
    for name, x, y in zip(NAMES, got, want):
        assert np.array_equal(x, y), f"{what}: {name} differs"


def grow(*a, **kw):
    from mifx.ops import gbdt_gpu

    return gbdt_gpu.grow_lossguide_numpy(*a, **kw)


def depth_of(tree):
    d = np.zeros(len(tree[0]), int)
    for k in np.flatnonzero(tree[0] >= 0):  # parents come before their children
        d[tree[3][k]] = d[tree[4][k]] = d[k] + 1
    return d.max()


GEOMETRIES = [{}, dict(_rows_per_wg=64, _feat_tile=4, _grid_x=3), dict(_rows_per_wg=256, _feat_tile=12, _grid_x=512)]


@pytest.mark.parametrize("n,f,depth,leaves", [(1, 3, 0, 4), (2, 3, 0, 4), (300, 3, 0, 2), (300, 3, 0, 3), (300, 3, 0, 8),
                                               (300, 3, 2, 8), (5000, 13, 0, 32), (5000, 13, 4, 4096)])
def test_device_tree_equals_host_twin(n, f, depth, leaves):
    bins, nbins = C.make_bins(n, f, seed=n + leaves)
    assert n < 5000 or {1, 256} <= set(nbins.tolist())  # 13 features: two feature tiles, every kind of bin count
    g, h = C.float_grads(n, n)
    want = twin(bins, nbins, g, h, depth, leaves)
    assert n < 300 or (len(want[0]) == 2 * leaves - 1 if depth == 0 else depth_of(want) == depth)
    for geo in GEOMETRIES if n == 5000 else GEOMETRIES[:2]:  # 64 rows per chunk, 3 workgroups: a node spans many chunks
        same(grow(bins, nbins, g, h, depth, leaves, **geo), want, f"{geo}")


def test_out_of_range_bins_are_missing():
    bins, nbins = C.make_bins(1000, 3, seed=9)
    g, h = C.float_grads(1000, 9)
    want = twin(bins, nbins, g, h, 0, 16)
    odd = bins.copy()
    odd[odd == 0xFFFF] = np.resize(np.array([256, 300, 0xFFFE, 5000], np.uint16), (odd == 0xFFFF).sum())
    same(twin(odd, nbins, g, h, 0, 16), want, "host")
    same(grow(odd, nbins, g, h, 0, 16), want, "device")


def _walk(bins, nbins, tree, i):
    fe, sb, dl, le, ri, val = tree[:6]
    k = 0
    while fe[k] >= 0:
        b = int(bins[fe[k], i])
        k = (le[k] if b <= sb[k] else ri[k]) if b < nbins[fe[k]] else (le[k] if dl[k] else ri[k])
    return val[k]


def test_sampled_rows_feature_mask_and_margins():
    n, f, seed = 5000, 11, 21
    bins, nbins = C.make_bins(n, f, seed)
    g, h = C.float_grads(n, seed)
    mask = xgb.level_mask(seed, 2, f, 1, 0.5, 1.0)[0]
    rows = xgb.sample_rows(seed, 2, 0.5, n)
    want = twin(bins, nbins, g, h, 0, 24, rows, mask)
    assert (want[6] < 0).sum() > 2000 and set(want[0][want[0] >= 0]) <= set(np.flatnonzero(mask))
    start = np.random.default_rng(1).normal(size=n)
    for geo in GEOMETRIES[:2]:
        got = grow(bins, nbins, g, h, 0, 24, subsample=0.5, seed=seed, round=2, feature_mask=mask, margin=start, **geo)
        same(got[:9], want, f"{geo}")
        assert np.array_equal(got[9], start + np.array([_walk(bins, nbins, want, i) for i in range(n)]))


def test_staircase_chain_deeper_than_twelve():
    """One feature of 40 steps whose gradient triples from step to step: every split peels the top step off, so the tree is a
    chain; max_depth = 0 lets it pass depth 12, and the walk of the rows outside the sample follows it to the end."""
    n = 4000
    step = (np.arange(n) % 40).astype(np.uint16)
    bins, nbins = step[None, :].copy(), np.array([40], np.int32)
    g, h = (-(3.0 ** step.astype(np.float64))).astype(np.float32), np.ones(n, np.float32)
    rows = xgb.sample_rows(5, 0, 0.5, n)
    want = twin(bins, nbins, g, h, 0, 30, rows)
    assert depth_of(want) == 29 and len(want[0]) == 59  # a pure chain
    got = grow(bins, nbins, g, h, 0, 30, subsample=0.5, seed=5, round=0, margin=np.zeros(n))
    same(got[:9], want)
    assert np.array_equal(got[9], np.array([_walk(bins, nbins, want, i) for i in range(n)]))


def test_ties_expand_the_lower_id_first():
    r = np.random.default_rng(3)
    half = r.integers(0, 8, (2, 200)).astype(np.uint16)
    bins = np.concatenate([np.r_[np.zeros((1, 200), np.uint16), half], np.r_[np.ones((1, 200), np.uint16), half]], 1)
    nbins = np.array([2, 8, 8], np.int32)
    g1 = (20.0 + 3.0 * half[0] + r.integers(-8, 9, 200) / 4.0).astype(np.float32)
    g, h = np.concatenate([g1, -g1]), np.ones(400, np.float32)
    full = twin(bins, nbins, g, h, 2, 4)
    assert full[0][0] == 0 and full[7][1] == full[7][2] > 0  # both children of the root: the same gain
    want = twin(bins, nbins, g, h, 0, 3)
    assert want[0][1] >= 0 and want[0][2] < 0
    same(grow(bins, nbins, g, h, 0, 3), want)


def _data(classes=0):
    r = np.random.default_rng(8)
    X = r.normal(size=(900, 6))
    y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.1, 900)
    X[r.random(X.shape) < 0.1] = np.nan
    if classes:
        y = np.digitize(y, np.quantile(y, np.arange(1, classes) / classes))
    return X[:600], y[:600], X[600:], y[600:]


def _same_trees(a, b, trees):
    for t in range(trees):
        for u, v in zip(a._trees[t] + a._node_stats[t], b._trees[t] + b._node_stats[t]):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"tree {t}"


def test_regressor_equals_host_twin_model():
    X, y, Xe, ye = _data()
    kw = dict(n_estimators=5, grow_policy="lossguide", max_leaves=8, max_depth=0, subsample=0.7, colsample_bytree=0.7)
    a = XGBRegressor(device="gpu", **kw).fit(X, y, eval_set=[(Xe, ye)])
    b = XGBRegressor(device="cpu", fixed_point=True, **kw).fit(X, y, eval_set=[(Xe, ye)])
    assert a.n_trees_ == b.n_trees_ == 5 and all(len(t[0]) == 15 for t in a._trees)
    _same_trees(a, b, 5)
    assert a.evals_result_ == b.evals_result_ and a._base_margin == b._base_margin
    assert np.array_equal(a.predict(Xe), b.predict(Xe))


@pytest.mark.parametrize("classes", [2, 3])
def test_classifier_first_round_equals_host_twin_and_fits_repeat(classes):
    """As for depth-wise growth: the first round's gradients come from one shared margin and are exact, so its trees
    are the twin's bit for bit; later rounds see exp's last bit. Two device fits are equal throughout."""
    X, y, Xe, ye = _data(classes)
    kw = dict(n_estimators=5, grow_policy="lossguide", max_leaves=8, base_score=0.5)
    a, a2 = (XGBClassifier(device="gpu", **kw).fit(X, y, eval_set=[(Xe, ye)]) for _ in range(2))
    b = XGBClassifier(device="cpu", fixed_point=True, **kw).fit(X, y, eval_set=[(Xe, ye)])
    K = a._num_class()
    assert a.n_trees_ == b.n_trees_ == 5 * K and K == (1 if classes == 2 else 3)
    _same_trees(a, b, K)
    _same_trees(a, a2, 5 * K)
    name = a._metric_name()
    assert a.evals_result_["validation_0"][name][0] == b.evals_result_["validation_0"][name][0]
    assert a.evals_result_ == a2.evals_result_ and a.evals_result_["validation_0"][name][-1] < np.log(classes)


def test_device_limits_raise_before_any_launch():
    X, y = np.zeros((8, 2)), np.arange(8.0)
    for kw in (dict(max_leaves=4097), dict(max_leaves=8, max_depth=13), dict(max_leaves=8, max_bins=257)):
        with pytest.raises(ValueError, match="device='gpu' supports"):
            XGBRegressor(device="gpu", grow_policy="lossguide", **kw).fit(X, y)
