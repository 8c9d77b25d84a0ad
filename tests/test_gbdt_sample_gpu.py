"""Stochastic boosting and instance weights on the device learner (csrc/gbdt_gpu.hip) against the host twin
mifx_gbdt_grow_fixed_ex: exact equality of every tree array and of leaf_of_row with its -1s, for any launch geometry;
the weighted gradient kernel; the margins of rows outside the sample; XGB*(device="gpu") end to end."""
import numpy as np
import pytest
import torch

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, XGBRegressor, xgb
from mifx.gbdt import sample as S
from test_gbdt_sample_cpu import grow_ex

pytestmark = pytest.mark.gpu

NS = [1, 2, 63, 65, 257, 5000]


def _G():
    from mifx.ops import gbdt_gpu

    return gbdt_gpu


def _rounds(seed, rate, n):
    """Two rounds for a shape: for n <= 2 the first with an empty and the first with a non-empty sample."""
    if n > 2:
        return [0, 1]
    sizes = [int(S.row_mask(seed, r, rate, n).sum()) for r in range(64)]
    return [sizes.index(0), next(r for r, s in enumerate(sizes) if s > 0)]


def _twin(bins, nbins, g, h, depth, seed, rnd, rate, mask=None, mcw=1.0):
    rows = xgb.sample_rows(seed, rnd, rate, bins.shape[1]) if rate < 1.0 else None
    return grow_ex(bins, nbins, g, h, depth, mcw, fixed=True, rows=rows, mask=mask)


@pytest.mark.parametrize("n,f", [(n, f) for n in NS for f in C.FS])
def test_device_grower_equals_host_twin_on_sampled_rows(n, f):
    G = _G()
    seed = n * 31 + f
    bins, nbins = C.make_bins(n, f, seed)
    g, h = C.float_grads(n, seed)
    gb, hb = C.float_grads(n, seed, 1e30)
    empty = 0
    for depth in (0, 3, 6):
        bst = G.Booster(bins, nbins, depth, torch.device("cuda", 0))
        for rate in (0.5, 0.1):
            for rnd in _rounds(seed, rate, n):
                got = G.grow_numpy(bins, nbins, g, h, depth, subsample=rate, seed=seed, round=rnd, _booster=bst)
                want = _twin(bins, nbins, g, h, depth, seed, rnd, rate)
                C.assert_same_tree(got, want, f"depth {depth} rate {rate} round {rnd}")
                if (want[6] < 0).all():
                    empty += 1
                    assert len(got[0]) == 1 and got[5][0] == 0.0 and not np.signbit(got[5][0])
        got = G.grow_numpy(bins, nbins, gb, hb, depth, subsample=0.5, seed=seed, round=1, _booster=bst)
        C.assert_same_tree(got, _twin(bins, nbins, gb, hb, depth, seed, 1, 0.5), f"1e30 depth {depth}")
        if f >= 3 and depth > 0:  # per-level masks, with and without row sampling
            mask = S.level_mask(seed, depth, f, depth, 0.7, 0.5)
            for rate in (1.0, 0.5):
                got = G.grow_numpy(bins, nbins, g, h, depth, 0.0, subsample=rate, seed=seed, round=3, level_mask=mask,
                                   _booster=bst)
                want = _twin(bins, nbins, g, h, depth, seed, 3, rate, mask, mcw=0.0)
                C.assert_same_tree(got, want, f"mask depth {depth} rate {rate}")
    if n <= 2:
        assert empty >= 3  # every depth met an empty sample


def test_sampled_grower_geometry_independent():
    G = _G()
    bins, nbins = C.make_bins(5000, 11, seed=4)
    g, h = C.float_grads(5000, 4)
    mask = S.level_mask(4, 0, 11, 6, 1.0, 0.5)
    kw = dict(subsample=0.5, seed=4, round=2, level_mask=mask)
    ref = G.grow_numpy(bins, nbins, g, h, 6, **kw)
    assert len(ref[0]) > 15 and (ref[6] < 0).sum() > 2000
    C.assert_same_tree(ref, _twin(bins, nbins, g, h, 6, 4, 2, 0.5, mask))
    C.assert_same_tree(G.grow_numpy(bins, nbins, g, h, 6, **kw), ref, "the same setting twice")
    for rows, tile in [(256, 4), (64, 1), (5000, 12)]:
        C.assert_same_tree(G.grow_numpy(bins, nbins, g, h, 6, _rows_per_wg=rows, _feat_tile=tile, **kw), ref,
                           f"rows_per_wg {rows} feat_tile {tile}")


def _walk(bins, nbins, tree, i):
    fe, sb, dl, le, ri, val = tree[:6]
    k = 0
    while fe[k] >= 0:
        b = int(bins[fe[k], i])
        k = (le[k] if b <= sb[k] else ri[k]) if b < nbins[fe[k]] else (le[k] if dl[k] else ri[k])
    return val[k]


def test_margins_of_rows_outside_the_sample_both_routes():
    """Every row's margin receives the tree's output: the sampled rows their leaf's value, the others the value the
    tree walk over their bins ends in; both routes add the same doubles."""
    G = _G()
    dev = torch.device("cuda", 0)
    n, f = 5000, 3
    bins, nbins = C.make_bins(n, f, seed=12)
    g, h = C.float_grads(n, 12)
    want = _twin(bins, nbins, g, h, 4, 6, 1, 0.5)
    start = np.random.default_rng(1).normal(size=n)
    expect = start + np.array([_walk(bins, nbins, want, i) for i in range(n)])
    sampled = want[6] >= 0
    assert np.array_equal(expect[sampled], (start + want[5][np.maximum(want[6], 0)])[sampled])
    bst = G.Booster(bins, nbins, 4, dev)
    gd, hd = torch.from_numpy(g).to(dev), torch.from_numpy(h).to(dev)
    for route in (0, 1):
        margin = torch.from_numpy(start).to(dev)
        tree = tuple(t[0] for t in bst.new_trees(1))
        bst.grow(gd, hd, tree, 1.0, 1.0, 0.0, 0.3, margin, subsample=0.5, seed=6, round=1, _margin_route=route)
        assert np.array_equal(margin.cpu().numpy(), expect), f"route {route}"
        assert np.array_equal(bst.leaf_of_row.cpu().numpy(), want[6])


def test_weighted_gradient_kernel():
    G = _G()
    r = np.random.default_rng(6)
    n = 5000
    m, y = r.normal(0, 3, n), r.normal(0, 3, n)
    m[:4] = [0.0, 40.0, -40.0, 800.0]
    w = r.uniform(0, 4, n).astype(np.float32)
    w[::7] = 0.0
    w[1] = 4.0
    dev = torch.device("cuda", 0)
    g, h = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
    md, wd = torch.from_numpy(m).to(dev), torch.from_numpy(w).to(dev)
    G.grad_hess("reg:squarederror", md, torch.from_numpy(y).to(dev), g, h, wd)
    assert np.array_equal(g.cpu().numpy(), (m - y).astype(np.float32) * w)
    assert np.array_equal(h.cpu().numpy(), w)
    lab = (r.random(n) < 0.5).astype(np.float64)
    G.grad_hess("binary:logistic", md, torch.from_numpy(lab).to(dev), g, h, wd)
    p = 1.0 / (1.0 + np.exp(-m))
    wg, wh = (p - lab).astype(np.float32) * w, np.maximum(p * (1 - p), 1e-16).astype(np.float32) * w
    dg, dh = np.abs(g.cpu().numpy() - wg), np.abs(h.cpu().numpy() - wh)
    print(f"weighted logistic gradient kernel: max |dg| / w {np.max(dg[w > 0] / w[w > 0]):.3g}, max |dh| / w "
          f"{np.max(dh[w > 0] / w[w > 0]):.3g} (bound 2^-23 = {2.0 ** -23:.3g})")
    # the unweighted kernel's bound (one float32 ulp at magnitude <= 1) times w; a zero weight leaves no room at all
    bound = 2.0 ** -23 * w.astype(np.float64)
    assert (dg <= bound).all() and (dh <= bound).all()
    assert not g.cpu().numpy()[::7].any() and not h.cpu().numpy()[::7].any()


def _reg_data():
    r = np.random.default_rng(8)
    X = r.normal(size=(900, 6))
    y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.1, 900)
    X[r.random(X.shape) < 0.1] = np.nan
    return X[:600], y[:600], X[600:], y[600:]


def _same_fit(a, b, Xe):
    assert a.n_trees_ == b.n_trees_ and a._base_margin == b._base_margin
    for t, (ta, tb) in enumerate(zip(a._trees, b._trees)):
        for u, v in zip(ta, tb):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"tree {t}"
    assert a.evals_result_ == b.evals_result_
    assert a.best_iteration == b.best_iteration and a.best_score == b.best_score
    assert np.array_equal(a.predict(Xe), b.predict(Xe))


def test_regressor_gpu_equals_host_twin_with_sampling_and_weights():
    X, y, Xe, ye = _reg_data()
    w = np.random.default_rng(3).uniform(0, 2, len(y)).astype(np.float32)
    kw = dict(n_estimators=40, subsample=0.5, colsample_bytree=0.5, colsample_bylevel=0.5, random_state=17)
    fit = dict(eval_set=[(Xe, ye)], early_stopping_rounds=10)
    b = XGBRegressor(device="cpu", fixed_point=True, **kw).fit(X, y, sample_weight=w, **fit)
    a = XGBRegressor(device="gpu", **kw).fit(X, y, sample_weight=w, **fit)
    assert a.n_trees_ > 10
    _same_fit(a, b, Xe)
    dev = torch.device("cuda", 0)
    c = XGBRegressor(device="gpu", **kw).fit(torch.from_numpy(X).to(dev), y, sample_weight=torch.from_numpy(w).to(dev),
                                             **fit)
    _same_fit(c, b, Xe)
    d = XGBRegressor(device="gpu", **dict(kw, random_state=18)).fit(X, y, sample_weight=w, **fit)
    assert any(len(ta[0]) != len(tb[0]) or not np.array_equal(ta[0], tb[0]) for ta, tb in zip(a._trees, d._trees))


def test_classifier_gpu_first_tree_with_weights_and_scale_pos_weight():
    X, y, Xe, ye = _reg_data()
    lab, elab = (y > 1.2).astype(int), (ye > 1.2).astype(int)
    w = np.random.default_rng(4).uniform(0, 2, len(y)).astype(np.float32)
    # base_score 0.5: the first margin is 0.0, so p = 0.5 and the unweighted pair (+-0.5, 0.25) is exact everywhere
    kw = dict(n_estimators=5, scale_pos_weight=2.5, subsample=0.5, colsample_bytree=0.5, random_state=2, base_score=0.5)
    a = XGBClassifier(device="gpu", **kw).fit(X, lab, eval_set=[(Xe, elab)], sample_weight=w)
    b = XGBClassifier(device="cpu", fixed_point=True, **kw).fit(X, lab, eval_set=[(Xe, elab)], sample_weight=w)
    assert a._base_margin == 0.0 == b._base_margin and a.n_trees_ == b.n_trees_ == 5
    for u, v in zip(a._trees[0], b._trees[0]):  # the first round's gradients come from one shared margin
        assert np.array_equal(u, v)
    la, lb = a.evals_result_["validation_0"]["logloss"], b.evals_result_["validation_0"]["logloss"]
    print("weighted classifier logloss per round, gpu vs twin: " +
          " ".join(f"{u:.17g}/{v:.17g}" for u, v in zip(la, lb)))
    assert la[0] == lb[0]


def test_weights_on_another_device_are_refused():
    X, y = np.zeros((4, 2)), np.arange(4.0)
    w = torch.ones(4, device="cuda:0")
    with pytest.raises(ValueError, match="GPU"):
        XGBRegressor().fit(X, y, sample_weight=w)  # a host model
    with pytest.raises(ValueError, match="GPU"):
        XGBRegressor(device="cuda:1").fit(X, y, sample_weight=w)
