"""The device GBDT learner (csrc/gbdt_gpu.hip, mifx/ops/gbdt_gpu.py, XGB*(device="gpu")) against its host twin
mifx_gbdt_grow_fixed: exact equality of every tree array and of leaf_of_row -- integer histograms leave no room for a
tolerance -- over the shape grid of tests/gbdt_cases.py, for any launch geometry, and end to end."""
import math
import pickle

import numpy as np
import pytest
import torch

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, XGBRegressor

pytestmark = pytest.mark.gpu


def _G():
    from mifx.ops import gbdt_gpu

    return gbdt_gpu


@pytest.mark.parametrize("n,f", C.SHAPES)
def test_device_grower_equals_host_twin(n, f):
    G = _G()
    seed = n * 31 + f
    bins, nbins = C.make_bins(n, f, seed)
    grads = {"float": C.float_grads(n, seed), "1e-30": C.float_grads(n, seed, 1e-30),
             "1e30": C.float_grads(n, seed, 1e30), "dyadic": C.dyadic_grads(n, seed)}
    for depth, mcw, gamma in C.PARAMS:
        for name, (g, h) in grads.items():
            if name in ("1e-30", "1e30") and (mcw, gamma) != (1.0, 0.0):
                continue  # the scaled gradients once per depth
            got = G.grow_numpy(bins, nbins, g, h, depth, mcw, 1.0, gamma, 0.3)
            what = f"{name} depth {depth} mcw {mcw} gamma {gamma}"
            C.assert_same_tree(got, C.host_grow(bins, nbins, g, h, depth, mcw, gamma, fixed=True), what)
            if name == "dyadic":  # exactly representable: the double learner grows the same tree
                C.assert_same_tree(got, C.host_grow(bins, nbins, g, h, depth, mcw, gamma, fixed=False), what)


def test_device_grower_levels_that_die_early_and_deep_trees():
    G = _G()
    bins, nbins = np.array([[0, 1]], np.uint16), np.array([2], np.int32)
    g, h = np.array([-1.0, 1.0], np.float32), np.ones(2, np.float32)
    got = G.grow_numpy(bins, nbins, g, h, 6, 0.0, 1.0, 0.0, 0.3)  # level 1: two single-row leaves, levels 2-6 dead
    C.assert_same_tree(got, C.host_grow(bins, nbins, g, h, 6, 0.0, 0.0, fixed=True))
    assert len(got[0]) == 3
    bins, nbins = C.make_bins(300, 3, seed=1)
    z, one = np.zeros(300, np.float32), np.ones(300, np.float32)
    got = G.grow_numpy(bins, nbins, z, one, 6, 1.0, 1.0, 0.0, 0.3)  # all-zero g: the root is the only node
    C.assert_same_tree(got, C.host_grow(bins, nbins, z, one, 6, 1.0, 0.0, fixed=True))
    assert len(got[0]) == 1
    bins, nbins = C.make_bins(5000, 3, seed=2)  # depth 10: up to 1024 nodes in a level, most rows in tiny nodes
    g, h = C.float_grads(5000, 2)
    C.assert_same_tree(G.grow_numpy(bins, nbins, g, h, 10, 0.0, 1.0, 0.0, 0.3),
                       C.host_grow(bins, nbins, g, h, 10, 0.0, 0.0, fixed=True))


def test_device_grower_out_of_range_bins_are_missing():
    """Any uint16 content is in bounds: a value >= nbins[j] routes and accumulates like 0xFFFF."""
    G = _G()
    bins, nbins = C.make_bins(1000, 3, seed=3)
    g, h = C.float_grads(1000, 3)
    odd = bins.copy()
    odd[odd == 0xFFFF] = np.random.default_rng(0).integers(300, 0xFFFF, (odd == 0xFFFF).sum()).astype(np.uint16)
    C.assert_same_tree(G.grow_numpy(odd, nbins, g, h, 4), G.grow_numpy(bins, nbins, g, h, 4))


def test_device_grower_geometry_independent():
    G = _G()
    bins, nbins = C.make_bins(5000, 11, seed=4)
    g, h = C.float_grads(5000, 4)
    ref = G.grow_numpy(bins, nbins, g, h, 6)
    assert len(ref[0]) > 15
    C.assert_same_tree(G.grow_numpy(bins, nbins, g, h, 6), ref, "the same setting twice")
    for rows, tile in [(256, 4), (64, 1), (5000, 12), (1000, 3)]:
        C.assert_same_tree(G.grow_numpy(bins, nbins, g, h, 6, _rows_per_wg=rows, _feat_tile=tile), ref,
                           f"rows_per_wg {rows} feat_tile {tile}")


def test_gradient_kernel():
    G = _G()
    r = np.random.default_rng(6)
    n = 5000
    m, y = r.normal(0, 3, n), r.normal(0, 3, n)
    m[:4] = [0.0, 40.0, -40.0, 800.0]  # p = 0.5; p rounds to 1; p tiny; exp overflows to p = 1... and h clamps
    dev = torch.device("cuda", 0)
    g, h = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
    md = torch.from_numpy(m).to(dev)
    G.grad_hess("reg:squarederror", md, torch.from_numpy(y).to(dev), g, h)
    assert np.array_equal(g.cpu().numpy(), (m - y).astype(np.float32))
    assert np.array_equal(h.cpu().numpy(), np.ones(n, np.float32))
    lab = (r.random(n) < 0.5).astype(np.float64)
    G.grad_hess("binary:logistic", md, torch.from_numpy(lab).to(dev), g, h)
    p = 1.0 / (1.0 + np.exp(-m))
    wg, wh = (p - lab).astype(np.float32), np.maximum(p * (1 - p), 1e-16).astype(np.float32)
    eg, eh = np.abs(g.cpu().numpy() - wg).max(), np.abs(h.cpu().numpy() - wh).max()
    print(f"logistic gradient kernel: max |dg| {eg:.3g}, max |dh| {eh:.3g} (bound 2^-23 = {2.0 ** -23:.3g})")
    assert eg <= 2.0 ** -23 and eh <= 2.0 ** -23  # one float32 ulp at magnitude <= 1


def _reg_data():
    r = np.random.default_rng(8)
    X = r.normal(size=(900, 6))
    y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.1, 900)
    X[r.random(X.shape) < 0.1] = np.nan
    return X[:600], y[:600], X[600:], y[600:]


def test_regressor_gpu_equals_host_twin_end_to_end():
    X, y, Xe, ye = _reg_data()
    kw = dict(n_estimators=60, learning_rate=0.3)
    a = XGBRegressor(device="gpu", **kw).fit(X, y, eval_set=[(Xe, ye)], early_stopping_rounds=10)
    b = XGBRegressor(device="cpu", fixed_point=True, **kw).fit(X, y, eval_set=[(Xe, ye)], early_stopping_rounds=10)
    assert a.n_trees_ == b.n_trees_ and a.n_trees_ > 10
    for t, (ta, tb) in enumerate(zip(a._trees, b._trees)):
        for u, v in zip(ta, tb):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"tree {t}"
    assert a.evals_result_ == b.evals_result_
    assert a.best_iteration == b.best_iteration and a.best_score == b.best_score and a._base_margin == b._base_margin
    assert np.array_equal(a.predict(Xe), b.predict(Xe))
    c = pickle.loads(pickle.dumps(a))
    assert np.array_equal(c.predict(Xe), a.predict(Xe))
    d = XGBRegressor(device="cuda:0", n_estimators=5).fit(X, y)  # no eval set: nothing read back before the end
    e = XGBRegressor(fixed_point=True, n_estimators=5).fit(X, y)
    assert d.best_iteration is None and d.evals_result_ == {} and np.array_equal(d.predict(Xe), e.predict(Xe))


def test_classifier_gpu_planted_rule():
    r = np.random.default_rng(9)
    n = 2000
    X = r.integers(0, 10, (n, 5)).astype(np.float64)  # ten distinct values: one bin each, the rule's cuts exist
    y = np.where((X[:, 0] >= 5) & (X[:, 1] >= 5), "b", "a")  # learnable greedily at depth 2
    keep = np.concatenate([np.flatnonzero(y == "a")[:300], np.flatnonzero(y == "b")[:300]])  # balanced: mean 0.5
    X, y = X[keep], y[keep]
    kw = dict(n_estimators=20, max_depth=2, learning_rate=0.3)
    a = XGBClassifier(device="gpu", **kw).fit(X, y, eval_set=[(X, y)])
    a2 = XGBClassifier(device="gpu", **kw).fit(X, y, eval_set=[(X, y)])
    b = XGBClassifier(**kw).fit(X, y, eval_set=[(X, y)])
    assert a._base_margin == 0.0 == b._base_margin
    for u, v in zip(a._trees[0], b._trees[0]):  # g = +-0.5, h = 0.25: exact in every learner
        assert np.array_equal(u, v)
    for ta, tb in zip(a._trees, a2._trees):
        assert all(np.array_equal(u, v) for u, v in zip(ta, tb))
    assert a.evals_result_ == a2.evals_result_
    assert (a.predict(X) == y).all() and (b.predict(X) == y).all()
    la, lb = a.evals_result_["validation_0"]["logloss"], b.evals_result_["validation_0"]["logloss"]
    print("classifier logloss per round, gpu vs cpu: " + " ".join(f"{u:.17g}/{v:.17g}" for u, v in zip(la, lb)))
    assert la[-1] < math.log(2) and la[-1] < la[0]
    assert a.predict_proba(X).shape == (len(y), 2)


def test_device_limits_raise_before_any_launch():
    X, y = np.zeros((4, 2)), np.zeros(4)
    with pytest.raises(ValueError, match="max_bins"):
        XGBRegressor(device="gpu", max_bins=257).fit(X, y)
    with pytest.raises(ValueError, match="max_depth"):
        XGBRegressor(device="gpu", max_depth=13).fit(X, y)
    with pytest.raises(ValueError, match="GPU"):
        XGBRegressor(device="cuda:64").fit(X, y)  # one visible GPU is all this learner uses
    with pytest.raises(ValueError, match="2\\^31"):
        _G().check_limits(2 ** 31, 256, 6)
    with pytest.raises(ValueError, match="fixed point"):
        XGBRegressor(device="gpu", fixed_point=False)
