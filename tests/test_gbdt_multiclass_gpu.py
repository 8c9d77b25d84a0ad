"""Multi-class XGBClassifier on the device: the softmax gradient kernel (csrc/gbdt_gpu.hip) against the numpy rule, a
device round of K trees against the host twin bit for bit, XGBClassifier(device="gpu") end to end, and the one-launch
multi-class forest prediction (csrc/gbdt_prep.hip) against the host's per-class walk bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, xgb
from test_gbdt_multiclass_cpu import _bin_walk, planted, softmax
from test_gbdt_sample_cpu import grow_ex

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _G():
    from mifx.ops import gbdt_gpu

    return gbdt_gpu


def _P():
    from mifx.ops import gbdt_prep

    return gbdt_prep


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the gradient kernel

def rule(margin, yi):
    """The specification: float32 g, h [K, n] from float64 margins [K, n] and class indices."""
    p = softmax(margin)
    g = (p - (yi == np.arange(len(margin))[:, None])).astype(np.float32)
    return g, np.maximum(2 * p * (1 - p), 1e-16).astype(np.float32)


@pytest.mark.parametrize("K", [3, 4, 7, 33])
@pytest.mark.parametrize("n", [1, 63, 65, 257, 5000])
def test_softmax_gradient_kernel(n, K):
    G = _G()
    r = np.random.default_rng(n * 100 + K)
    m = r.normal(0, 3, (K, n))
    special = [np.full(K, 1.7), np.where(np.arange(K) == 1, 41.0, 1.0), np.where(np.arange(K) == K - 1, 803.0, 3.0),
               np.where(np.arange(K) == 0, -801.0, -1.0)]  # equal; one 40 above; one 800 above; one 800 below
    for i, col in enumerate(special[:n]):
        m[:, i] = col
    yi = r.integers(0, K, n)
    yi[:min(n, 4)] = [0, 1, K - 1, 0][:min(n, 4)]
    w = r.uniform(0, 4, n).astype(np.float32)
    w[::7] = 0.0
    md, yd, wd = up(m), up(yi.astype(np.float64)), up(w)
    g, h, gw, hw = (torch.full((K, n), 7.0, dtype=torch.float32, device=DEV) for _ in range(4))
    G.grad_hess_softmax(md, yd, g, h)
    G.grad_hess_softmax(md, yd, gw, hw, wd)
    g, h, gw, hw = (t.cpu().numpy() for t in (g, h, gw, hw))
    wg, wh = rule(m, yi)
    eg, eh = np.abs(g.astype(np.float64) - wg).max(), np.abs(h.astype(np.float64) - wh).max()
    print(f"softmax gradient kernel n {n} K {K}: max |dg| {eg:.3g}, max |dh| {eh:.3g} (bound 2^-23 = {2.0 ** -23:.3g})")
    assert eg <= 2.0 ** -23 and eh <= 2.0 ** -23  # one float32 spacing at magnitude <= 1
    # equal margins: p = 1 / K by one IEEE division, nothing to differ in
    assert np.array_equal(g[:, 0], wg[:, 0]) and np.array_equal(h[:, 0], wh[:, 0])
    assert np.array_equal(h[:, 0], np.full(K, np.float32(max(2 * (1.0 / K) * (1 - 1.0 / K), 1e-16))))
    if n > 2:  # every other e_k underflows: p is 0 or 1 and h clamps
        assert np.array_equal(h[:, 2], np.full(K, np.float32(1e-16)))
        assert not g[:, 2].any()  # the row's label is the class with p = 1
    # weights: the unweighted float32 pair times the float32 weight, one multiply each
    assert np.array_equal(gw, g * w) and np.array_equal(hw, h * w)
    assert not gw[:, ::7].any() and not hw[:, ::7].any()


# ---- one device round = one gradient launch + K growers, against the host twin fed the device's gradients

def _device_tree(bst, tree):
    cnt = int(tree[6].item())
    return tuple(t[:cnt].cpu().numpy() for t in tree[:6]) + (bst.leaf_of_row.cpu().numpy(),)


@pytest.mark.parametrize("subsample", [1.0, 0.5])
def test_device_round_equals_host_twin(subsample):
    G = _G()
    n, f, depth, K, rounds, seed = 1000, 11, 3, 3, 5, 77
    bins, nbins = C.make_bins(n, f, seed=5)
    yi = np.random.default_rng(5).integers(0, K, n)
    bst = G.Booster(bins, nbins, depth, DEV)
    margin = torch.full((K, n), 0.5, dtype=torch.float64, device=DEV)
    host_margin = np.full((K, n), 0.5)
    g, h = (torch.empty((K, n), dtype=torch.float32, device=DEV) for _ in range(2))
    yd = up(yi.astype(np.float64))
    trees = bst.new_trees(rounds * K)
    split = 0
    for it in range(rounds):
        G.grad_hess_softmax(margin, yd, g, h)
        gh, hh = g.cpu().numpy(), h.cpu().numpy()
        for k in range(K):
            t = it * K + k
            tree = tuple(x[t] for x in trees)
            bst.grow(g[k], h[k], tree, 1.0, 1.0, 0.0, 0.3, margin[k], subsample=subsample, seed=seed, round=t)
            got = _device_tree(bst, tree)
            gk, hk = np.ascontiguousarray(gh[k]), np.ascontiguousarray(hh[k])
            if subsample == 1.0:
                want = C.host_grow(bins, nbins, gk, hk, depth, 1.0, 0.0, fixed=True)
                host_margin[k] += want[5][want[6]]
            else:  # the tree index keys the draw; rows outside the sample walk the tree
                rows = xgb.sample_rows(seed, t, subsample, n)
                want = grow_ex(bins, nbins, gk, hk, depth, 1.0, fixed=True, rows=rows)
                assert (want[6] < 0).sum() == n - len(rows) > 300
                host_margin[k] += _bin_walk(bins, nbins, want)
            C.assert_same_tree(got, want, f"round {it} class {k}")
            split += len(want[0]) > 1
        assert np.array_equal(margin.cpu().numpy(), host_margin), f"margins after round {it}"
    assert split >= rounds * K - 2  # the trees are trees


# ---- end to end

def test_classifier_gpu_planted_rule_four_classes():
    X, y = planted()
    kw = dict(n_estimators=12, max_depth=2)
    a = XGBClassifier(device="gpu", **kw).fit(X, y, eval_set=[(X, y)])
    a2 = XGBClassifier(device="gpu", **kw).fit(X, y, eval_set=[(X, y)])
    b = XGBClassifier(device="cpu", fixed_point=True, **kw).fit(X, y, eval_set=[(X, y)])
    assert a.n_trees_ == a2.n_trees_ == b.n_trees_ == 48 and a._base_margin == 0.5
    for k in range(4):  # g = 0.25 / -0.75, h = 0.375 from one shared margin: exact everywhere
        for u, v in zip(a._trees[k], b._trees[k]):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"first round, class {k}"
    for ta, tb in zip(a._trees, a2._trees):
        assert all(np.array_equal(u, v) for u, v in zip(ta, tb))
    assert a.evals_result_ == a2.evals_result_
    assert (a.predict(X) == y).all()
    la, lb = a.evals_result_["validation_0"]["mlogloss"], b.evals_result_["validation_0"]["mlogloss"]
    print("4-class mlogloss per round, gpu vs twin: " + " ".join(f"{u:.17g}/{v:.17g}" for u, v in zip(la, lb)))
    assert len(la) == 12 and la[-1] < la[0] and la[-1] < math.log(4)
    p = a.predict_proba(X)
    assert p.shape == (len(y), 4) and np.abs(p.sum(1) - 1).max() <= 1e-12


def test_classifier_gpu_with_sampling_weights_and_early_stopping():
    """Tensors on the device in, draws keyed by the tree index, rounds counted by early stopping: the first round's
    trees are the twin's (shared margins, exact gradients), and the model predicts from (best_iteration + 1) K trees."""
    X, y, Xe, ye = _data(3)
    w = np.random.default_rng(4).uniform(0.5, 2, len(y)).astype(np.float32)
    kw = dict(n_estimators=40, max_depth=3, subsample=0.5, colsample_bytree=0.6, colsample_bylevel=0.7, random_state=3)
    a = XGBClassifier(device="gpu", **kw).fit(up(X), up(y), eval_set=[(up(Xe), ye)], early_stopping_rounds=3,
                                              sample_weight=up(w))
    b = XGBClassifier(device="cpu", fixed_point=True, **kw).fit(X, y, eval_set=[(Xe, ye)], early_stopping_rounds=3,
                                                                sample_weight=w)
    for k in range(3):
        for u, v in zip(a._trees[k], b._trees[k]):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"first round, class {k}"
    loss = a.evals_result_["validation_0"]["mlogloss"]
    assert loss[0] == b.evals_result_["validation_0"]["mlogloss"][0]
    assert a.best_iteration == int(np.argmin(loss)) and a.n_trees_ == len(loss) * 3
    assert len(loss) == a.best_iteration + 4 or len(loss) == 40
    limit = (a.best_iteration + 1) * 3
    want = np.stack([a._predict_trees(Xe, a._trees[k:limit:3], a._base_margin) for k in range(3)])
    assert np.array_equal(a._margins(Xe), want) and np.array_equal(a._margins(up(Xe)).cpu().numpy(), want)


# ---- prediction

def _data(K, n=700, f=7, seed=31):
    r = np.random.default_rng(seed + K)
    X = r.normal(size=(n, f))
    score = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.5, n)
    y = np.searchsorted(np.quantile(score, np.arange(1, K) / K), score)
    X[r.random(X.shape) < 0.08] = np.nan
    return X[:500], y[:500], X[500:], y[500:]


@functools.lru_cache(maxsize=None)
def _models(K):
    """One model trained on the device and one on the host (double histograms), both stopped early."""
    X, y, Xe, ye = _data(K)
    kw = dict(n_estimators=25, max_depth=4)
    fit = dict(eval_set=[(Xe, ye)], early_stopping_rounds=2)
    ms = (XGBClassifier(device="gpu", **kw).fit(X, y, **fit), XGBClassifier(**kw).fit(X, y, **fit))
    for m in ms:
        assert m._num_class() == K and m.n_trees_ > (m.best_iteration + 1) * K > K
        assert max(len(t[0]) for t in m._trees) > 7  # a chunk of 7 nodes does not hold every tree
    return ms


@functools.lru_cache(maxsize=None)
def _table(n):
    r = np.random.default_rng(n)
    X = r.normal(size=(n, 7))
    X[r.random(X.shape) < 0.1] = np.nan
    return X


def _host_margins(m, X, limit, K):
    return np.stack([m._predict_trees(X, m._trees[k:limit:K], m._base_margin) for k in range(K)])


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
def test_multiclass_prediction_equals_host_per_class_walk(n, K):
    P = _P()
    X64 = _table(n)
    for m in _models(K):
        forest = P.DeviceForest(m._trees, m._nfeat, DEV)
        for X in (X64, X64.astype(np.float32)):
            Xd = up(X)
            for limit in (0, (m.best_iteration + 1) * K, m.n_trees_):
                want = _host_margins(m, X.astype(np.float64), limit, K)
                for chunk in (1, 7, None):  # 1: every tree is walked from global memory; 7: some are
                    for route in ("registers", "output", "launches"):
                        got = P.predict_multi(forest, Xd, m._base_margin, K, limit, _nodes_per_chunk=chunk,
                                              _route=route)
                        assert got.dtype == torch.float64 and tuple(got.shape) == (K, n) and got.is_contiguous()
                        assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64)), \
                            f"{X.dtype} limit {limit} chunk {chunk} route {route}"
            # the wider register tile, and more classes than it holds (the default route is then one launch per
            # class): the same forest read as 9 and as 17 classes (tree t -> class t % 9, t % 17)
            for classes in (9, 17):
                want = _host_margins(m, X.astype(np.float64), m.n_trees_ - 1, classes)
                for chunk in (7, None):
                    for route in (None, "output"):
                        got = P.predict_multi(forest, Xd, m._base_margin, classes, m.n_trees_ - 1,
                                              _nodes_per_chunk=chunk, _route=route)
                        assert np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64)), \
                            f"{classes} classes, chunk {chunk}, route {route}"
        # the estimator on a device tensor: probabilities stay there, labels come back once
        p = m.predict_proba(up(X64))
        assert isinstance(p, torch.Tensor) and p.device == DEV and tuple(p.shape) == (n, K)
        ph = m.predict_proba(X64)
        # the margins are the same bits; torch.exp and numpy's may differ in the last bit of every e_k, so of s too, and
        # the quotient rounds once more: at most 4 spacings of a double at p <= 1
        assert ph.shape == (n, K) and np.abs(p.cpu().numpy() - ph).max() <= 2.0 ** -50
        lab = m.predict(up(X64))
        assert isinstance(lab, np.ndarray) and np.array_equal(lab, m.predict(X64))


def test_prediction_arguments_are_checked_before_any_launch():
    P = _P()
    m = _models(3)[1]
    forest = P.DeviceForest(m._trees, m._nfeat, DEV)
    Xd = up(_table(4))
    with pytest.raises(ValueError, match="num_class"):
        P.predict_multi(forest, Xd, 0.5, 0)
    with pytest.raises(ValueError, match="register"):
        P.predict_multi(forest, Xd, 0.5, P._fns()["reg_classes"]() + 1, _route="registers")
    with pytest.raises(ValueError, match="route"):
        P.predict_multi(forest, Xd, 0.5, 3, _route="fastest")
    with pytest.raises(ValueError, match="n_trees"):
        P.predict_multi(forest, Xd, 0.5, 3, m.n_trees_ + 1)
    with pytest.raises(ValueError, match="features"):
        P.predict_multi(forest, up(np.zeros((4, 6))), 0.5, 3)
    assert tuple(P.predict_multi(forest, Xd, 0.5, 300).shape) == (300, 4)  # the number of classes has no upper limit
