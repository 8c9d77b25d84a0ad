"""Leaf-wise growth (grow_policy="lossguide", max_leaves) on the host learners: with a budget that does not bind the
tree is the depth-wise one up to node numbering; with a binding budget it is the best-first prefix of the depth-wise
tree, checked against a selection and leaf values computed here in Python integers."""
import numpy as np
import pytest

from mifx.gbdt import XGBClassifier, XGBRegressor, xgb


def _table(n=2000, f=5, seed=0):
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, f))
    y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.1, n)
    X[r.random(X.shape) < 0.1] = np.nan
    return X, y


def _one_tree(X, y, fixed, **kw):
    m = XGBRegressor(n_estimators=1, n_jobs=1, base_score=0.0, device="cpu" if fixed else None,
                     fixed_point=True if fixed else None, **kw).fit(X, y)
    return m, m._trees[0], m._node_stats[0]


@pytest.mark.parametrize("fixed", [True, False])
@pytest.mark.parametrize("d", [1, 3, 6])
def test_budget_that_does_not_bind_gives_the_depthwise_leaves(d, fixed):
    X, y = _table()
    a, ta, _ = _one_tree(X, y, fixed, max_depth=d)
    b, tb, _ = _one_tree(X, y, fixed, max_depth=d, grow_policy="lossguide", max_leaves=2 ** d)
    pa, pb = a.predict(X), b.predict(X)
    assert len(ta[0]) == len(tb[0]) > 1
    if fixed:
        assert np.array_equal(pa, pb)
        return
    assert sorted(ta[5][ta[0] < 0]) == pytest.approx(sorted(tb[5][tb[0] < 0]), rel=1e-12, abs=0)  # the same leaf set
    assert np.allclose(pa, pb, rtol=1e-12, atol=0)  # double sums of <= 2000 terms reorder by at most n 2^-53 ~ 2e-13


def _leaf_of(tree, x):
    fe, thr, dl, le, ri, _ = tree
    k = 0
    while fe[k] >= 0:
        k = (le[k] if dl[k] else ri[k]) if np.isnan(x[fe[k]]) else (le[k] if x[fe[k]] < thr[k] else ri[k])
    return k


def _best_first(tree, gain, budget):
    """Depth-wise node ids in the order a best-first selection splits them: the largest gain among the open nodes,
    ties to the node created earlier. Returns [(depth-wise id, its id in the lossguide tree)]."""
    fe, _, _, le, ri, _ = tree
    created, open_, order = {0: 0}, [0], []
    while len(order) + 1 < budget and any(fe[k] >= 0 for k in open_):
        k = max((k for k in open_ if fe[k] >= 0), key=lambda k: (gain[k], -created[k]))
        open_.remove(k)
        order.append((k, created[k]))
        for c in (le[k], ri[k]):
            created[int(c)] = len(created)
            open_.append(int(c))
    return order, created


@pytest.mark.parametrize("L", [2, 3, 7, 20])
def test_binding_budget_is_the_best_first_prefix(L):
    X, y = _table(seed=L)
    n, d, eta, lam = len(y), 6, 0.3, 1.0
    _, ta, (gain, _) = _one_tree(X, y, True, max_depth=d)
    m, tb, (gb, _) = _one_tree(X, y, True, max_depth=d, grow_policy="lossguide", max_leaves=L)
    order, created = _best_first(ta, gain, L)
    assert len(order) == L - 1 and len(tb[0]) == 2 * L - 1
    for dw, lg in order:  # the same split, and children numbered in creation order
        assert (tb[0][lg], tb[1][lg], tb[2][lg]) == (ta[0][dw], ta[1][dw], ta[2][dw]) and gb[lg] == gain[dw]
        assert (tb[3][lg], tb[4][lg]) == (created[ta[3][dw]], created[ta[4][dw]])
    assert sorted(np.flatnonzero(tb[0] >= 0)) == sorted(lg for _, lg in order)
    # leaf values from rows quantised here: -eta G / (H + lambda) with G, H summed in Python integers
    g = (0.0 - y).astype(np.float32)  # base_score 0: margin 0, g = margin - y, h = 1
    lib = xgb._lib()
    eg, eh = lib.mifx_gbdt_quant_exp(float(np.abs(g).max()), n), lib.mifx_gbdt_quant_exp(1.0, n)
    qg = [int(np.rint(np.ldexp(float(v), eg))) for v in g]
    leaf = np.array([_leaf_of(tb, x) for x in X])
    for k in np.flatnonzero(tb[0] < 0):
        rows = np.flatnonzero(leaf == k)
        G, H = sum(qg[i] for i in rows), len(rows) << eh
        assert tb[5][k] == -eta * np.ldexp(float(G), -eg) / (np.ldexp(float(H), -eh) + lam)


@pytest.mark.parametrize("fixed", [True, False])
def test_ties_expand_the_lower_id_first(fixed):
    """Two halves separated by feature 0, identical but for the sign of y: g and -g give both children of the root the
    same candidate with the same gain (the score is G^2 / (H + lambda)); with a budget of 3 leaves the left child
    (id 1) is the one that is split."""
    r = np.random.default_rng(3)
    half, yh = r.integers(0, 8, (200, 2)).astype(np.float64), r.integers(-8, 9, 200) / 4.0
    X = np.concatenate([np.c_[np.zeros(200), half], np.c_[np.ones(200), half]])
    y1 = 20.0 + 3.0 * half[:, 0] + yh
    y = np.concatenate([y1, -y1])
    _, t, (gain, _) = _one_tree(X, y, fixed, max_depth=2)
    assert t[0][0] == 0 and gain[1] == gain[2] > 0  # depth-wise: both children split, with equal gains
    _, t, _ = _one_tree(X, y, fixed, max_depth=0, grow_policy="lossguide", max_leaves=3)
    assert t[0][1] >= 0 and t[0][2] < 0 and (t[3][1], t[4][1]) == (3, 4)


def test_argument_errors():
    X, y = _table(50, 3)
    with pytest.raises(ValueError, match="max_leaves"):
        XGBRegressor(max_leaves=8)  # depth-wise has no leaf budget
    with pytest.raises(ValueError, match="max_leaves"):
        XGBRegressor(grow_policy="lossguide", max_leaves=1)
    with pytest.raises(ValueError, match="grow_policy"):
        XGBClassifier(grow_policy="bestfirst")
    with pytest.raises(ValueError, match="colsample_bylevel"):
        XGBRegressor(grow_policy="lossguide", max_leaves=8, colsample_bylevel=0.5)
    m = XGBRegressor(grow_policy="lossguide", max_leaves=8)
    m.max_leaves = 0
    with pytest.raises(ValueError, match="max_leaves"):
        m.fit(X, y)
    for kw in (dict(max_leaves=4097), dict(max_leaves=8, max_depth=13)):  # device limits: before any launch, no GPU
        with pytest.raises(ValueError, match="device='gpu' supports"):
            XGBRegressor(device="gpu", grow_policy="lossguide", **kw).fit(X, y)
    old = XGBRegressor(n_estimators=2).fit(X, y)
    del old.grow_policy, old.max_leaves  # a model pickled before the parameters existed
    assert old._policy() == ("depthwise", 0) and old.fit(X, y).n_trees_ == 2
