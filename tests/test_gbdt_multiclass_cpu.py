"""Multi-class XGBClassifier (multi:softprob, K >= 3 classes) on the two host learners: a planted rule, the exact first
round, the definition pinned against a hand-written boosting loop (gradients before the round, class-major margins,
tree t = round * K + k for class k, draws keyed by t), early stopping in rounds, the errors, pickling, and the
two-class path left as it was."""
import math
import pickle

import numpy as np
import pytest

from mifx.gbdt import XGBClassifier, xgb
from test_gbdt_sample_cpu import grow_ex

LEARNERS = [dict(), dict(device="cpu", fixed_point=True)]


def planted(seed=9):
    """600 rows, 4 string classes = the quadrant of (x0 >= 5, x1 >= 5): one-against-rest is learnable at depth 2.
    Ten distinct values per feature: one bin each, so the rule's cuts exist."""
    r = np.random.default_rng(seed)
    X = r.integers(0, 10, (4000, 5)).astype(np.float64)
    y = np.array(["ant", "bee", "cat", "dog"])[2 * (X[:, 0] >= 5) + (X[:, 1] >= 5)]
    keep = np.concatenate([np.flatnonzero(y == c)[:150] for c in np.unique(y)])  # balanced
    return X[keep], y[keep]


def softmax(m):
    """The specified rule on [K, n] margins: double, the sum in class order."""
    e = np.exp(m - m.max(0))
    s = e[0].copy()
    for k in range(1, len(e)):
        s += e[k]
    return e / s


@pytest.mark.parametrize("kw", LEARNERS)
def test_planted_rule(kw):
    X, y = planted()
    rounds = 12
    m = XGBClassifier(n_estimators=rounds, max_depth=2, **kw).fit(X, y, eval_set=[(X, y)])
    assert list(m.classes_) == ["ant", "bee", "cat", "dog"] and m._base_margin == 0.5
    assert m.n_trees_ == rounds * 4 and m.best_iteration is None
    assert (m.predict(X) == y).all()
    p = m.predict_proba(X)
    assert p.shape == (len(y), 4) and p.dtype == np.float64
    assert np.abs(p.sum(1) - 1.0).max() <= 1e-12
    assert (m.classes_[p.argmax(1)] == y).all()
    assert list(m.evals_result_["validation_0"]) == ["mlogloss"]
    loss = m.evals_result_["validation_0"]["mlogloss"]
    assert len(loss) == rounds and all(b < a for a, b in zip(loss, loss[1:])) and loss[-1] < math.log(4)
    # the metric is the specified one, from the model's own margins after the last round
    yi = np.searchsorted(m.classes_, y)
    want = -np.mean(np.log(np.clip(softmax(m._margins(X))[yi, np.arange(len(y))], 1e-15, 1 - 1e-15)))
    assert loss[-1] == float(want)


def test_first_round_is_exact_in_both_learners():
    """Equal margins give p = 1/4 by one division: g is 0.25 or -0.75 and h is 0.375, all dyadic, so the double
    learner and the fixed-point learner grow the same four trees."""
    X, y = planted()
    a = XGBClassifier(n_estimators=1, max_depth=3).fit(X, y)
    b = XGBClassifier(n_estimators=1, max_depth=3, device="cpu", fixed_point=True).fit(X, y)
    g, h = a._grad_hess(np.full((4, len(y)), 0.5), np.searchsorted(a.classes_, y).astype(np.float64))
    assert set(np.unique(g)) == {np.float32(0.25), np.float32(-0.75)} and set(np.unique(h)) == {np.float32(0.375)}
    assert a.n_trees_ == b.n_trees_ == 4
    for k, (ta, tb) in enumerate(zip(a._trees, b._trees)):
        assert len(ta[0]) > 1, f"class {k}: the tree has no split"
        for u, v in zip(ta, tb):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"class {k}"
    assert not np.array_equal(a._trees[0][0], a._trees[1][0]) or not np.array_equal(a._trees[0][5], a._trees[1][5])


def _bin_walk(bins, nbins, tree):
    """The leaf value of every row of a binned column-major [f, n] table: bin <= split_bin goes left, missing by
    default_left."""
    fe, sb, dl, le, ri, val = tree[:6]
    out = np.empty(bins.shape[1])
    for i in range(bins.shape[1]):
        k = 0
        while fe[k] >= 0:
            b = int(bins[fe[k], i])
            k = (le[k] if b <= sb[k] else ri[k]) if b < nbins[fe[k]] else (le[k] if dl[k] else ri[k])
        out[i] = val[k]
    return out


def test_definition_against_a_hand_written_loop():
    K, rounds, depth, seed = 3, 6, 3, 21
    r = np.random.default_rng(4)
    n, f = 400, 6
    X = r.normal(size=(n, f))
    score = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.3, n)
    y = np.array([-5, 2, 30])[np.searchsorted(np.quantile(score, [0.4, 0.7]), score)]  # unequal class sizes
    X[r.random(X.shape) < 0.05] = np.nan
    w = r.uniform(0, 3, n).astype(np.float32)
    w[:5] = 0.0
    kw = dict(n_estimators=rounds, max_depth=depth, subsample=0.5, colsample_bytree=0.7, random_state=seed,
              min_child_weight=0.5)
    m = XGBClassifier(device="cpu", fixed_point=True, **kw).fit(X, y, sample_weight=w)
    assert m.n_trees_ == rounds * K and list(m.classes_) == [-5, 2, 30]

    ref = XGBClassifier(device="cpu", fixed_point=True, **kw)
    bins = ref._bin_matrix(np.ascontiguousarray(X))
    nbins = (ref._ncut + 1).astype(np.int32)
    yi = np.searchsorted([-5, 2, 30], y)
    margin = np.full((K, n), 0.5)
    used = set()
    for it in range(rounds):
        p = softmax(margin)  # every class's pair from the margins at the start of the round
        g = (p - (yi == np.arange(K)[:, None])).astype(np.float32) * w
        h = np.maximum(2 * p * (1 - p), 1e-16).astype(np.float32) * w
        for k in range(K):
            t = it * K + k
            rows = xgb.sample_rows(seed, t, 0.5, n)
            mask = xgb.level_mask(seed, t, f, depth, 0.7, 1.0)
            used.add((tuple(rows[:8]), tuple(mask[0])))
            tree = grow_ex(bins, nbins, np.ascontiguousarray(g[k]), np.ascontiguousarray(h[k]), depth, 0.5,
                           fixed=True, rows=rows, mask=mask)
            fe, sb, dl, le, ri, val = tree[:6]
            thr = np.array([ref._cuts[a][b] if a >= 0 else 0.0 for a, b in zip(fe, sb)])
            for name, got, want in zip(("feature", "threshold", "default_left", "left", "right", "value"), m._trees[t],
                                       (fe, thr, dl, le, ri, val)):
                assert np.array_equal(got, want), f"round {it} class {k}: {name}"
            margin[k] += _bin_walk(bins, nbins, tree)
    assert len(used) == rounds * K  # every tree drew its own rows and features
    assert any(len(t[0]) > 3 for t in m._trees)
    assert np.array_equal(m.predict_proba(X), softmax(margin).T)
    assert np.array_equal(m.predict(X), np.array([-5, 2, 30])[margin.argmax(0)])


@pytest.mark.parametrize("kw", LEARNERS)
def test_early_stopping_counts_rounds(kw):
    r = np.random.default_rng(12)
    X = r.normal(size=(500, 5))
    y = (np.searchsorted([-0.5, 0.5], X[:, 0] + r.normal(0, 1.0, 500)) + 10)  # noisy: the eval loss turns early
    Xt, yt, Xe, ye = X[:300], y[:300], X[300:], y[300:]
    K = 3
    m = XGBClassifier(n_estimators=200, max_depth=4, **kw).fit(Xt, yt, eval_set=[(Xe, ye)], early_stopping_rounds=4)
    loss = m.evals_result_["validation_0"]["mlogloss"]
    assert m.best_iteration == int(np.argmin(loss)) and m.best_score == min(loss)
    assert len(loss) == m.best_iteration + 1 + 4 < 200 and m.n_trees_ == len(loss) * K
    limit = (m.best_iteration + 1) * K
    margin = np.full((K, len(ye)), m._base_margin)
    for t in range(limit):
        margin[t % K] += m._predict_trees(Xe, [m._trees[t]], 0.0)
    assert np.array_equal(m.predict_proba(Xe), softmax(margin).T)
    assert np.array_equal(m.predict(Xe), m.classes_[margin.argmax(0)])
    full = np.stack([m._predict_trees(Xe, m._trees[k::K], m._base_margin) for k in range(K)])
    assert not np.array_equal(full, margin)  # the later trees exist and are not used


def test_errors_pickle_and_base_score():
    X, y = planted()
    for dev in (None, "gpu"):  # device="gpu": refused on the host, before the device is looked for
        with pytest.raises(ValueError, match="scale_pos_weight"):
            XGBClassifier(n_estimators=2, scale_pos_weight=2.0, device=dev).fit(X, y)
    with pytest.raises(ValueError, match="classes_"):
        XGBClassifier(n_estimators=2).fit(X, y, eval_set=[(X, np.where(y == "ant", "eel", y))])
    m = XGBClassifier(n_estimators=3, max_depth=2, base_score=0.2).fit(X, y)
    assert m._base_margin == 0.2  # a raw margin, the same for every class
    c = pickle.loads(pickle.dumps(m))
    assert c.n_trees_ == 12 and list(c.classes_) == list(m.classes_)
    assert np.array_equal(c.predict_proba(X), m.predict_proba(X)) and np.array_equal(c.predict(X), m.predict(X))
    # softmax is shift invariant and the first gradients do not see the intercept: the same trees
    d = XGBClassifier(n_estimators=1, max_depth=2).fit(X, y)
    for ta, tb in zip(m._trees[:4], d._trees):
        assert all(np.array_equal(u, v) for u, v in zip(ta, tb))
    assert np.array_equal(m.predict(np.full((2, 5), np.nan)), m.predict(np.full((2, 5), np.nan)))


def test_tie_goes_to_the_lowest_class():
    X, y = planted()
    m = XGBClassifier(n_estimators=0).fit(X, y)  # no tree: every margin is the intercept
    assert m.n_trees_ == 0 and (m.predict(X[:7]) == "ant").all()
    assert np.array_equal(m.predict_proba(X[:7]), np.full((7, 4), 0.25))


def test_two_classes_stay_binary_logistic():
    X, y = planted()
    two = np.where(np.isin(y, ["ant", "bee"]), "no", "yes")
    m = XGBClassifier(n_estimators=5, max_depth=2).fit(X, two, eval_set=[(X, two)])
    assert m._num_class() == 1 and m.n_trees_ == 5 and list(m.evals_result_["validation_0"]) == ["logloss"]
    assert m.predict_proba(X).shape == (len(y), 2) and (m.predict(X) == two).all()
    assert m._base_margin == 0.0  # the log-odds of a balanced sample, not multi:softprob's 0.5
    c = pickle.loads(pickle.dumps(m))
    assert c._num_class() == 1 and np.array_equal(c.predict_proba(X), m.predict_proba(X))
