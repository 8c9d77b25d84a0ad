"""eval_metric="auc" on the host: mifx.gbdt.xgb.auc against a plain O(P N) numpy double loop over all pairs, and
XGBClassifier(eval_metric=...) on the host learners. Every comparison is exact equality."""
import numpy as np
import pytest

from mifx.gbdt import XGBClassifier, xgb

MARGIN_SETS = ("normal", "ties", "equal", "separated", "reversed")
LABEL_SETS = ("mixed", "one_positive", "one_negative")


def make_case(m: int, margins: str, labels: str, seed: int = 0):
    """(margin float64 [m], y 0 / 1 [m]); the separated sets order the classes by margin."""
    rng = np.random.default_rng(1000 * m + seed)
    if labels == "mixed":
        y = (rng.random(m) < 0.4).astype(np.float64)
        y[0], y[-1] = 1.0, 0.0
    else:  # exactly one row of the rare class
        y = np.full(m, float(labels == "one_negative"))
        y[m // 2] = float(labels == "one_positive")
    if margins == "normal":
        x = rng.standard_normal(m)
    elif margins == "ties":
        x = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 3.0]), m)
    elif margins == "equal":
        x = np.full(m, 0.7)
    else:
        x = rng.random(m) + np.where(y == 1.0, 2.0, 0.0) * (1.0 if margins == "separated" else -1.0)
    return x, y


def pair_loop(margin: np.ndarray, pos: np.ndarray):
    """(U2, P, N) as Python ints and the score: (m_i > m_j) + 0.5 (m_i == m_j) over every (positive i, negative j)."""
    p, n = margin[pos], margin[~pos]
    above = int((p[:, None] > n[None, :]).sum())
    tied = int((p[:, None] == n[None, :]).sum())
    return 2 * above + tied, len(p), len(n)


@pytest.mark.parametrize("labels", LABEL_SETS)
@pytest.mark.parametrize("margins", MARGIN_SETS)
@pytest.mark.parametrize("m", [2, 65, 257, 3000])
def test_auc_equals_the_pair_loop(m, margins, labels):
    x, y = make_case(m, margins, labels)
    u2, P, N = pair_loop(x, y == 1.0)
    score, (U2, Pc, Nc) = xgb.auc(x, y, return_counts=True)
    assert (int(U2[0]), int(Pc[0]), int(Nc[0])) == (u2, P, N)
    assert score == u2 / (2 * P * N)
    want = {"equal": 0.5, "separated": 1.0, "reversed": 0.0}.get(margins)
    assert want is None or score == want
    assert xgb.auc(x, y, threads=1) == xgb.auc(x, y, threads=5) == score


def test_auc_multiclass_is_the_prevalence_weighted_loop():
    from fractions import Fraction

    rng = np.random.default_rng(3)
    y = rng.integers(0, 3, 501).astype(np.float64)
    x = np.round(rng.standard_normal((3, 501)), 1) + (y == np.arange(3.0)[:, None])  # (rounded: ties)
    loops = [pair_loop(x[k], y == k) for k in range(3)]
    score, counts = xgb.auc(x, y, return_counts=True)
    assert [tuple(int(c[k]) for c in counts) for k in range(3)] == loops
    assert score == float(sum(p * Fraction(u, 2 * p * n) for u, p, n in loops) / sum(p for _, p, _ in loops))


def test_auc_refuses_bad_input():
    with pytest.raises(ValueError):
        xgb.auc(np.array([0.1, np.inf, 0.3]), np.array([0.0, 1.0, 1.0]))
    with pytest.raises(ValueError):
        xgb.auc(np.array([0.1, 0.2, 0.3]), np.array([1.0, 1.0, 1.0]))


def planted(n, seed, classes=2):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 6))
    s = X[:, 0] + 0.5 * X[:, 1] * X[:, 2] + 0.8 * rng.standard_normal(n)
    return X, np.digitize(s, np.quantile(s, np.arange(1, classes) / classes))


@pytest.mark.parametrize("fixed_point", [False, True])
@pytest.mark.parametrize("classes", [2, 3])
def test_fit_stops_on_the_maximum_and_records_auc(classes, fixed_point):
    (X, y), (ex, ey) = planted(600, 1, classes), planted(300, 2, classes)
    clf = XGBClassifier(n_estimators=60, max_depth=3, learning_rate=0.5, eval_metric="auc", fixed_point=fixed_point)
    clf.fit(X, y, eval_set=[(ex, ey)], early_stopping_rounds=4)
    hist = clf.evals_result_["validation_0"]["auc"]
    K = clf._num_class()
    assert len(hist) < 60 and clf.best_iteration == int(np.argmax(hist)) == len(hist) - 5
    assert clf.best_score == max(hist) > 0.7
    for it, score in enumerate(hist):
        trees = clf._trees[:(it + 1) * K]
        margin = np.stack([clf._predict_trees(ex, trees[k::K], clf._base_margin) for k in range(K)])
        assert score == xgb.auc(margin if K > 1 else margin[0], ey.astype(np.float64))


def test_one_class_eval_set_raises_before_the_first_round():
    (X, y), (ex, _) = planted(200, 1), planted(50, 2)
    clf = XGBClassifier(n_estimators=3, eval_metric="auc")
    with pytest.raises(ValueError, match="no positive or no negative"):
        clf.fit(X, y, eval_set=[(ex, np.ones(50, dtype=y.dtype))])
    assert clf._trees == []


def test_unknown_or_mismatched_metric_raises():
    with pytest.raises(ValueError):
        XGBClassifier(eval_metric="aucpr")
    X, y = planted(200, 1)
    with pytest.raises(ValueError):
        XGBClassifier(n_estimators=2, eval_metric="mlogloss").fit(X, y)
    with pytest.raises(ValueError):
        XGBClassifier(n_estimators=2, eval_metric="logloss").fit(*planted(200, 1, 3))


@pytest.mark.parametrize("classes", [2, 3])
def test_default_metric_is_unchanged(classes):
    (X, y), ev = planted(300, 1, classes), planted(150, 2, classes)
    name = "logloss" if classes == 2 else "mlogloss"
    fits = [XGBClassifier(n_estimators=8, max_depth=3, **kw).fit(X, y, eval_set=[ev], early_stopping_rounds=3)
            for kw in ({}, {"eval_metric": None}, {"eval_metric": name})]
    old = fits[0]
    del old.__dict__["eval_metric"]  # a model pickled before the argument existed
    assert old._metric_name() == name
    for clf in fits[1:]:
        assert clf.evals_result_ == old.evals_result_ and clf.best_iteration == old.best_iteration
        assert all(np.array_equal(a, b) for t, u in zip(clf._trees, old._trees) for a, b in zip(t, u))
