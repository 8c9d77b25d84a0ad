"""reg:absoluteerror / reg:quantileerror on the host learners: mifx_gbdt_leaf_refresh and every fitted tree's leaf values
against the plain reference of gbdt_quantile_cases.py (exact equality), the metrics, the errors, and one coverage check."""
import numpy as np
import pytest

import gbdt_quantile_cases as Q
from mifx.gbdt import XGBClassifier, XGBRegressor, xgb


@pytest.mark.parametrize("name", list(Q.CASES))
def test_host_refresh_equals_reference(name):
    resid, h, leaf, value, alpha, _ = Q.CASES[name]
    got = value.copy()
    xgb.leaf_refresh(resid, h, leaf, got, alpha, Q.ETA, threads=3)
    assert np.array_equal(Q.bits(got), Q.bits(Q.reference_refresh(resid, h, leaf, value, alpha)))


def _data(n=600, f=5, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, f))
    X[rng.random((n, f)) < 0.05] = np.nan
    y = np.nan_to_num(X[:, 0]) + rng.standard_exponential(n) * (1.0 + (np.nan_to_num(X[:, 1]) > 0))
    return X, y, rng.uniform(0.0, 2.0, n).astype(np.float32)


def _walk(tree, X):
    """the leaf id of every row"""
    fe, thr, dl, le, ri, _ = tree
    k = np.zeros(len(X), np.int64)
    for _ in range(len(fe)):
        x = X[np.arange(len(X)), np.maximum(fe[k], 0)]
        left = np.where(np.isnan(x), dl[k] != 0, x < thr[k])
        k = np.where(fe[k] >= 0, np.where(left, le[k], ri[k]), k)
    return k


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("objective,alpha", [("reg:absoluteerror", 0.5), ("reg:quantileerror", 0.8)])
@pytest.mark.parametrize("extra", [{}, {"subsample": 0.5, "grow_policy": "lossguide", "max_leaves": 6, "max_depth": 0}])
def test_fitted_leaves_are_the_reference_quantiles(fixed, objective, alpha, extra):
    X, y, w = _data()
    kw = dict(n_estimators=4, max_depth=3, learning_rate=Q.ETA, objective=objective, quantile_alpha=alpha,
              random_state=5) | extra
    m = XGBRegressor(device="cpu" if fixed else None, fixed_point=fixed or None, **kw)
    m.fit(X, y, eval_set=[(X[:100], y[:100])], sample_weight=w if extra else None)
    h = w if extra else np.ones(len(y), np.float32)
    margin = np.full(len(y), m._base_margin)
    order = np.argsort(y, kind="stable")  # the intercept: the lower weighted quantile of y
    cum = np.cumsum(h[order].astype(np.float64))
    assert m._base_margin == y[order[np.searchsorted(cum, alpha * cum[-1])]]
    for t, tree in enumerate(m._trees):
        leaf = _walk(tree, X).astype(np.int32)
        if extra:
            keep = np.zeros(len(y), bool)
            keep[xgb.sample_rows(5, t, 0.5, len(y))] = True
            leaf[~keep] = -1
        want = Q.reference_refresh(y - margin, h, leaf, tree[5], alpha)
        assert np.array_equal(Q.bits(tree[5]), Q.bits(want)), t
        assert len(np.unique(leaf[leaf >= 0])) > 1
        margin = margin + tree[5][_walk(tree, X)]
    assert np.array_equal(m.predict(X), margin)
    name = "mae" if objective == "reg:absoluteerror" else "quantile"
    hist = m.evals_result_["validation_0"][name]
    r = y[:100] - margin[:100]
    want = np.mean(np.abs(r)) if name == "mae" else np.mean(np.maximum(alpha * r, (alpha - 1.0) * r))
    assert len(hist) == 4 and hist[-1] == want


@pytest.mark.parametrize("kw,match", [
    ({"objective": "reg:pseudohubererror"}, "reg:squarederror.*reg:absoluteerror.*reg:quantileerror"),
    ({"objective": "reg:absoluteerror", "quantile_alpha": 0.3}, "reg:quantileerror"),
    ({"objective": "reg:quantileerror", "quantile_alpha": [0.1, 0.9]}, "multi-quantile models are not implemented"),
    ({"objective": "reg:quantileerror", "quantile_alpha": 1.0}, r"\(0, 1\)"),
])
def test_bad_arguments_raise(kw, match):
    with pytest.raises(ValueError, match=match):
        XGBRegressor(**kw)


def test_classifier_takes_no_objective_and_old_pickles_are_squared_error():
    with pytest.raises(TypeError):
        XGBClassifier(objective="reg:absoluteerror")
    m = XGBRegressor(objective="reg:absoluteerror")
    del m.__dict__["objective"], m.__dict__["quantile_alpha"]  # a model pickled before the arguments existed
    assert m._objective == "reg:squarederror" and m._refresh_alpha() is None and m._metric_name() == "rmse"


def test_interval_covers_its_share_of_rows():
    """y = x0 + heteroscedastic noise, 4000 rows: the share of training rows below the 0.1 / 0.9 models. The host
    learner gives 0.099 and 0.900 here; a quantile model that works stays within 0.04 of its alpha (the leaves are
    exact in-sample quantiles of the last residuals; the rows then move by 0.3 of them), one that ignores alpha is
    0.4 away."""
    rng = np.random.default_rng(0)
    X = rng.normal(size=(4000, 4))
    y = X[:, 0] + rng.normal(size=4000) * (0.5 + 0.5 * (X[:, 1] > 0))
    for alpha in (0.1, 0.9):
        m = XGBRegressor(n_estimators=40, max_depth=3, objective="reg:quantileerror", quantile_alpha=alpha).fit(X, y)
        share = float(np.mean(y < m.predict(X)))
        print(f"alpha {alpha}: share below the prediction {share:.4f}")
        assert abs(share - alpha) < 0.04
