"""reg:absoluteerror / reg:quantileerror on the device (csrc/gbdt_quantile.hip): the leaf refresh against the plain
reference of gbdt_quantile_cases.py and the host function, and XGBRegressor(device="gpu") against its host twin --
exact equality throughout."""
import numpy as np
import pytest

import gbdt_quantile_cases as Q
from mifx.gbdt import XGBRegressor, xgb

pytestmark = pytest.mark.gpu


def _device_refresh(resid, h, leaf, value, alpha, rows_per_wg, repeat=1):
    import torch

    from mifx.ops import gbdt_gpu as G

    dev = G.device_for(0)
    refresh = G.LeafRefresh(len(resid), len(value), dev, _rows_per_wg=rows_per_wg)
    y = torch.from_numpy(resid).to(dev)  # y - 0.0 is the residual, signed zeros included
    margin = torch.zeros(len(resid), dtype=torch.float64, device=dev)
    out = []
    for _ in range(repeat):  # a second call on the same workspace starts from cleared counters
        v = torch.from_numpy(value).to(dev)
        refresh(torch.from_numpy(leaf).to(dev), v, margin, y, torch.from_numpy(h).to(dev), alpha, Q.ETA)
        out.append(v.cpu().numpy())
    return out


@pytest.mark.parametrize("name", list(Q.CASES))
def test_device_refresh_equals_reference_and_host(name):
    resid, h, leaf, value, alpha, rows_per_wg = Q.CASES[name]
    first, second = _device_refresh(resid, h, leaf, value, alpha, rows_per_wg, repeat=2)
    host = value.copy()
    xgb.leaf_refresh(resid, h, leaf, host, alpha, Q.ETA)
    want = Q.bits(Q.reference_refresh(resid, h, leaf, value, alpha))
    assert np.array_equal(Q.bits(first), want) and np.array_equal(Q.bits(second), want)
    assert np.array_equal(Q.bits(host), want)


def test_chunking_changes_no_bit():
    resid, h, leaf, value, alpha, _ = Q.CASES["chunked"]
    got = [_device_refresh(resid, h, leaf, value, alpha, r)[0] for r in (64, 512, 1000, None)]
    assert all(np.array_equal(Q.bits(g), Q.bits(got[0])) for g in got)


@pytest.mark.parametrize("objective,alpha", [("reg:absoluteerror", 0.5), ("reg:quantileerror", 0.9)])
@pytest.mark.parametrize("policy", [{"max_depth": 4}, {"grow_policy": "lossguide", "max_leaves": 12, "max_depth": 0}])
@pytest.mark.parametrize("sampled", [False, True])
def test_regressor_equals_host_twin(objective, alpha, policy, sampled):
    rng = np.random.default_rng(11)
    X = rng.normal(size=(2000, 8))
    X[rng.random(X.shape) < 0.03] = np.nan
    y = np.nan_to_num(X[:, 0]) * 2.0 + rng.standard_exponential(2000) * (1.0 + (np.nan_to_num(X[:, 1]) > 0))
    w = rng.uniform(0.0, 2.0, 2000).astype(np.float32) if sampled else None
    stop = sampled and "max_leaves" in policy  # one case with an eval set and early stopping
    kw = dict(n_estimators=30 if stop else 5, learning_rate=0.3, objective=objective, quantile_alpha=alpha,
              subsample=0.5 if sampled else 1.0, random_state=2, **policy)
    fit = dict(sample_weight=w, **(dict(eval_set=[(X[:300], y[:300] + rng.normal(size=300) * 3)],
                                        early_stopping_rounds=2) if stop else {}))
    a = XGBRegressor(device="gpu", **kw).fit(X, y, **fit)
    b = XGBRegressor(device="cpu", fixed_point=True, **kw).fit(X, y, **fit)
    assert len(a._trees) == len(b._trees) >= 3 and a._base_margin == b._base_margin
    for ta, tb in zip(a._trees, b._trees):
        assert all(np.array_equal(p, q) for p, q in zip(ta[:5], tb[:5]))
        assert np.array_equal(Q.bits(ta[5]), Q.bits(tb[5]))
    assert a.best_iteration == b.best_iteration and a.evals_result_ == b.evals_result_
    assert np.array_equal(Q.bits(a.predict(X)), Q.bits(b.predict(X)))
