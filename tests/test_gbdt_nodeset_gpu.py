"""interaction_constraints and colsample_bynode on the device growers (k_nodeset and the per-node masks of
csrc/gbdt_gpu.hip and csrc/gbdt_lossguide.hip, the wave's work in csrc/gbdt_nodeset.h) against the fixed-point host
twins: the trees and node statistics of every round, bit for bit. f crosses a wave's lanes, a 64-bit word and the
histogram's feature tile; the groups overlap, span a word boundary and leave features out."""
import numpy as np
import pytest

from mifx.gbdt import XGBClassifier, XGBRegressor

pytestmark = pytest.mark.gpu

POLICIES = [dict(max_depth=4), dict(grow_policy="lossguide", max_leaves=8, max_depth=0)]
SHAPES = [(3, 300), (13, 5000), (65, 300), (130, 5000)]


def table(f, n, missing_last=False):
    """[n, f] with ~5 % NaN; y mixes products of features that share a group, products that no group allows and single
    features, so the constraints bind at every depth."""
    r = np.random.default_rng(f + n)
    X = r.normal(size=(n, f))
    y = X[:, 0] * X[:, 1 % f] + X[:, f // 2] * X[:, f - 1] + X[:, 2 % f] * X[:, f // 3] + 0.5 * X[:, f - 2]
    if f > 64:
        y += X[:, 60] * X[:, 64] + X[:, 59]
    X[r.random(X.shape) < 0.05] = np.nan
    if missing_last:
        X[:, -1] = np.nan
    return X, y


def groups_for(f):
    """Overlapping groups (feature f // 2 fits two), a run that crosses bit 63 / 64 and one that ends at the last
    feature (a word boundary of its own at f = 130); features 2 and 3 are in no group when f >= 13."""
    runs = [[0, 1 % f, f // 2], [f // 2, f - 1], list(range(58, min(f, 70))), list(range(max(4, f - 9), f))]
    return [g for g in runs if g]


def same_models(a, b):
    assert a.n_trees_ == b.n_trees_ > 0 and max(len(t[0]) for t in a._trees) > 3
    for t in range(a.n_trees_):
        for u, v in zip(a._trees[t] + a._node_stats[t], b._trees[t] + b._node_stats[t]):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"tree {t}"


@pytest.mark.parametrize("mono,subsample", [(False, 1.0), (True, 0.5)])
@pytest.mark.parametrize("constrained,rate", [(True, 1.0), (True, 0.5), (False, 0.5)])
@pytest.mark.parametrize("policy", POLICIES, ids=["depthwise", "lossguide"])
@pytest.mark.parametrize("f,n", SHAPES)
def test_model_equals_the_host_twin(f, n, policy, constrained, rate, mono, subsample):
    X, y = table(f, n)
    kw = dict(n_estimators=3, subsample=subsample, colsample_bynode=rate, colsample_bytree=0.9 if mono else 1.0,
              interaction_constraints=groups_for(f) if constrained else None,
              monotone_constraints=[(1, -1, 0)[j % 3] for j in range(f)] if mono else None, **policy)
    same_models(XGBRegressor(device="gpu", **kw).fit(X, y), XGBRegressor(device="cpu", fixed_point=True, **kw).fit(X, y))


def test_colsample_bylevel_is_the_level_set_and_a_missing_only_feature_never_splits():
    X, y = table(13, 300, missing_last=True)
    kw = dict(n_estimators=3, max_depth=4, colsample_bylevel=0.7, colsample_bynode=0.5,
              interaction_constraints=groups_for(13))
    a = XGBRegressor(device="gpu", **kw).fit(X, y)
    same_models(a, XGBRegressor(device="cpu", fixed_point=True, **kw).fit(X, y))
    assert all((t[0] != 12).all() for t in a._trees)


@pytest.mark.parametrize("policy", POLICIES, ids=["depthwise", "lossguide"])
def test_multiclass_draws_are_keyed_by_the_tree_index(policy):
    X, y = table(13, 300)
    lab = np.digitize(y, np.quantile(y, [1 / 3, 2 / 3]))
    kw = dict(n_estimators=2, colsample_bynode=0.5, interaction_constraints=groups_for(13), **policy)
    a = XGBClassifier(device="gpu", **kw).fit(X, lab)
    same_models(a, XGBClassifier(device="cpu", fixed_point=True, **kw).fit(X, lab))
    assert a.n_trees_ == 6
