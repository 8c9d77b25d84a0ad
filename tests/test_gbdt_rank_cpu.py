"""XGBRanker on the host: mifx_gbdt_rank_grad against the plain reference of gbdt_rank_cases.py, the NDCG metric, the
argument checks, the direction of early stopping and learning on a planted problem."""
import numpy as np
import pytest

import gbdt_rank_cases as C
from mifx.gbdt import XGBRanker, xgb


@pytest.mark.parametrize("objective", C.OBJECTIVES)
@pytest.mark.parametrize("topk", [0, 1, 3])
def test_host_gradients_within_the_derived_bound(objective, topk):
    margin, y, gptr = C.table()
    g, h = xgb.rank_grad(objective, margin, y, gptr, topk, threads=4)
    rg, rh, Ag, Ah = C.table_reference(objective, topk)
    assert np.isfinite(g).all() and np.isfinite(h).all() and (h >= 0).all()
    assert C.within(g, rg, Ag).all() and C.within(h, rh, Ah).all()
    assert (h[(Ah > 0)] > 0).all()  # the hessian floor: a row with a pair never has h = 0, even where exp overflowed
    one = xgb.rank_grad(objective, margin, y, gptr, topk, threads=1)
    assert np.array_equal(one[0], g) and np.array_equal(one[1], h)


@pytest.mark.parametrize("objective", C.OBJECTIVES)
def test_host_equal_margins_exact_and_topk_beyond_the_group_is_all(objective):
    margin, y, gptr = C.table()
    g, h = xgb.rank_grad(objective, np.zeros_like(margin), y, gptr)
    rg, rh = C.flat_reference(objective)
    assert np.array_equal(g, rg) and np.array_equal(h, rh)
    a, b = xgb.rank_grad(objective, margin, y, gptr), xgb.rank_grad(objective, margin, y, gptr, topk=C.CAP)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_ndcg_by_hand():
    # group 0 ranks its labels 1, 2, 0 (ideal 2, 1, 0); group 1 holds no relevant row and scores 1
    margin, y, gptr = np.array([3.0, 2.0, 1.0, 0.5, 0.1]), np.array([1.0, 2.0, 0.0, 0.0, 0.0]), np.array([0, 3, 5])
    d = 1.0 / np.log2([2.0, 3.0])
    assert xgb.ndcg(margin, y, gptr) == pytest.approx(((1 * d[0] + 3 * d[1]) / (3 * d[0] + 1 * d[1]) + 1.0) / 2, 1e-15)
    assert xgb.ndcg(margin, y, gptr, k=1) == pytest.approx((1.0 / 3.0 + 1.0) / 2, 1e-15)
    assert xgb.ndcg(np.array([0.0, -0.0]), np.array([0.0, 1.0]), np.array([0, 2])) == pytest.approx(d[1], 1e-15)


def test_argument_errors():
    X, y, qid = C.planted()
    bad = [dict(qid=qid[::-1].copy()), dict(), dict(qid=qid, group=[len(y)]), dict(qid=qid, sample_weight=np.ones(len(y))),
           dict(qid=qid, eval_set=[(X, y)]), dict(group=[len(y) - 1])]
    for kw in bad:
        with pytest.raises(ValueError):
            XGBRanker(n_estimators=1).fit(X, y, **kw)
    for labels in (y + 0.5, y - 1.0, y + 30.0):
        with pytest.raises(ValueError):
            XGBRanker(n_estimators=1).fit(X, labels, qid=qid)
    for kw in (dict(objective="rank:map"), dict(lambdarank_pair_method="mean"), dict(lambdarank_pair_method="topk"),
               dict(lambdarank_num_pair_per_sample=2), dict(eval_metric="map")):
        with pytest.raises(ValueError):
            XGBRanker(**kw)


def test_early_stopping_maximises_ndcg():
    X, y, qid = C.planted()
    ev = dict(eval_set=[(X, y)], eval_qid=[qid])
    m = XGBRanker(n_estimators=30, max_depth=1, learning_rate=0.5).fit(X, y, qid=qid, early_stopping_rounds=3, **ev)
    hist = m.evals_result_["validation_0"]["ndcg"]
    assert m.best_score == max(hist) and m.best_iteration == int(np.argmax(hist)) > 0
    assert len(hist) == min(30, m.best_iteration + 4)  # stopped three rounds after the LARGEST score


@pytest.mark.parametrize("objective", C.OBJECTIVES)
def test_host_twin_learns_the_planted_order(objective):
    """Depth-1 trees cut one label step per round, so the first round cannot order five grades. Measured on the host:
    NDCG 0.8899 after round 1 and 0.9890 (rank:ndcg) / 1.0 (rank:pairwise) after round 10."""
    X, y, qid = C.planted()
    m = XGBRanker(n_estimators=10, max_depth=1, objective=objective, fixed_point=True)
    hist = m.fit(X, y, qid=qid, eval_set=[(X, y)], eval_group=[np.bincount(qid)]).evals_result_["validation_0"]["ndcg"]
    assert hist[9] > hist[0]
    assert np.array_equal(m.predict(X), m._predict_trees(X, m._trees, 0.0))
