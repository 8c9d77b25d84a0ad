"""XGBRanker on the device (csrc/gbdt_rank.hip): the gradient kernels against the plain reference of
gbdt_rank_cases.py and the host function, and XGBRanker(device="gpu") against its host twin."""
import numpy as np
import pytest

import gbdt_rank_cases as C
from mifx.gbdt import XGBRanker, xgb

pytestmark = pytest.mark.gpu


def _device_grad(objective, margin, y, gptr, topk=0, u8=False, **geometry):
    import torch

    from mifx.ops import gbdt_gpu as G
    from mifx.ops import gbdt_rank as R

    dev = G.device_for(0)
    assert R.max_group() == C.CAP
    plan = R.RankPlan(gptr, dev)
    g, h = (torch.full((len(y),), float("nan"), dtype=torch.float32, device=dev) for _ in range(2))
    yd = torch.from_numpy(y.astype(np.uint8) if u8 else y).to(dev)
    R.grad_hess_rank(objective, torch.from_numpy(margin).to(dev), yd, plan, g, h, topk, **geometry)
    return g.cpu().numpy(), h.cpu().numpy()


@pytest.mark.parametrize("objective", C.OBJECTIVES)
@pytest.mark.parametrize("topk", [0, 1, 3])
def test_device_gradients_within_the_derived_bound(objective, topk):
    margin, y, gptr = C.table()
    g, h = _device_grad(objective, margin, y, gptr, topk, u8=topk == 1)
    rg, rh, Ag, Ah = C.table_reference(objective, topk)
    assert np.isfinite(g).all() and np.isfinite(h).all() and (h[Ah > 0] > 0).all()
    assert C.within(g, rg, Ag).all() and C.within(h, rh, Ah).all()
    if topk == 0:  # k beyond every group is "all", bit for bit
        assert all(np.array_equal(a, b) for a, b in zip(_device_grad(objective, margin, y, gptr, C.CAP), (g, h)))


@pytest.mark.parametrize("objective", C.OBJECTIVES)
def test_equal_margins_exact_for_every_geometry(objective):
    margin, y, gptr = C.table()
    want = C.flat_reference(objective)
    for geometry in ({}, dict(_groups_per_wg=1, _threads=64)):
        got = _device_grad(objective, np.zeros_like(margin), y, gptr, **geometry)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    a = _device_grad(objective, margin, y, gptr, _groups_per_wg=4, _threads=256)
    b = _device_grad(objective, margin, y, gptr, _groups_per_wg=1, _threads=64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("policy", [{"max_depth": 2}, {"grow_policy": "lossguide", "max_leaves": 3, "max_depth": 0}])
@pytest.mark.parametrize("subsample", [1.0, 0.5])
def test_ranker_equals_host_twin(policy, subsample):
    import torch

    X, y, qid = C.planted()
    kw = dict(n_estimators=4, subsample=subsample, random_state=1, **policy)
    fit = dict(qid=qid, eval_set=[(X, y)], eval_qid=[qid])
    a = XGBRanker(device="gpu", **kw).fit(X, y, **fit)
    b = XGBRanker(device="cpu", fixed_point=True, **kw).fit(X, y, **fit)
    assert len(a._trees) == len(b._trees) == 4 and a._base_margin == b._base_margin == 0.0
    assert all(np.array_equal(p, q) for p, q in zip(a._trees[0] + a._node_stats[0], b._trees[0] + b._node_stats[0]))
    hist = a.evals_result_["validation_0"]["ndcg"]
    assert hist[0] == b.evals_result_["validation_0"]["ndcg"][0] and hist[-1] > hist[0]
    on_device = a.predict(torch.from_numpy(X).to("cuda:0"))
    assert np.array_equal(on_device.cpu().numpy(), a.predict(X))


@pytest.mark.parametrize("objective", C.OBJECTIVES)
def test_teacher_forced_rounds(objective):
    X, y, qid = C.planted()
    gptr = np.concatenate([[0], np.cumsum(np.bincount(qid))]).astype(np.int64)
    m = XGBRanker(n_estimators=4, max_depth=3, objective=objective, fixed_point=True).fit(X, y, qid=qid)
    for r in range(1, 5):
        margin = m._predict_trees(X, m._trees[:r], 0.0)
        g, h = _device_grad(objective, margin, y, gptr)
        hg, hh = xgb.rank_grad(objective, margin, y, gptr)
        _, _, Ag, Ah = C.reference(objective, margin, y, gptr)
        assert C.within(g, hg.astype(np.float64), Ag).all() and C.within(h, hh.astype(np.float64), Ah).all()


def test_group_above_cap_raises_before_any_launch():
    n = C.CAP + 1
    X = np.zeros((n, 2))
    with pytest.raises(ValueError, match=str(C.CAP)):
        XGBRanker(device="gpu", n_estimators=1).fit(X, np.zeros(n), group=[n])
