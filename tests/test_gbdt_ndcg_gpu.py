"""XGBRanker's eval metric ndcg / ndcg@k on the device (csrc/gbdt_ndcg.hip) against a plain per-group float64 loop of
its rule, bit for bit: the device evaluates no transcendental, and every operation is an IEEE double multiply, add or
divide in an order the rule fixes. Then XGBRanker(device="gpu") with and without the device metric: equal histories."""
import functools

import numpy as np
import pytest

import gbdt_rank_cases as C
from mifx.gbdt import XGBRanker, xgb

pytestmark = pytest.mark.gpu

CHUNK = 2048  # keys of the tiled route's LDS chunk
KS = (0, 1, 10, 64, 65, 10 ** 6)


@functools.lru_cache(maxsize=None)
def edges():
    """(margin, y, gptr): the sizes only the tiled route has -- one and two tiles (256, 257), the chunk and one more,
    one row beyond the gradient kernels' limit -- and a group of four tiles whose 65 largest margins, relevant and
    distinct, all sit at the end of its LAST tile, where an early exit under @k must not hide them."""
    rng = np.random.default_rng(11)
    sizes = [256, 257, CHUNK, CHUNK + 1, C.CAP + 1, 1000]
    margin = [np.round(rng.normal(size=m), 1) for m in sizes]  # one decimal: many ties
    y = [rng.integers(0, 5, m).astype(np.float64) for m in sizes]
    margin[-1][-65:] = 100.0 + rng.normal(size=65)
    y[-1][-65:] = rng.integers(1, 5, 65)
    gptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return np.concatenate(margin), np.concatenate(y), gptr


TABLES = {"table": C.table, "edges": edges}


@functools.lru_cache(maxsize=None)
def reference(which, k):
    """The groups' scores by the rule, one Python loop per group; their mean is cross-checked against xgb.ndcg."""
    margin, y, gptr = TABLES[which]()
    D = xgb.discount_tables(int(np.diff(gptr).max()))[0]
    bits = margin.view(np.uint64)
    key = np.where(bits >> np.uint64(63), ~bits, bits | np.uint64(1 << 63))
    out = np.ones(len(gptr) - 1)
    for q, (a, b) in enumerate(zip(gptr[:-1], gptr[1:])):
        gain = np.exp2(y[a:b]) - 1.0
        by_rank = np.lexsort((np.arange(b - a), ~key[a:b]))  # key descending, ties to the lower row
        by_label = np.argsort(-y[a:b], kind="stable")
        dcg = idcg = 0.0
        for r in range(b - a if k == 0 else min(k, b - a)):
            dcg, idcg = dcg + gain[by_rank[r]] * D[r], idcg + gain[by_label[r]] * D[r]
        if idcg > 0:
            out[q] = dcg / idcg
    assert float(np.mean(out)) == xgb.ndcg(margin, y, gptr, k)
    return out


def device_scores(which, k, **geometry):
    import torch

    from mifx.ops import gbdt_gpu as G
    from mifx.ops import gbdt_ndcg as N

    margin, y, gptr = TABLES[which]()
    dev = G.device_for(0)
    plan = N.NdcgPlan(gptr, y, k, dev)
    md = torch.from_numpy(margin).to(dev)[None]  # [1, m]: what fit passes
    got = plan.group_scores(md, **geometry).cpu().numpy()
    assert plan.score(md, **geometry) == float(np.mean(got))
    return got


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("which", list(TABLES))
def test_group_scores_bit_for_bit(which, k):
    want = reference(which, k)
    assert (which == "edges" or (want == 1.0).any()) and (want < 1.0).any()  # (a group of all-zero labels scores 1.0)
    assert np.array_equal(device_scores(which, k), want)


@pytest.mark.parametrize("k", [0, 10])
@pytest.mark.parametrize("which", list(TABLES))
def test_geometry_changes_no_bit(which, k):
    for groups_per_wg in (1, 2, 3, 4):
        for chunk in (512, CHUNK):
            got = device_scores(which, k, _groups_per_wg=groups_per_wg, _chunk=chunk)
            assert np.array_equal(got, reference(which, k)), (groups_per_wg, chunk)


def _fit(metric):
    X, y, qid = C.planted()
    ex, ey, eq = C.planted(4)
    fit = XGBRanker(device="gpu", n_estimators=5, max_depth=3, eval_metric=metric).fit(
        X, y, qid=qid, eval_set=[(ex, ey)], eval_qid=[eq], early_stopping_rounds=2)
    assert len(fit.evals_result_["validation_0"][metric]) >= 3
    return fit.evals_result_, fit.best_score, fit.best_iteration


def _refuse(*args, **kwargs):
    raise AssertionError("not on this path")


@pytest.mark.parametrize("metric", ["ndcg", "ndcg@3"])
def test_fit_scores_on_the_device_with_the_hosts_bits(metric, monkeypatch):
    with monkeypatch.context() as mp:
        mp.setattr(XGBRanker, "_metric", _refuse)  # the host metric is never called
        on_device = _fit(metric)
    monkeypatch.setattr(XGBRanker, "_device_metric", lambda self, ey, dev: None)
    assert on_device == _fit(metric)


def test_group_above_the_limit_takes_the_host_path(monkeypatch):
    from mifx.ops import gbdt_ndcg as N

    on_device = _fit("ndcg")
    monkeypatch.setattr(N, "max_group", lambda: 8)  # the planted groups hold up to 40 rows
    monkeypatch.setattr(N, "NdcgPlan", _refuse)
    assert _fit("ndcg") == on_device
