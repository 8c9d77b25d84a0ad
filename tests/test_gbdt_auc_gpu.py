"""eval_metric="auc" on the device (csrc/gbdt_auc.hip): the integer pair counts against the numpy pair loop of
test_gbdt_auc_cpu.py, and XGBClassifier(device="gpu", eval_metric="auc") against its host twin. Exact equality only."""
import numpy as np
import pytest

from mifx.gbdt import XGBClassifier
from test_gbdt_auc_cpu import LABEL_SETS, MARGIN_SETS, make_case, pair_loop, planted

pytestmark = pytest.mark.gpu


def device_counts(margin, y, K=1, group=None, **geometry):
    """[(U2, P, N)] per class from the device, as Python ints"""
    import torch

    from mifx.ops import gbdt_auc as A
    from mifx.ops import gbdt_gpu as G

    dev = G.device_for(0)
    plan = A.AucPlan(y, K, dev, _group=group)
    md = torch.from_numpy(np.ascontiguousarray(margin, np.float64).reshape(K, -1)).to(dev)
    first = plan.counts(md, **geometry)
    assert np.array_equal(plan.counts(md, **geometry), first)  # the counters are cleared by every call
    return [(int(u), int(p), int(n)) for u, p, n in zip(first, plan.P, plan.N)]


@pytest.mark.parametrize("margins", MARGIN_SETS)
@pytest.mark.parametrize("m", [2, 65, 257, 3000])
def test_device_counts_equal_the_pair_loop(m, margins):
    for labels in LABEL_SETS:
        x, y = make_case(m, margins, labels)
        assert device_counts(x, y) == [pair_loop(x, y == 1.0)], labels


@pytest.mark.parametrize("negatives", [1, 63, 64, 65])
def test_tile_boundaries(negatives):
    """A private tile of 64 positives: one short of a tile, a whole one, one more, and several with a short last one,
    against 1, 63, 64 and 65 negatives (an eval set of a single row has one class only and is refused)."""
    rng = np.random.default_rng(negatives)
    for positives in (63, 64, 65, 3 * 64 + 17):
        y = rng.permutation(np.repeat([0.0, 1.0], [negatives, positives]))
        x = np.round(rng.standard_normal(len(y)), 1)  # (rounded: ties inside and across the tiles)
        assert device_counts(x, y, _tile=64) == [pair_loop(x, y == 1.0)], positives
    with pytest.raises(ValueError):
        device_counts(np.zeros(1), np.ones(1))


@pytest.mark.parametrize("margins", ["normal", "ties"])
def test_span_over_several_chunks_and_two_geometries(margins):
    x, y = make_case(3000, margins, "mixed", seed=1)
    want = [pair_loop(x, y == 1.0)]
    assert device_counts(x, y) == want
    assert device_counts(x, y, _tile=100, _threads=64, _chunk=96) == want  # spans of about 150 negatives and far more


@pytest.mark.parametrize("group", [None, 2])
def test_three_classes(group):
    rng = np.random.default_rng(5)
    y = rng.integers(0, 3, 700).astype(np.float64)
    x = np.round(rng.standard_normal((3, 700)), 1) + (y == np.arange(3.0)[:, None])
    assert device_counts(x, y, K=3, group=group, _tile=128) == [pair_loop(x[k], y == k) for k in range(3)]


@pytest.mark.parametrize("classes", [2, 3])
def test_teacher_forced_scores_equal_the_host(classes):
    import torch

    from mifx.ops import gbdt_auc as A
    from mifx.ops import gbdt_gpu as G

    (X, y), (ex, ey) = planted(500, 1, classes), planted(333, 2, classes)
    clf = XGBClassifier(n_estimators=6, max_depth=3, eval_metric="auc", fixed_point=True).fit(X, y, eval_set=[(ex, ey)])
    K, dev = clf._num_class(), G.device_for(0)
    plan = A.AucPlan(ey.astype(np.float64), K, dev)
    for it, score in enumerate(clf.evals_result_["validation_0"]["auc"]):
        trees = clf._trees[:(it + 1) * K]
        margin = np.stack([clf._predict_trees(ex, trees[k::K], clf._base_margin) for k in range(K)])
        assert plan.score(torch.from_numpy(margin).to(dev), _tile=64) == score


@pytest.mark.parametrize("classes", [2, 3])
def test_gpu_fit_against_the_host_twin(classes):
    (X, y), ev = planted(800, 1, classes), planted(400, 2, classes)
    kw = dict(n_estimators=40, max_depth=3, learning_rate=0.5, eval_metric="auc")
    gpu = XGBClassifier(device="gpu", **kw).fit(X, y, eval_set=[ev], early_stopping_rounds=4)
    cpu = XGBClassifier(device="cpu", fixed_point=True, **kw).fit(X, y, eval_set=[ev], early_stopping_rounds=4)
    hist = gpu.evals_result_["validation_0"]["auc"]
    assert hist[0] == cpu.evals_result_["validation_0"]["auc"][0]
    assert max(hist) > hist[0] > 0.5
    assert gpu.best_iteration == int(np.argmax(hist)) and gpu.best_score == max(hist)
