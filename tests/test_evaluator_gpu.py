"""The Evaluator's GPU path (mifx.evaluator.metrics.compute_sliced_metrics(device="cuda")) against the same metrics
computed from the host segment_hist: one segmented reduction per slice spec at HIST_BUCKETS = 10000 buckets.

Which kernel path a case reaches (csrc/analyzers.hip segment_hist_k): the overall slice is ns = 1, nb = 10000 ->
20000 bins in an 80 KB dynamic LDS table (above 64 KB, so behind hipFuncSetAttribute); one slicing column of three
values is ns = 3 -> 60000 bins, the global-atomic path.

The reference -- binary_metrics_from_hist over the host segment_hist -- is pinned on the CPU against the per-row
binary_metrics (test_hist_metrics_match_row_metrics); the host segment_hist itself against a per-row loop in
tests/test_analyzers_gpu.py."""
import functools

import numpy as np
import pytest

from mifx.evaluator import metrics as M
from mifx.ops import analyzers as an

EXACT = ("example_count", "accuracy", "auc", "precision", "recall", "label/mean")
CLOSE = ("average_loss", "prediction/mean", "calibration")  # from fp64 atomics in arbitrary order: 1e-9 relative


@functools.lru_cache(maxsize=None)
def _data(n=30_000):
    r = np.random.default_rng(21)
    y = (r.random(n) < 0.25).astype(np.float32)
    p = np.clip(r.normal(0.3 + 0.3 * y, 0.2), -0.05, 1.05).astype(np.float32)  # some clipped at both ends
    k = np.arange(40)
    p[:40] = (k * 250 / M.HIST_BUCKETS).astype(np.float32)  # on bucket edges
    p[40:44] = [0.0, 1.0, 1e-7, 0.75]
    hour = np.array([3, 12, 19])[r.integers(0, 3, n)]
    return y, p, hour


def _expected(y, p, seg, ns):
    sums, hist = an.segment_hist(seg, y, p, ns, M.HIST_BUCKETS, device=None)
    return [M.binary_metrics_from_hist(sums[i], hist[i]) for i in range(ns)]


def test_hist_metrics_match_row_metrics():
    """binary_metrics_from_hist(host segment_hist) against the per-row binary_metrics: counts, accuracy, precision,
    recall and label mean are the same numbers; loss and prediction mean the same sums in another order. The bucketed
    AUC treats the pairs inside one bucket as ties, so it is within sum_b pos_b neg_b / (2 npos nneg) of the rank AUC.
    (No probability is exactly 0.5 here: precision / recall count bucket nb / 2 as predicted positive, accuracy and
    the per-row metrics use p > 0.5.)"""
    y, p, _ = _data()
    y, p = y[44:5044], p[44:5044]
    assert not (p == 0.5).any()
    seg = np.zeros(y.size, np.int32)
    sums, hist = an.segment_hist(seg, y, p, 1, M.HIST_BUCKETS, device=None)
    got = M.binary_metrics_from_hist(sums[0], hist[0])
    pc = np.clip(p, 1e-7, 1 - 1e-7)  # float32, as segment_hist clips
    want = M.binary_metrics(y, pc)
    for k in ("example_count", "precision", "recall", "label/mean"):
        assert got[k] == want[k], k
    for k in ("accuracy", "average_loss", "prediction/mean", "calibration"):
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    neg, pos = hist[0, :, 0].astype(np.float64), hist[0, :, 1].astype(np.float64)
    bound = 0.5 * (pos * neg).sum() / (pos.sum() * neg.sum())
    assert 0 < bound < 1e-3 and abs(got["auc"] - want["auc"]) <= bound + 1e-12


def _check(res, spec_key, slices, want):
    got = [s for s in res.slices if s["spec"] == spec_key]
    assert [s["slice"] for s in got] == slices
    for s, w in zip(got, want):
        g = s["metrics"]
        assert set(g) == set(w)
        for k in EXACT:
            assert g[k] == w[k], (s["slice"], k)
        for k in CLOSE:
            assert g[k] == pytest.approx(w[k], rel=1e-9, abs=0), (s["slice"], k)


@pytest.mark.gpu
def test_overall_slice_is_the_80kb_lds_table():
    """Default spec: ns = 1, nb = 10000, segment_hist_k's LDS path at the Evaluator's own size."""
    y, p, hour = _data()
    res = M.compute_sliced_metrics(y, p, {"hour": hour}, device="cuda")
    want = _expected(y, p, np.zeros(y.size, np.int32), 1)
    assert len(res.slices) == 1
    _check(res, "Overall", [[]], want)
    assert res.overall()["example_count"] == y.size and 0.5 < res.overall()["auc"] < 1.0


@pytest.mark.gpu
def test_one_slicing_column_of_three_values():
    """One slicing column with 3 values: the overall slice again (LDS path) plus ns = 3, nb = 10000 -> 60000 bins on
    the global-atomic path; the slices come out in sorted value order, each equal to the host reduction of its
    rows."""
    y, p, hour = _data()
    res = M.compute_sliced_metrics(y, p, {"hour": hour}, [M.SliceSpec(columns=["hour"])], device="cuda")
    assert len(res.slices) == 4
    _check(res, "Overall", [[]], _expected(y, p, np.zeros(y.size, np.int32), 1))
    seg = np.searchsorted([3, 12, 19], hour).astype(np.int32)
    want = _expected(y, p, seg, 3)
    _check(res, "hour", [[["hour", 3]], [["hour", 12]], [["hour", 19]]], want)
    assert sum(w["example_count"] for w in want) == y.size
