"""monotone_constraints on the device growers (k_split_mono / k_decide_mono of csrc/gbdt_gpu.hip, k_split_mono of
csrc/gbdt_lossguide.hip) against the host twins mifx_gbdt_grow_fixed_mono / mifx_gbdt_grow_fixed_lossguide_mono: bit for
bit, for any launch geometry; then the models, and the promise on device predictions."""
import numpy as np
import pytest
import torch

import gbdt_monotone_cases as M
from mifx.gbdt import XGBClassifier, XGBRanker, XGBRegressor, xgb

pytestmark = pytest.mark.gpu

POLICIES = [dict(max_depth=2), dict(max_depth=6), dict(grow_policy="lossguide", max_leaves=8, max_depth=0)]
NAMES = ("feature", "split_bin", "default_left", "left", "right", "value", "leaf_of_row", "gain", "cover")


def twin(bins, nbins, g, h, mono, depth, leaves=0, lam=1.0, gamma=0.0):
    """The nine arrays of NAMES from the host twin (leaves > 0: the leaf-wise one)."""
    (f, n), cap, p, lib = bins.shape, (2 * leaves - 1 if leaves else 2 ** (depth + 1)), xgb._p, xgb._lib()
    fe, sb, le, ri = (np.empty(cap, np.int32) for _ in range(4))
    dl, val, leaf = np.empty(cap, np.uint8), np.empty(cap, np.float64), np.empty(n, np.int32)
    gain, cover = np.empty(cap, np.float64), np.empty(cap, np.float64)
    fn = lib.mifx_gbdt_grow_fixed_lossguide_mono if leaves else lib.mifx_gbdt_grow_fixed_mono
    cnt = fn(p(bins, xgb._U16), n, f, p(nbins, xgb._I), p(g, xgb._F), p(h, xgb._F), depth, *([leaves] if leaves else []),
             1.0, lam, gamma, 0.3, 1, cap, p(fe, xgb._I), p(sb, xgb._I), p(dl, xgb._U8), p(le, xgb._I), p(ri, xgb._I),
             p(val, xgb._D), p(leaf, xgb._I), None, 0, None, p(gain, xgb._D), p(cover, xgb._D),
             p(np.asarray(mono, np.int32), xgb._I))
    assert cnt > 0
    return tuple(a[:cnt].copy() for a in (fe, sb, dl, le, ri, val)) + (leaf, gain[:cnt].copy(), cover[:cnt].copy())


def device(bins, nbins, g, h, mono, depth, leaves=0, lam=1.0, gamma=0.0, **geo):
    from mifx.ops import gbdt_gpu as G

    if leaves:
        return G.grow_lossguide_numpy(bins, nbins, g, h, depth, leaves, 1.0, lam, gamma, 0.3, monotone=mono, **geo)
    return G.grow_numpy(bins, nbins, g, h, depth, 1.0, lam, gamma, 0.3, stats=True, monotone=mono, **geo)


def same(got, want, what):
    assert len(got[0]) == len(want[0]), f"{what}: node count {len(got[0])} against {len(want[0])}"
    for name, x, y in zip(NAMES, got, want):
        assert np.array_equal(x, y), f"{what}: {name} differs"


def edge_bins(n=3000, seed=2):
    """Bin counts 1, 2, 4, 5 (a lane's run boundary), 255, 256 (the wave's last lane) and 64 without a missing row;
    the gradient follows features 4 and 6 up and down, so constrained candidates are rejected and weights clamped."""
    r = np.random.default_rng(seed)
    nbins = np.array([1, 2, 4, 5, 255, 256, 64], np.int32)
    bins = np.stack([r.integers(0, nb, n) for nb in nbins]).astype(np.uint16)
    bins[:6][r.random((6, n)) < 0.1] = 0xFFFF
    g = np.sin(bins[4] / 20.0) + np.cos(bins[6] / 8.0) + bins[3] / 4.0 - bins[5] / 100.0 + r.normal(0, 0.3, n)
    return bins, nbins, g.astype(np.float32), r.uniform(0.5, 1.0, n).astype(np.float32)


@pytest.mark.parametrize("geo", [{}, dict(_rows_per_wg=64, _feat_tile=1), dict(_rows_per_wg=256, _feat_tile=12)])
@pytest.mark.parametrize("depth,leaves", [(2, 0), (6, 0), (0, 8), (5, 40)])
def test_grower_equals_host_twin_at_the_split_kernel_edges(depth, leaves, geo):
    bins, nbins, g, h = edge_bins()
    mono = [1, -1, 1, -1, 1, -1, -1]
    want = twin(bins, nbins, g, h, mono, depth, leaves)
    free = twin(bins, nbins, g, h, [0] * 6 + [1], depth, leaves)
    assert len(want[0]) > 3 and not np.array_equal(want[5], free[5])  # the constraints bind
    same(device(bins, nbins, g, h, mono, depth, leaves, **geo), want, f"{geo}")


@pytest.mark.parametrize("leaves", [0, 16])
def test_rejected_features_and_point_intervals(leaves):
    """(a) g falls with the bin of feature 0, so the weight rises: under -1 every candidate of it is rejected, and the
    node falls to feature 1 or, alone, turns leaf. (b) lambda 0 and gamma -1: a node whose raw weight lies above its
    interval still splits (both children clamp to the bound, gain 1) and hands its right child the interval [m, m]."""
    r = np.random.default_rng(4)
    b0 = r.integers(0, 8, 500).astype(np.uint16)
    bins, nbins = np.stack([b0, r.integers(0, 8, 500).astype(np.uint16)]), np.array([8, 8], np.int32)
    g, h = (-8.0 * b0 + (bins[1] % 3)).astype(np.float32), np.ones(500, np.float32)
    want = twin(bins, nbins, g, h, [-1, 0], 3, leaves, lam=0.0)  # (lambda 0: a weight is its rows' mean)
    assert len(want[0]) > 1 and (want[0] != 0).all()
    same(device(bins, nbins, g, h, [-1, 0], 3, leaves, lam=0.0), want, "falls to the next feature")
    want = twin(bins[:1], nbins[:1], g, h, [-1], 3, leaves, lam=0.0)
    assert len(want[0]) == 1
    same(device(bins[:1], nbins[:1], g, h, [-1], 3, leaves, lam=0.0), want, "turns leaf")
    # (b) feature 0 in {0 .. 3} under +1, feature 1 in {0, 1, 2} free: 400 rows at y = 1000 right of the root's cut, left
    # of it 100 rows at 0 (feature 1 = 0) and 8 rows near 2000 (feature 1 in {1, 2}), far above the root's midpoint
    f0 = np.r_[np.repeat([2, 3], 200), np.repeat([0, 1], 50), np.repeat([0, 1], 4)].astype(np.uint16)
    f1 = np.r_[np.zeros(500, int), np.tile([1, 2], 4)].astype(np.uint16)
    y = np.r_[np.full(400, 1000.0), np.zeros(100), 2000.0 + 10 * np.arange(8)]
    bins, nbins, g, h = np.stack([f0, f1]), np.array([4, 3], np.int32), (-y).astype(np.float32), np.ones(508, np.float32)
    want = twin(bins, nbins, g, h, [1, 0], 5, leaves, lam=0.0, gamma=-1.0)
    values, counts = np.unique(want[5][want[0] < 0], return_counts=True)
    assert counts.max() >= 3 and 0 < values[counts.argmax()] < 0.3 * 1000  # several leaves sit on one clamped bound
    same(device(bins, nbins, g, h, [1, 0], 5, leaves, lam=0.0, gamma=-1.0), want, "point interval")


def _same_models(a, b, trees):
    assert a.n_trees_ >= trees and b.n_trees_ >= trees
    for t in range(trees):
        for u, v in zip(a._trees[t] + a._node_stats[t], b._trees[t] + b._node_stats[t]):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"tree {t}"


@pytest.mark.parametrize("subsample", [1.0, 0.5])
@pytest.mark.parametrize("policy", POLICIES)
def test_model_equals_host_twin_and_keeps_the_promise(policy, subsample):
    X, y = M.table()
    kw = dict(n_estimators=4, subsample=subsample, monotone_constraints=M.MONO, **policy)
    a = XGBRegressor(device="gpu", **kw).fit(X, y)
    _same_models(a, XGBRegressor(device="cpu", fixed_point=True, **kw).fit(X, y), 4)
    dev = torch.device("cuda", 0)
    M.assert_promise(lambda S: a.predict(S).cpu().numpy(), X, lambda S: torch.from_numpy(S).to(dev))


@pytest.mark.parametrize("policy", POLICIES[1:])
def test_multiclass_and_ranker_first_trees_equal_the_host_twin(policy):
    X, y = M.table()
    kw = dict(n_estimators=2, monotone_constraints=M.MONO, **policy)
    lab = np.digitize(y, np.quantile(y, [1 / 3, 2 / 3]))
    a = XGBClassifier(device="gpu", base_score=0.5, **kw).fit(X, lab)
    _same_models(a, XGBClassifier(device="cpu", fixed_point=True, base_score=0.5, **kw).fit(X, lab), 3)
    qid = np.repeat(np.arange(15), 20)
    a = XGBRanker(device="gpu", **kw).fit(X, lab, qid=qid)
    _same_models(a, XGBRanker(device="cpu", fixed_point=True, **kw).fit(X, lab, qid=qid), 1)
