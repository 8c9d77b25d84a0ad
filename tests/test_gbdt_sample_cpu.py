"""Stochastic boosting and instance weights of mifx.gbdt on the host: the draws of csrc/gbdt_sample.h against their
numpy twin (mifx/gbdt/sample.py), the *_ex growers against the UNCHANGED growers on gathered sub-tables and on
nbins = 1 columns, the estimators' new parameters, every ValueError, and the stand-alone sanitizer harness."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, XGBRegressor, xgb
from mifx.gbdt import sample as S

ROOT = os.path.join(os.path.dirname(__file__), "..")
RATES = [0.1, 0.5, 0.8, 1.0]
SEEDS = [0, 1, 2 ** 63 + 5]
ROUNDS = [0, 1, 59]


def c_row_mask(seed, rnd, rate, n):
    keep = np.empty(n, np.uint8)
    cnt = xgb._lib().mifx_gbdt_sample_rows(seed, rnd, float(rate), n, xgb._p(keep, xgb._U8))
    assert cnt == int(keep.sum()) and set(np.unique(keep)) <= {0, 1}
    return keep.astype(bool)


def c_choose(seed, rnd, site, rate, f, cand=None):
    out = np.empty(f, np.uint8)
    cm = None if cand is None else np.isin(np.arange(f), cand).astype(np.uint8)
    k = xgb._lib().mifx_gbdt_sample_features(seed, rnd, site, float(rate), None if cm is None else xgb._p(cm, xgb._U8),
                                             f, xgb._p(out, xgb._U8))
    assert k == int(out.sum())
    return np.flatnonzero(out)


def grow_ex(bins, nbins, g, h, depth, mcw=1.0, gamma=0.0, fixed=True, threads=1, rows=None, mask=None, lam=1.0):
    """(feature, split_bin, default_left, left, right, value, leaf_of_row) from mifx_gbdt_grow[_fixed]_ex."""
    lib, p = xgb._lib(), xgb._p
    f, n = bins.shape
    cap = 2 ** (depth + 1)
    fe, sb, le, ri = (np.empty(cap, np.int32) for _ in range(4))
    dl, val, leaf = np.empty(cap, np.uint8), np.empty(cap, np.float64), np.full(n, -7, np.int32)
    fn = lib.mifx_gbdt_grow_fixed_ex if fixed else lib.mifx_gbdt_grow_ex
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    cnt = fn(p(bins, xgb._U16), n, f, p(nbins, xgb._I), p(g, xgb._F), p(h, xgb._F), depth, float(mcw), float(lam),
             float(gamma), 0.3, threads, cap, p(fe, xgb._I), p(sb, xgb._I), p(dl, xgb._U8), p(le, xgb._I),
             p(ri, xgb._I), p(val, xgb._D), p(leaf, xgb._I), None if rows is None else p(rows, xgb._I),
             0 if rows is None else len(rows), None if mask is None else p(mask, xgb._U8))
    assert cnt > 0, cnt
    return fe[:cnt].copy(), sb[:cnt].copy(), dl[:cnt].copy(), le[:cnt].copy(), ri[:cnt].copy(), val[:cnt].copy(), leaf


# ---- the generator

@pytest.mark.parametrize("n", [1, 2, 63, 65, 5000])
def test_row_mask_c_equals_numpy_twin(n):
    for rate in RATES:
        masks = {}
        for seed in SEEDS:
            for rnd in ROUNDS:
                got = c_row_mask(seed, rnd, rate, n)
                assert np.array_equal(got, S.row_mask(seed, rnd, rate, n)), (n, rate, seed, rnd)
                assert np.array_equal(np.flatnonzero(got), xgb.sample_rows(seed, rnd, rate, n))
                masks[seed, rnd] = got
                if rate == 1.0:
                    assert got.all()
                if n == 5000 and rate < 1.0:  # the rule's own worst case over seeds 0-7, rounds 0-59: 3.5 sigma
                    assert abs(int(got.sum()) - n * rate) <= 5 * math.sqrt(n * rate * (1 - rate)), (rate, seed, rnd)
        if n == 5000 and rate < 1.0:
            for a in SEEDS:
                assert not np.array_equal(masks[a, 0], masks[a, 1]) and not np.array_equal(masks[a, 1], masks[a, 59])
            for r in ROUNDS:
                assert not np.array_equal(masks[0, r], masks[1, r])
                assert not np.array_equal(masks[1, r], masks[SEEDS[2], r])


def test_empty_and_single_row_samples_grow_the_specified_trees():
    """Seed 0, one row, rate 0.1: the sample is empty in some of rounds 0-5 and holds the row in others. Empty: one
    node of value +0.0 and leaf_of_row -1 (no division: lambda = 0 too); non-empty: the tree of the unsampled row."""
    bins, nbins = np.array([[0], [1]], np.uint16), np.array([2, 3], np.int32)
    g, h = np.array([0.5], np.float32), np.array([1.0], np.float32)
    sizes = []
    for rnd in range(6):
        rows = xgb.sample_rows(0, rnd, 0.1, 1)
        sizes.append(len(rows))
        for fixed in (True, False):
            for lam in (1.0, 0.0):
                t = grow_ex(bins, nbins, g, h, 3, 0.0, fixed=fixed, rows=rows, lam=lam)
                if len(rows) == 0:
                    assert len(t[0]) == 1 and t[0][0] == -1 and t[3][0] == -1 and t[4][0] == -1
                    assert t[5][0] == 0.0 and not np.signbit(t[5][0]) and t[6][0] == -1
                else:
                    C.assert_same_tree(t, C.host_grow(bins, nbins, g, h, 3, 0.0, 0.0, fixed=fixed, lam=lam))
                    assert t[6][0] == 0 and t[5][0] == -0.3 * 0.5 / (1.0 + lam)
    assert 0 in sizes and 1 in sizes


def test_feature_choice_c_equals_numpy_twin():
    for f in (1, 3, 11, 36):
        for rate in (0.01, 0.3, 0.5, 0.99, 1.0):
            for seed in SEEDS:
                for rnd in (0, 7):
                    tree = c_choose(seed, rnd, S.SITE_TREE, rate, f)
                    assert np.array_equal(tree, S.choose_features(seed, rnd, S.SITE_TREE, rate, np.arange(f)))
                    assert len(tree) == max(1, int(rate * f))
                    lv = c_choose(seed, rnd, S.SITE_LEVEL0 + 2, rate, f, tree)
                    assert np.array_equal(lv, S.choose_features(seed, rnd, S.SITE_LEVEL0 + 2, rate, tree))
                    assert len(lv) == max(1, int(rate * len(tree))) and set(lv) <= set(tree)
                    for bt, bl in ((rate, 1.0), (1.0, rate), (rate, rate)):
                        m = xgb.level_mask(seed, rnd, f, 4, bt, bl)
                        assert np.array_equal(m, S.level_mask(seed, rnd, f, 4, bt, bl))
                        assert m.shape == (4, f) and m.sum(1).min() >= 1
                        if bl == 1.0:
                            assert (m == m[0]).all() and m[0].sum() == max(1, int(bt * f))
                        else:
                            ts = np.flatnonzero(S.level_mask(seed, rnd, f, 1, bt, 1.0)[0])
                            assert all(set(np.flatnonzero(r)) <= set(ts) for r in m)
                            assert (m.sum(1) == max(1, int(bl * len(ts)))).all()


def test_feature_choice_covers_every_feature():
    for seed in (0, 1, 7):
        counts = np.zeros(11, int)
        for rnd in range(100):
            counts[c_choose(seed, rnd, S.SITE_TREE, 0.5, 11)] += 1
        assert counts.min() >= 25 and counts.max() <= 75 and counts.sum() == 500, counts  # the rule gives 35-54


# ---- the *_ex growers against unchanged code

def _rows_for(n, k):
    rows = np.flatnonzero(S.row_mask(n + k, k, 0.5, n)).astype(np.int32)
    return rows if len(rows) else np.array([n - 1], np.int32)


@pytest.mark.parametrize("n,f", C.SHAPES)
def test_row_list_equals_unchanged_grower_on_the_gathered_subtable(n, f):
    bins, nbins = C.make_bins(n, f, seed=n * 31 + f)
    for k, depth in enumerate((0, 3, 6)):
        rows = _rows_for(n, k)
        sub = np.ascontiguousarray(bins[:, rows])
        for fixed, (g, h) in ((True, C.float_grads(n, n + f)), (True, C.dyadic_grads(n, n + f)),
                              (False, C.dyadic_grads(n, n + f))):
            want = C.host_grow(sub, nbins, g[rows].copy(), h[rows].copy(), depth, 1.0, 0.0, fixed=fixed)
            got = grow_ex(bins, nbins, g, h, depth, fixed=fixed, rows=rows)
            C.assert_same_tree(got[:6], want[:6], f"depth {depth} fixed {fixed}")
            assert np.array_equal(got[6][rows], want[6]), f"depth {depth} fixed {fixed}: leaf_of_row"
            off = np.ones(n, bool)
            off[rows] = False
            assert (got[6][off] == -1).all()
            # every row listed: the unsampled tree, and so are the null arguments
            C.assert_same_tree(grow_ex(bins, nbins, g, h, depth, fixed=fixed, rows=np.arange(n)),
                               C.host_grow(bins, nbins, g, h, depth, 1.0, 0.0, fixed=fixed))
            C.assert_same_tree(grow_ex(bins, nbins, g, h, depth, fixed=fixed),
                               C.host_grow(bins, nbins, g, h, depth, 1.0, 0.0, fixed=fixed))


@pytest.mark.parametrize("n,f", C.SHAPES)
def test_tree_mask_equals_unchanged_grower_with_one_bin_columns(n, f):
    bins, nbins = C.make_bins(n, f, seed=n * 31 + f)
    for depth in (0, 3, 6):
        tree_set = S.level_mask(n, depth, f, 1, 0.5, 1.0)[0]
        mask = np.tile(tree_set, (depth, 1))
        nb1 = np.where(tree_set == 1, nbins, 1).astype(np.int32)
        one = bins.copy()  # the reference's table: a masked column holds its one bin (the double learner does not
        one[(tree_set == 0) & (nbins > 1)] = 0  # clamp a bin index, so the column must fit its nbins = 1)
        for fixed, (g, h) in ((True, C.float_grads(n, n + f)), (True, C.dyadic_grads(n, n + f)),
                              (False, C.dyadic_grads(n, n + f))):
            want = C.host_grow(one, nb1, g, h, depth, 1.0, 0.0, fixed=fixed)
            if fixed:  # the twin clamps: the table itself with nbins = 1 is the same tree
                C.assert_same_tree(C.host_grow(bins, nb1, g, h, depth, 1.0, 0.0, fixed=True), want)
            got = grow_ex(bins, nbins, g, h, depth, fixed=fixed, mask=mask)
            C.assert_same_tree(got, want, f"depth {depth} fixed {fixed}")
            assert set(got[0][got[0] >= 0]) <= set(np.flatnonzero(tree_set))


def _depths(t):
    depth = np.zeros(len(t[0]), int)
    for k in range(len(t[0])):
        if t[0][k] >= 0:
            depth[t[3][k]] = depth[t[4][k]] = depth[k] + 1
    return depth


@pytest.mark.parametrize("n,f", [(5000, 11), (1000, 3), (30000, 11)])
def test_level_mask_confines_each_depth_and_threads_agree(n, f):
    bins, nbins = C.make_bins(n, f, seed=n + f)
    g, h = C.float_grads(n, n)
    mask = S.level_mask(3, 1, f, 6, 1.0, 0.5)
    rows = np.flatnonzero(S.row_mask(3, 1, 0.5, n)).astype(np.int32)
    assert len({tuple(r) for r in mask}) > 1
    for fixed in (True, False):
        t = grow_ex(bins, nbins, g, h, 6, 0.0, fixed=fixed, rows=rows, mask=mask)
        split = t[0] >= 0
        assert split.sum() > (5 if f > 3 else 0)  # f = 3: one feature per level, and one of the three is constant
        assert all(mask[d, j] for d, j in zip(_depths(t)[split], t[0][split]))
        C.assert_same_tree(grow_ex(bins, nbins, g, h, 6, 0.0, fixed=fixed, rows=rows, mask=mask, threads=4), t)


def test_bad_row_lists_are_refused():
    bins, nbins = C.make_bins(10, 2, seed=1)
    g, h = C.float_grads(10, 1)
    for rows in ([3, 3], [5, 2], [-1], [10]):
        for fixed in (True, False):
            with pytest.raises(AssertionError):
                grow_ex(bins, nbins, g, h, 2, fixed=fixed, rows=rows)


# ---- the estimators

def _data(n=800, f=6, seed=11):
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, f))
    y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.1, n)
    X[r.random(X.shape) < 0.05] = np.nan
    return X[: n * 3 // 4], y[: n * 3 // 4], X[n * 3 // 4:], y[n * 3 // 4:]


def _same_model(a, b):
    assert a.n_trees_ == b.n_trees_ and a._base_margin == b._base_margin
    for t, (ta, tb) in enumerate(zip(a._trees, b._trees)):
        for u, v in zip(ta, tb):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"tree {t}"
    assert a.evals_result_ == b.evals_result_


@pytest.mark.parametrize("fixed", [False, True])
def test_defaults_and_unit_weights_give_the_default_model(fixed):
    X, y, Xe, ye = _data()
    kw = dict(n_estimators=12, fixed_point=fixed)
    ref = XGBRegressor(**kw).fit(X, y, eval_set=[(Xe, ye)])
    for m in (XGBRegressor(subsample=1.0, colsample_bytree=1.0, colsample_bylevel=1.0, random_state=5, **kw)
              .fit(X, y, eval_set=[(Xe, ye)]),
              XGBRegressor(**kw).fit(X, y, eval_set=[(Xe, ye)], sample_weight=np.ones(len(y)))):
        _same_model(m, ref)
        assert np.array_equal(m.predict(Xe), ref.predict(Xe))
    lab = (y > np.median(y)).astype(int)
    cref = XGBClassifier(**kw).fit(X, lab, eval_set=[(Xe, (ye > np.median(y)).astype(int))])
    c = XGBClassifier(scale_pos_weight=1.0, **kw).fit(X, lab, eval_set=[(Xe, (ye > np.median(y)).astype(int))],
                                                      sample_weight=np.ones(len(y), np.float32))
    _same_model(c, cref)
    assert np.array_equal(c.predict_proba(Xe), cref.predict_proba(Xe))


@pytest.mark.parametrize("fixed", [False, True])
def test_random_state_decides_the_model(fixed):
    X, y, Xe, ye = _data()
    kw = dict(n_estimators=8, fixed_point=fixed, subsample=0.5, colsample_bytree=0.5, colsample_bylevel=0.5)
    a = XGBRegressor(random_state=3, **kw).fit(X, y, eval_set=[(Xe, ye)])
    _same_model(XGBRegressor(random_state=3, **kw).fit(X, y, eval_set=[(Xe, ye)]), a)
    b = XGBRegressor(random_state=4, **kw).fit(X, y, eval_set=[(Xe, ye)])
    assert any(len(ta[0]) != len(tb[0]) or not np.array_equal(ta[0], tb[0]) for ta, tb in zip(a._trees, b._trees))
    full = XGBRegressor(n_estimators=8, fixed_point=fixed).fit(X, y)
    assert any(len(ta[0]) != len(tb[0]) or not np.array_equal(ta[0], tb[0]) for ta, tb in zip(a._trees, full._trees))
    # it still learns: better on held-out rows than the constant predictor, whose error is their spread
    assert float(np.sqrt(np.mean((a.predict(Xe) - ye) ** 2))) < ye.std()


def test_n_jobs_does_not_change_a_sampled_fixed_point_model():
    r = np.random.default_rng(5)
    X = r.normal(size=(30000, 12))  # n_s * f > 200k: the threaded paths run
    y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.1, 30000)
    w = r.uniform(0, 2, 30000)
    kw = dict(n_estimators=4, max_bins=64, fixed_point=True, subsample=0.5, colsample_bytree=0.5,
              colsample_bylevel=0.5, random_state=9)
    a = XGBRegressor(n_jobs=1, **kw).fit(X, y, sample_weight=w)
    b = XGBRegressor(n_jobs=4, **kw).fit(X, y, sample_weight=w)
    _same_model(a, b)
    assert np.array_equal(a.predict(X[:500]), b.predict(X[:500]))


@pytest.mark.parametrize("fixed", [False, True])
def test_first_weighted_tree_equals_a_hand_made_grow(fixed):
    X, y, _, _ = _data()
    w = np.random.default_rng(2).uniform(0, 4, len(y)).astype(np.float32)
    w[:7] = 0.0
    m = XGBRegressor(n_estimators=1, fixed_point=fixed, max_depth=4).fit(X, y, sample_weight=w)
    base = float(np.average(y, weights=w.astype(np.float64)))
    assert m._base_margin == base and base != float(np.mean(y))
    g = (np.full(len(y), base) - y).astype(np.float32) * w
    ref = XGBRegressor(n_estimators=1, fixed_point=fixed, max_depth=4)
    bins = ref._bin_matrix(np.ascontiguousarray(X))
    tree = ref._grow(bins, (ref._ncut + 1).astype(np.int32), g, w.copy(), np.empty(len(y), np.int32))
    for u, v in zip(m._trees[0], tree):
        assert np.array_equal(u, v)
    # a tensor and a list are weights too
    import torch

    m2 = XGBRegressor(n_estimators=1, fixed_point=fixed, max_depth=4).fit(X, y, sample_weight=torch.from_numpy(w))
    _same_model(m2, m)


def test_weighted_intercepts_and_scale_pos_weight():
    X, y, _, _ = _data()
    lab = np.where(y > np.quantile(y, 0.7), "pos", "neg")
    y01 = (lab == "pos").astype(np.float64)
    w = np.random.default_rng(3).uniform(0.5, 2, len(y)).astype(np.float32)
    c = XGBClassifier(n_estimators=3).fit(X, lab, sample_weight=w)
    p = float(np.average(y01, weights=w.astype(np.float64)))
    assert c._base_margin == float(np.log(p / (1 - p)))
    for fixed in (False, True):
        a = XGBClassifier(n_estimators=5, fixed_point=fixed, scale_pos_weight=3).fit(X, lab, sample_weight=w)
        b = XGBClassifier(n_estimators=5, fixed_point=fixed).fit(X, lab, sample_weight=np.where(y01 == 1, w * 3, w))
        _same_model(a, b)
        a = XGBClassifier(n_estimators=5, fixed_point=fixed, scale_pos_weight=3).fit(X, lab)
        b = XGBClassifier(n_estimators=5, fixed_point=fixed).fit(X, lab, sample_weight=np.where(y01 == 1, 3.0, 1.0))
        _same_model(a, b)
        p3 = 3 * y01.sum() / (3 * y01.sum() + (1 - y01).sum())
        assert abs(a._base_margin - np.log(p3 / (1 - p3))) < 1e-12
        plain = XGBClassifier(n_estimators=5, fixed_point=fixed).fit(X, lab)
        assert (a.predict(X) == "pos").sum() > (plain.predict(X) == "pos").sum()


def test_value_errors_without_a_gpu():
    X, y = np.random.default_rng(0).normal(size=(20, 2)), np.arange(20.0)
    for dev in (None, "gpu"):  # device="gpu": refused before the device is looked for
        for name in ("subsample", "colsample_bytree", "colsample_bylevel"):
            for bad in (0.0, -0.5, 1.5, float("nan")):
                with pytest.raises(ValueError, match=name):
                    XGBRegressor(device=dev, **{name: bad})
                m = XGBRegressor(device=dev)
                setattr(m, name, bad)
                with pytest.raises(ValueError, match=name):
                    m.fit(X, y)
        for bad, what in ((np.ones(19), "one weight per row"), (np.ones((20, 2)), "one weight per row"),
                          (-np.ones(20), "non-negative"), (np.r_[np.ones(19), np.nan], "finite"),
                          (np.r_[np.ones(19), np.inf], "finite"), (np.zeros(20), "all zero")):
            for cls in (XGBRegressor, XGBClassifier):
                with pytest.raises(ValueError, match=what):
                    cls(device=dev).fit(X, (y > 9).astype(int) if cls is XGBClassifier else y, sample_weight=bad)
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="scale_pos_weight"):
                XGBClassifier(device=dev, scale_pos_weight=bad)
            m = XGBClassifier(device=dev)
            m.scale_pos_weight = bad
            with pytest.raises(ValueError, match="scale_pos_weight"):
                m.fit(X, (y > 9).astype(int))


# ---- the sanitizer harness

@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_gbdt_sample_sanitizers(tmp_path, san):
    """tools/sanitize/gbdt_sample_fuzz.cpp: a stand-alone program over mifx_gbdt_grow_ex / mifx_gbdt_grow_fixed_ex with
    random row lists (empty and single-row ones too) and random level masks, under ASan + UBSan and under TSan."""
    exe = str(tmp_path / "gbdt_sample_fuzz")
    subprocess.run(["g++", "-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer", "-std=c++17", "-pthread",
                    os.path.join(ROOT, "tools", "sanitize", "gbdt_sample_fuzz.cpp"),
                    os.path.join(ROOT, "csrc", "gbdt.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1",
               TSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    if "ThreadSanitizer: unexpected memory mapping" in r.stderr and shutil.which("setarch"):
        # a kernel with more address-space randomisation than this TSan runtime knows: run it without ASLR
        r = subprocess.run(["setarch", os.uname().machine, "-R", exe], capture_output=True, text=True, timeout=600,
                           env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "WARNING: ThreadSanitizer" not in r.stderr
