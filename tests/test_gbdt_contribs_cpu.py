"""Node statistics, importances and feature contributions of mifx.gbdt on the host: gain and cover from both host
growers on exactly summable gradients; predict_contribs against a brute-force Shapley enumeration carried by this
file (2^f subsets, the recursive v(S)); additivity on a depth-12 forest; thread-count independence; every
importance type against a hand computation; every ValueError; pickling; the stand-alone sanitizer harness."""
import itertools
import math
import os
import pickle
import shutil
import subprocess

import numpy as np
import pytest

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, XGBRegressor, xgb
from test_gbdt_sample_cpu import grow_ex

ROOT = os.path.join(os.path.dirname(__file__), "..")


def grow_stats(bins, nbins, g, h, depth, mcw=1.0, gamma=0.0, fixed=True, threads=1, rows=None, mask=None, lam=1.0):
    """grow_ex's seven outputs from mifx_gbdt_grow[_fixed]_stats, then the nodes' gain and cover."""
    lib, p = xgb._lib(), xgb._p
    f, n = bins.shape
    cap = 2 ** (depth + 1)
    fe, sb, le, ri = (np.empty(cap, np.int32) for _ in range(4))
    dl, val, leaf = np.empty(cap, np.uint8), np.empty(cap, np.float64), np.full(n, -7, np.int32)
    gain, cover = np.full(cap, np.nan), np.full(cap, np.nan)
    fn = lib.mifx_gbdt_grow_fixed_stats if fixed else lib.mifx_gbdt_grow_stats
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    cnt = fn(p(bins, xgb._U16), n, f, p(nbins, xgb._I), p(g, xgb._F), p(h, xgb._F), depth, float(mcw), float(lam),
             float(gamma), 0.3, threads, cap, p(fe, xgb._I), p(sb, xgb._I), p(dl, xgb._U8), p(le, xgb._I),
             p(ri, xgb._I), p(val, xgb._D), p(leaf, xgb._I), None if rows is None else p(rows, xgb._I),
             0 if rows is None else len(rows), None if mask is None else p(mask, xgb._U8), p(gain, xgb._D),
             p(cover, xgb._D))
    assert cnt > 0, cnt
    return (fe[:cnt].copy(), sb[:cnt].copy(), dl[:cnt].copy(), le[:cnt].copy(), ri[:cnt].copy(), val[:cnt].copy(), leaf,
            gain[:cnt].copy(), cover[:cnt].copy())


# ---- statistics

@pytest.mark.parametrize("n,f", C.SHAPES)
def test_host_growers_record_gain_and_cover(n, f):
    """On dyadic gradients every sum is exact: the root's cover is sum(h), a parent's cover is its children's, the
    gain is above the leaf threshold at inner nodes and 0 at leaves, both learners agree bit for bit, and the trees
    are the ones the entries without statistics grow."""
    bins, nbins = C.make_bins(n, f, seed=n + f)
    g, h = C.dyadic_grads(n, n + f)
    splits = 0
    for depth, gamma in [(0, 0.0), (1, 0.0), (3, 0.25), (6, 0.0)]:
        per = []
        for fixed in (False, True):
            t = grow_stats(bins, nbins, g, h, depth, 1.0, gamma, fixed=fixed, threads=1 + fixed)
            C.assert_same_tree(t[:7], grow_ex(bins, nbins, g, h, depth, 1.0, gamma, fixed=fixed), f"depth {depth}")
            fe, le, ri, gain, cover = t[0], t[3], t[4], t[7], t[8]
            assert cover[0] == h.astype(np.float64).sum()
            inner = fe >= 0
            assert np.array_equal(cover[le[inner]] + cover[ri[inner]], cover[inner])
            assert (gain[inner] > 1e-6).all() and (gain[~inner] == 0.0).all() and not np.signbit(gain[~inner]).any()
            splits += int(inner.sum())
            per.append(t)
        for a, b in zip(per[0][7:], per[1][7:]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), f"depth {depth}"
    assert splits > 0 or n < 3 or f == 1


def test_statistics_of_sampled_and_masked_trees():
    """A row list: the cover is over the listed rows; the tree is the *_ex entry's; an empty list gives cover 0."""
    n, f = 1000, 3
    bins, nbins = C.make_bins(n, f, seed=5)
    g, h = C.dyadic_grads(n, 5)
    rows = xgb.sample_rows(3, 1, 0.5, n)
    mask = xgb.level_mask(3, 1, f, 4, 0.7, 0.7)
    for fixed in (False, True):
        t = grow_stats(bins, nbins, g, h, 4, fixed=fixed, rows=rows, mask=mask)
        C.assert_same_tree(t[:7], grow_ex(bins, nbins, g, h, 4, fixed=fixed, rows=rows, mask=mask))
        assert t[8][0] == h[rows].astype(np.float64).sum() and (t[0] >= 0).any()
        e = grow_stats(bins, nbins, g, h, 4, fixed=fixed, rows=np.zeros(0, np.int32))
        assert len(e[0]) == 1 and e[7][0] == 0.0 and e[8][0] == 0.0


# ---- the oracle: brute-force Shapley values of the path-dependent game

def tree_value(tree, cover, X, S):
    """v(S) of one tree for every row of X: follow the row at nodes whose feature is in S (x < thr left, NaN by
    default_left), average both children by cover(child) / cover(node) at the others. The recursion is evaluated
    from the last node to the root (children have larger indices)."""
    fe, thr, dl, le, ri, val = tree
    v = [None] * len(fe)
    for k in range(len(fe) - 1, -1, -1):
        if fe[k] < 0:
            v[k] = np.full(len(X), val[k])
        elif fe[k] in S:
            x = X[:, fe[k]]
            left = np.where(np.isnan(x), bool(dl[k]), x < thr[k])
            v[k] = np.where(left, v[le[k]], v[ri[k]])
        else:
            v[k] = (cover[le[k]] / cover[k]) * v[le[k]] + (cover[ri[k]] / cover[k]) * v[ri[k]]
    return v[0]


def shapley(trees, covers, X, f, base):
    """[n, f + 1]: the Shapley value of every feature in the game v(S) = sum over trees of tree_value, and
    base + v(empty) in column f."""
    sets = [frozenset(s) for r in range(f + 1) for s in itertools.combinations(range(f), r)]
    v = {s: sum(tree_value(t, c, X, s) for t, c in zip(trees, covers)) + np.zeros(len(X)) for s in sets}
    out = np.zeros((len(X), f + 1))
    for j in range(f):
        for s in sets:
            if j not in s:
                wt = math.factorial(len(s)) * math.factorial(f - len(s) - 1) / math.factorial(f)
                out[:, j] += wt * (v[s | {j}] - v[s])
    out[:, f] = base + v[frozenset()]
    return out


def leaf_scale(trees):
    """S: the sum over the trees of the largest |leaf value|."""
    return sum(float(np.abs(t[5][t[0] < 0]).max()) for t in trees)


def table(n, f, seed):
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, f))
    y = np.sin(2 * X[:, 0]) + (X[:, f // 2] > 0.3) * X[:, -1] + 0.3 * r.normal(size=n)
    X[r.random(X.shape) < 0.1] = np.nan
    return X, y


def probe_rows(X, count=40):
    """Rows to explain: ordinary ones with ~10 % NaN, then all-NaN, all +inf and all -inf."""
    f = X.shape[1]
    return np.concatenate([X[:count], np.full((1, f), np.nan), np.full((1, f), np.inf), np.full((1, f), -np.inf)])


def max_depth_of(tree):
    depth = np.zeros(len(tree[0]), int)
    for k in np.flatnonzero(tree[0] >= 0):
        depth[tree[3][k]] = depth[tree[4][k]] = depth[k] + 1
    return int(depth.max())


def _models():
    out = {}
    X, y = table(300, 1, 1)
    out["f1"] = (XGBRegressor(n_estimators=4, max_depth=4).fit(X, y), X)
    X, y = table(1000, 3, 2)
    w = np.random.default_rng(2).uniform(0.5, 2, len(y)).astype(np.float32)
    out["f3_depth6_weighted_subsampled"] = (XGBRegressor(n_estimators=5, max_depth=6, subsample=0.5, random_state=3)
                                            .fit(X, y, sample_weight=w), X)
    X, y = table(1000, 6, 3)
    out["f6_depth8_binary"] = (XGBClassifier(n_estimators=4, max_depth=8, fixed_point=True).fit(X, y > 0.2), X)
    X, y = table(600, 3, 4)
    out["three_classes"] = (XGBClassifier(n_estimators=1, max_depth=4).fit(X, np.digitize(y, [-0.4, 0.6])), X)
    X, y = table(400, 3, 5)
    noise = np.random.default_rng(5).normal(size=100)
    out["early_stopped"] = (XGBRegressor(n_estimators=5, max_depth=5, learning_rate=1.0)
                            .fit(X[:300], y[:300], eval_set=[(X[300:], noise)], early_stopping_rounds=1), X)
    X, y = table(100, 3, 6)
    # base_score 0: the leaves carry the mean (with the estimated intercept they are ~1e-9, and S, which the bound is
    # stated in, would be ten orders below the intercept that the bias column holds)
    out["single_leaves"] = (XGBRegressor(n_estimators=3, max_depth=0, base_score=0.0).fit(X, y + 1.0), X)
    return out


@pytest.fixture(scope="module")
def models():
    return _models()


def test_models_are_the_cases_meant(models):
    assert max_depth_of(models["f3_depth6_weighted_subsampled"][0]._trees[0]) == 6  # 6 > f: a path repeats a feature
    assert max(max_depth_of(t) for t in models["f6_depth8_binary"][0]._trees) == 8
    es = models["early_stopped"][0]
    assert es.best_iteration is not None and es.best_iteration + 1 < es.n_trees_
    assert all(len(t[0]) == 1 for t in models["single_leaves"][0]._trees)
    assert models["three_classes"][0]._num_class() == 3
    assert all(m.n_trees_ <= 5 for m, _ in models.values())


@pytest.mark.parametrize("name", ["f1", "f3_depth6_weighted_subsampled", "f6_depth8_binary", "three_classes",
                                  "early_stopped", "single_leaves"])
def test_contribs_equal_brute_force_shapley(models, name):
    m, X = models[name]
    P = probe_rows(X)
    f, K, limit = X.shape[1], m._num_class(), m._tree_limit()
    got = m.predict_contribs(P)
    assert got.shape == ((len(P), f + 1) if K == 1 else (len(P), K, f + 1)) and got.dtype == np.float64
    got = got.reshape(len(P), K, f + 1)
    for k in range(K):
        trees = m._trees[k:limit:K]
        want = shapley(trees, [s[1] for s in m._node_stats[k:limit:K]], P, f, m._base_margin)
        S = leaf_scale(trees)
        err = np.abs(got[:, k] - want).max()
        print(f"{name} class {k}: max |phi - oracle| = {err:.3g} = {err / S:.3g} S (S = {S:.4g}, bound 1e-12 S)")
        assert err <= 1e-12 * S
    P32 = np.where(np.isnan(P), 0.5, P).astype(np.float32)  # a float32 table means its exact widening
    assert np.array_equal(m.predict_contribs(P32), m.predict_contribs(P32.astype(np.float64)))


def test_early_stopped_contribs_use_best_iteration(models):
    m, X = models["early_stopped"]
    P = probe_rows(X)
    c = m.predict_contribs(P)
    assert np.abs(c.sum(-1) - m.predict(P)).max() <= 1e-12 * leaf_scale(m._trees[:m._tree_limit()])
    full = pickle.loads(pickle.dumps(m))
    full.best_iteration = None
    assert not np.array_equal(full.predict_contribs(P), c)


# ---- additivity, unused features, determinism

@pytest.fixture(scope="module")
def deep():
    r = np.random.default_rng(11)
    X = r.normal(size=(1000, 11))
    X[:, 10] = 1.5  # a constant column: no cut, so no tree can use it
    y = np.sin(3 * X[:, 0]) * X[:, 1] + np.abs(X[:, 2] - X[:, 3]) + np.cos(X[:, 4] * X[:, 5]) + X[:, 6:10].sum(1)
    X[r.random(X.shape) < 0.1] = np.nan
    m = XGBRegressor(n_estimators=3, max_depth=12, min_child_weight=1.0).fit(X, y)
    assert max(max_depth_of(t) for t in m._trees) == 12
    return m, X


def test_additivity_and_unused_feature_on_a_depth_12_forest(deep):
    m, X = deep
    P = probe_rows(X, 200)
    c = m.predict_contribs(P)
    S = leaf_scale(m._trees)
    err = np.abs(c.sum(-1) - m._predict_trees(P, m._trees, m._base_margin)).max()
    print(f"depth 12: max |sum(phi) - margin| = {err:.3g} = {err / S:.3g} S")
    assert err <= 1e-12 * S
    assert (c[:, 10] == 0.0).all() and np.abs(c[:, :10]).max() > 0
    assert "f10" not in m.get_score()


def test_multiclass_rows_sum_to_their_margins():
    X, y = table(600, 4, 8)
    m = XGBClassifier(n_estimators=4, max_depth=4).fit(X, np.digitize(y, [-0.4, 0.6]))
    P = probe_rows(X)
    c = m.predict_contribs(P)
    assert c.shape == (len(P), 3, 5)
    margins = m._margins(P)
    for k in range(3):
        assert np.abs(c[:, k].sum(-1) - margins[k]).max() <= 1e-12 * leaf_scale(m._trees[k::3])


def test_contribs_do_not_depend_on_the_thread_count(deep):
    m, X = deep
    P = probe_rows(X, 297)
    m.n_jobs = 1
    a = m.predict_contribs(P)
    m.n_jobs = 4
    b = m.predict_contribs(P)
    m.n_jobs = None
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- importances

def test_importances_equal_a_hand_computation(models):
    for name in ("f6_depth8_binary", "three_classes", "f3_depth6_weighted_subsampled"):
        m, X = models[name]
        f = X.shape[1]
        cnt, tg, tc = [0] * f, [0.0] * f, [0.0] * f
        for (fe, *_), (gain, cover) in zip(m._trees, m._node_stats):
            for k in range(len(fe)):
                if fe[k] >= 0:
                    cnt[fe[k]] += 1
                    tg[fe[k]] += gain[k]
                    tc[fe[k]] += cover[k]
        want = {"weight": cnt, "total_gain": tg, "total_cover": tc,
                "gain": [a / max(c, 1) for a, c in zip(tg, cnt)], "cover": [a / max(c, 1) for a, c in zip(tc, cnt)]}
        for kind, w in want.items():
            got = m.get_score(kind)
            assert sorted(got) == sorted(f"f{j}" for j in range(f) if cnt[j])
            for j in range(f):
                if cnt[j]:  # sums of < 2^11 positive doubles in another order: 2^11 ulp at the most
                    assert got[f"f{j}"] == pytest.approx(w[j], rel=2.0 ** -42, abs=0)
            fi = type(m)(importance_type=kind)
            fi.__dict__.update({k: v for k, v in m.__dict__.items() if k != "importance_type"})
            imp = fi.feature_importances_
            assert imp.dtype == np.float32 and imp.shape == (f,)
            assert abs(float(imp.astype(np.float64).sum()) - 1.0) <= f * 2.0 ** -24
            assert np.allclose(imp, np.asarray(w, float) / sum(w), rtol=2.0 ** -22, atol=0)
        assert m.importance_type == "gain" and np.array_equal(
            m.feature_importances_, (np.asarray(m._importance("gain")) / sum(m._importance("gain"))).astype(np.float32))


def test_importances_of_a_forest_without_splits(models):
    m, X = models["single_leaves"]
    assert m.get_score() == {} and m.get_score("gain") == {}
    assert np.array_equal(m.feature_importances_, np.zeros(X.shape[1], np.float32))


# ---- errors, old models, pickling

def test_zero_cover_child_is_refused_by_contribs_only(models):
    m = pickle.loads(pickle.dumps(models["f3_depth6_weighted_subsampled"][0]))
    X = models["f3_depth6_weighted_subsampled"][1]
    want = m.predict(X)
    child = int(m._trees[1][3][0])
    m._node_stats[1][1][child] = 0.0
    with pytest.raises(ValueError, match="cover"):
        m.predict_contribs(X)
    assert np.array_equal(m.predict(X), want)
    m._node_stats[1][1][child] = np.inf
    m._paths = None
    with pytest.raises(ValueError, match="cover"):
        m.predict_contribs(X)


def test_model_without_statistics_keeps_predicting_and_asks_for_a_refit(models):
    src, X = models["f6_depth8_binary"]
    m = pickle.loads(pickle.dumps(src))
    del m.__dict__["_node_stats"]
    assert np.array_equal(m.predict_proba(X), src.predict_proba(X))
    for call in (lambda: m.predict_contribs(X), lambda: m.get_score(), lambda: m.feature_importances_):
        with pytest.raises(ValueError, match="refit"):
            call()
    m._node_stats = src._node_stats[:-1]  # hand-assigned trees that the statistics do not match
    with pytest.raises(ValueError, match="refit"):
        m.predict_contribs(X)


def test_bad_arguments_are_rejected(models):
    m, X = models["f6_depth8_binary"]
    with pytest.raises(ValueError, match="features"):
        m.predict_contribs(X[:, :5])
    with pytest.raises(ValueError, match="features"):
        m.predict_contribs(X[0])
    with pytest.raises(ValueError, match="importance_type"):
        m.get_score("splits")
    bad = XGBRegressor(importance_type="splits")
    bad.__dict__.update({k: v for k, v in m.__dict__.items() if k != "importance_type"})
    with pytest.raises(ValueError, match="importance_type"):
        bad.feature_importances_


def test_pickle_keeps_statistics_and_drops_caches(models):
    m, X = models["f3_depth6_weighted_subsampled"]
    c = m.predict_contribs(X[:50])
    m._dev_paths = {0: "a device copy"}
    state = m.__getstate__()
    assert "_node_stats" in state and not {"_paths", "_dev_paths", "_dev_forest"} & set(state)
    r = pickle.loads(pickle.dumps(m))
    m._dev_paths = None
    for (ga, ca), (gb, cb) in zip(m._node_stats, r._node_stats):
        assert np.array_equal(ga, gb) and np.array_equal(ca, cb)
    assert np.array_equal(r.predict_contribs(X[:50]), c) and r.get_score("gain") == m.get_score("gain")
    m.fit(X[:200], np.arange(200.0))
    assert m._dev_paths is None and len(m._node_stats) == m.n_trees_


# ---- the sanitizer harness

@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_gbdt_contribs_sanitizers(tmp_path):
    """tools/sanitize/gbdt_contribs_fuzz.cpp: a stand-alone program over mifx_gbdt_paths_build and mifx_gbdt_contribs
    with random and malformed forests, under ASan + UBSan (the sanitizer runtimes linked statically into it)."""
    exe = str(tmp_path / "gbdt_contribs_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-omit-frame-pointer", "-std=c++17", "-pthread",
                    os.path.join(ROOT, "tools", "sanitize", "gbdt_contribs_fuzz.cpp"),
                    os.path.join(ROOT, "csrc", "gbdt.cpp"), "-o", exe], check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
