"""Device feature preparation and prediction of mifx.gbdt (csrc/gbdt_prep.hip, mifx/ops/gbdt_prep.py) against the host
functions of csrc/gbdt.cpp: cuts equal mifx_gbdt_cuts, bins equal mifx_gbdt_bin, predictions equal mifx_gbdt_predict
bit for bit -- exact equality everywhere, for any launch geometry -- and XGB*(device="gpu") end to end on data that is
on the device already."""
import math

import numpy as np
import pytest
import torch

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, XGBRegressor, xgb

pytestmark = pytest.mark.gpu

MAX_BINS = [2, 3, 16, 256]
DEV = torch.device("cuda", 0)


def _P():
    from mifx.ops import gbdt_prep

    return gbdt_prep


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- host references (csrc/gbdt.cpp through xgb._lib(), as gbdt_cases does)

def host_cuts(col, max_bins):
    col = np.ascontiguousarray(col, np.float64)
    buf = np.empty(max(1, max_bins), np.float64)
    m = xgb._lib().mifx_gbdt_cuts(xgb._p(col, xgb._D), len(col), 1, max_bins, xgb._p(buf, xgb._D))
    assert m >= 0
    return buf[:m].copy()


def host_tables(X, max_bins):
    cuts = [host_cuts(X[:, j], max_bins) for j in range(X.shape[1])]
    ncut = np.array([len(c) for c in cuts], np.int32)
    off = (np.cumsum(ncut) - ncut).astype(np.int32)
    flat = np.concatenate(cuts) if ncut.sum() else np.zeros(1)
    return cuts, np.ascontiguousarray(flat, np.float64), off, ncut


def host_bins(X, flat, off, ncut):
    """Row-major [n, f] uint16: mifx_gbdt_bin's column-major output, transposed."""
    X = np.ascontiguousarray(X, np.float64)
    n, f = X.shape
    out = np.empty((f, n), np.uint16)
    xgb._lib().mifx_gbdt_bin(xgb._p(X, xgb._D), n, f, xgb._p(flat, xgb._D), xgb._p(off, xgb._I), xgb._p(ncut, xgb._I),
                             xgb._p(out, xgb._U16), 1)
    return np.ascontiguousarray(out.T)


def device_bins_np(P, X, flat, off, ncut, **geometry):
    got = P.device_bins(up(X), P.CutTables(flat, off, ncut, DEV), **geometry)
    assert got.dtype == torch.int16 and got.is_contiguous() and tuple(got.shape) == X.shape
    return got.cpu().numpy().view(np.uint16)


# ---- columns

KINDS = ["normal", "ints == max_bins", "ints == max_bins + 1", "70% zeros", "rounded", "constant", "all NaN",
         "10% NaN", "90% NaN", "+-inf", "+-0.0", "ties and NaN"]


def _ints(r, n, distinct):
    col = r.integers(0, distinct, n).astype(np.float64)
    k = min(n, distinct)
    col[r.permutation(n)[:k]] = np.arange(k)  # every value present: exactly min(n, distinct) distinct values
    return col


def mixed_matrix(n, max_bins, seed):
    """[n, len(KINDS)] float64: one column per kind, so the cut counts differ per feature."""
    r = np.random.default_rng(seed)
    z = r.standard_normal
    nan10, nan90, ties = z(n), z(n), np.round(z(n), 1)
    nan10[r.random(n) < 0.1] = np.nan
    nan90[r.random(n) < 0.9] = np.nan
    ties[r.random(n) < 0.2] = np.nan
    infs = z(n)
    infs[r.random(n) < 0.1] = np.inf
    infs[r.random(n) < 0.1] = -np.inf
    pm = np.where(r.random(n) < 0.5, -0.0, 0.0)  # both zeros, among a few small integers
    other = r.random(n) < 0.3
    pm[other] = r.integers(-2, 3, n)[other]
    cols = [z(n), _ints(r, n, max_bins), _ints(r, n, max_bins + 1), np.where(r.random(n) < 0.7, 0.0, z(n)),
            np.round(z(n), 1), np.full(n, 1.5), np.full(n, np.nan), nan10, nan90, infs, pm, ties]
    assert len(cols) == len(KINDS)
    return np.ascontiguousarray(np.stack(cols, 1))


# ---- cuts

@pytest.mark.parametrize("max_bins", MAX_BINS)
@pytest.mark.parametrize("n", C.NS)
def test_cuts_equal_host(n, max_bins):
    P = _P()
    X = mixed_matrix(n, max_bins, seed=n * 7 + max_bins)
    for name, Xh in (("float64", X), ("float32", X.astype(np.float32))):
        want, wflat, woff, wncut = host_tables(Xh.astype(np.float64), max_bins)  # float32: its exact widening
        got, flat, off, ncut = P.device_cuts(up(Xh), max_bins)
        for j, kind in enumerate(KINDS):
            assert got[j].dtype == np.float64 and np.array_equal(got[j], want[j]), \
                f"{name} n {n} max_bins {max_bins} column '{kind}': {len(got[j])} cuts, host {len(want[j])}"
        assert np.array_equal(ncut, wncut) and np.array_equal(off, woff) and np.array_equal(flat, wflat)
        assert ncut.dtype == off.dtype == np.int32 and flat.dtype == np.float64
    if n >= 63 and max_bins >= 16:
        assert len(set(wncut)) > 2  # the features' cut counts differ
    assert wncut[KINDS.index("constant")] == 0 and wncut[KINDS.index("all NaN")] == 0


def test_cuts_regime_boundary_and_single_columns():
    """Exactly max_bins distinct values keep one bin per value; one more switches to count quantiles."""
    P = _P()
    r = np.random.default_rng(5)
    for max_bins in MAX_BINS:
        for distinct in (max_bins - 1, max_bins, max_bins + 1, 2 * max_bins + 1):
            col = _ints(r, 5000, max(1, distinct))[:, None]
            got = P.device_cuts(up(col), max_bins)[0][0]
            want = host_cuts(col[:, 0], max_bins)
            assert np.array_equal(got, want), f"max_bins {max_bins}, {distinct} distinct values"
            if distinct <= max_bins:
                assert len(got) == max(1, distinct) - 1
    with pytest.raises(ValueError, match="max_bins"):
        P.device_cuts(up(np.zeros((4, 1))), 1)
    with pytest.raises(ValueError, match="max_bins"):
        P.device_cuts(up(np.zeros((4, 1))), 257)


def test_cuts_geometry_independent():
    P = _P()
    X = mixed_matrix(5000, 16, seed=11)
    Xd = up(X)
    for max_bins in (16, 256):
        ref = P.device_cuts(Xd, max_bins)
        for blocks in (1, 7, 300, 4096):
            got = P.device_cuts(Xd, max_bins, _blocks=blocks)
            assert all(np.array_equal(a, b) for a, b in zip(got[0], ref[0])), f"blocks {blocks}"
            assert all(np.array_equal(a, b) for a, b in zip(got[1:], ref[1:])), f"blocks {blocks}"


# ---- bins

@pytest.mark.parametrize("max_bins", MAX_BINS)
@pytest.mark.parametrize("n", C.NS)
def test_bins_equal_host(n, max_bins):
    P = _P()
    X = mixed_matrix(n, max_bins, seed=n * 7 + max_bins)
    _, flat, off, ncut = host_tables(X, max_bins)
    want = host_bins(X, flat, off, ncut)
    assert np.array_equal(device_bins_np(P, X, flat, off, ncut), want)
    assert (want[np.isnan(X)] == 0xFFFF).all() and (want[:, KINDS.index("constant")] == 0).all()
    X32 = X.astype(np.float32)
    assert np.array_equal(device_bins_np(P, X32, flat, off, ncut), host_bins(X32.astype(np.float64), flat, off, ncut))


def probe_matrix(cuts, n, seed):
    """[n, f] values around the cuts: equal to a cut, just below and just above one, below the first and above the
    last, +-inf and NaN."""
    r = np.random.default_rng(seed)
    X = np.empty((n, len(cuts)))
    for j, c in enumerate(cuts):
        if not len(c):
            X[:, j] = r.standard_normal(n)
        else:
            pick = c[r.integers(0, len(c), n)]
            how = r.integers(0, 7, n)
            X[:, j] = np.select([how == 0, how == 1, how == 2, how == 3, how == 4, how == 5],
                                [pick, np.nextafter(pick, -np.inf), np.nextafter(pick, np.inf), c[0] - 1.0,
                                 c[-1] + 1.0, np.where(pick > 0, np.inf, -np.inf)], np.nan)
    return X


@pytest.mark.parametrize("f", [1, 3, 11, 40])  # 40 > one LDS feature tile of 32 features at 255 cuts each
def test_bins_at_the_cuts(f):
    P = _P()
    r = np.random.default_rng(f)
    T = r.standard_normal((1000, f))
    if f >= 3:
        T[:, 1] = 2.0  # a feature without a cut
        T[:, f - 1] = np.round(T[:, f - 1])  # a few cuts
    cuts, flat, off, ncut = host_tables(T, 256)
    assert ncut.max() == 255 and (f < 3 or ncut[1] == 0)
    X = probe_matrix(cuts, 777, seed=f)
    want = host_bins(X, flat, off, ncut)
    assert np.array_equal(device_bins_np(P, X, flat, off, ncut), want)
    assert (want[np.isnan(X)] == 0xFFFF).all() and want[~np.isnan(X)].max() == 255 and want.min() == 0
    if f >= 3:
        assert (want[:, 1][~np.isnan(X[:, 1])] == 0).all()
    for rows, tile in [(1, 1), (64, 5), (777, 32), (5000, 7)]:
        assert np.array_equal(device_bins_np(P, X, flat, off, ncut, _rows_per_wg=rows, _feat_tile=tile), want), \
            f"rows_per_wg {rows} feat_tile {tile}"


def test_cut_tables_checked_before_any_launch():
    P = _P()
    flat = np.arange(300, dtype=np.float64)
    for off, ncut in [([0], [256]), ([100], [250]), ([-1], [5]), ([0], [-1]), ([0, 1], [1])]:
        with pytest.raises(ValueError, match="cut"):
            P.CutTables(flat, np.array(off, np.int32), np.array(ncut, np.int32), DEV)
    with pytest.raises(ValueError, match="geometry"):
        P.device_bins(up(np.zeros((4, 1))), P.CutTables(flat, np.array([0], np.int32), np.array([5], np.int32), DEV),
                      _feat_tile=33)


# ---- prediction

def _table(n, f, seed, nan=0.1):
    r = np.random.default_rng(seed)
    X = r.standard_normal((n, f))
    y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.3, n)
    X[r.random(X.shape) < nan] = np.nan
    return X, y


@pytest.fixture(scope="module")
def models():
    """Forests grown by the host learner (device=None), once for the module."""
    X, y = _table(3000, 6, seed=21)
    Xe, ye = _table(500, 6, seed=22)
    Xd, _ = _table(5000, 4, seed=23, nan=0.05)
    yd = np.nan_to_num(Xd[:, 0] + 0.5 * Xd[:, 1])  # smooth in two features: balanced splits down to depth 12
    out = {
        "forest": XGBRegressor(n_estimators=40).fit(X, y),  # more nodes than one LDS chunk holds
        "deep": XGBRegressor(n_estimators=3, max_depth=12, min_child_weight=0, reg_lambda=0.0).fit(Xd, yd),
        "stopped": XGBRegressor(n_estimators=60, learning_rate=0.3).fit(X[:400], y[:400], eval_set=[(Xe, ye)],
                                                                        early_stopping_rounds=5),
        "empty": XGBRegressor(n_estimators=0).fit(X, y),
    }
    P = _P()
    assert sum(len(t[0]) for t in out["forest"]._trees) > P.NODES_PER_CHUNK
    assert max(len(t[0]) for t in out["deep"]._trees) > P.NODES_PER_CHUNK
    s = out["stopped"]
    assert s.best_iteration is not None and s.best_iteration + 1 < s.n_trees_
    assert out["empty"].n_trees_ == 0
    return out


def predict_inputs(model, n, seed):
    """[n, f]: 10 % NaN, +-inf, and values equal to the forest's thresholds in their features."""
    r = np.random.default_rng(seed)
    X = r.standard_normal((n, model._nfeat))
    pairs = [(f, t) for tr in model._trees for f, t in zip(tr[0], tr[1]) if f >= 0]
    for i in range(n if pairs else 0):  # one threshold per row, in the feature that uses it
        f, t = pairs[r.integers(0, len(pairs))]
        X[i, f] = t
    X[r.random(X.shape) < 0.1] = np.nan
    X[r.random(X.shape) < 0.03] = np.inf
    X[r.random(X.shape) < 0.03] = -np.inf
    return X


@pytest.mark.parametrize("n", [1, 64, 65, 1000, 5000])
@pytest.mark.parametrize("name", ["forest", "deep", "stopped", "empty"])
def test_predict_equals_host(models, name, n):
    m = models[name]
    X = predict_inputs(m, n, seed=n)
    for Xh in (X, X.astype(np.float32)):
        want = m.predict(Xh.astype(np.float64))  # the host walk (mifx_gbdt_predict); float32: its exact widening
        got = m.predict(up(Xh))
        assert isinstance(got, torch.Tensor) and got.device == DEV and got.dtype == torch.float64
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), f"{name} n {n} {Xh.dtype}"
    if name == "empty":
        assert (want == m._base_margin).all()
    if name == "stopped":  # best_iteration limits the trees, as on the host
        every = m._predict_trees(X, m._trees, m._base_margin)
        assert not np.array_equal(every, want)


def test_predict_geometry_independent(models):
    P = _P()
    for name in ("forest", "deep", "stopped"):
        m = models[name]
        X = predict_inputs(m, 1000, seed=3)
        want = bits(m._predict_trees(X, m._trees, m._base_margin))
        forest = P.DeviceForest(m._trees, m._nfeat, DEV)
        sizes = [len(t[0]) for t in m._trees]
        chunks = [1, min(sizes) - 1 if min(sizes) > 1 else 1, max(sizes), sum(sizes) // 2 + 1, 2730]
        for chunk in chunks:  # below one tree: all from global memory; mid-way: the forest split between two chunks
            chunk = min(chunk, 2730)
            got = P.predict(forest, up(X), m._base_margin, _nodes_per_chunk=chunk)
            assert np.array_equal(bits(got.cpu().numpy()), want), f"{name}: nodes_per_chunk {chunk}"
        for k in (0, 1, len(sizes) // 2):
            got = P.predict(forest, up(X), m._base_margin, k, _nodes_per_chunk=min(max(sizes), 2730))
            assert np.array_equal(bits(got.cpu().numpy()), bits(m._predict_trees(X, m._trees[:k], m._base_margin)))


def test_malformed_forest_raises_before_any_launch(models, monkeypatch):
    P = _P()
    monkeypatch.setitem(P._fns(), "predict", lambda *a: pytest.fail("the kernel was launched"))
    good = models["stopped"]._trees[0]
    assert len(good[0]) >= 3 and good[0][0] >= 0
    X = up(np.zeros((4, 6)))

    def broken(k, **change):
        t = [a.copy() for a in good]
        for key, v in change.items():
            t[{"feature": 0, "left": 3, "right": 4}[key]][k] = v
        return tuple(t)

    c = len(good[0])
    for bad in (broken(0, left=c), broken(0, right=c + 7), broken(0, right=-1), broken(0, feature=6),
                broken(0, left=0), broken(int(good[3][0]), feature=0, left=int(good[3][0]), right=c - 1)):
        with pytest.raises(ValueError, match="tree 1"):
            P.DeviceForest([good, bad], 6, DEV)
        m = XGBRegressor()
        m._trees, m._nfeat, m._base_margin = [good, bad], 6, 0.0
        with pytest.raises(ValueError, match="tree 1"):
            m.predict(X)


# ---- end to end

def _reg_data():
    r = np.random.default_rng(8)
    X = r.normal(size=(900, 6))
    y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.1, 900)
    X[r.random(X.shape) < 0.1] = np.nan
    return X[:600], y[:600], X[600:], y[600:]


def _same_model(a, b):
    assert a.n_trees_ == b.n_trees_ and a.n_trees_ > 10
    for t, (ta, tb) in enumerate(zip(a._trees, b._trees)):
        for u, v in zip(ta, tb):
            assert u.dtype == v.dtype and np.array_equal(u, v), f"tree {t}"
    assert a.evals_result_ == b.evals_result_
    assert a.best_iteration == b.best_iteration and a.best_score == b.best_score and a._base_margin == b._base_margin
    assert all(np.array_equal(u, v) for u, v in zip(a._cuts, b._cuts))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_regressor_fit_and_predict_on_device_tensors(dtype):
    X, y, Xe, ye = (a.astype(dtype) for a in _reg_data())
    kw = dict(n_estimators=60, learning_rate=0.3)
    fit = dict(early_stopping_rounds=10)
    wide = [a.astype(np.float64) for a in (X, y, Xe, ye)]  # float32 means its exact widening
    a = XGBRegressor(device="gpu", **kw).fit(up(X), up(y), eval_set=[(up(Xe), up(ye))], **fit)
    b = XGBRegressor(device="gpu", **kw).fit(wide[0], wide[1], eval_set=[(wide[2], wide[3])], **fit)
    c = XGBRegressor(device="cpu", fixed_point=True, **kw).fit(wide[0], wide[1], eval_set=[(wide[2], wide[3])], **fit)
    d = XGBRegressor(device="gpu", **kw).fit(torch.from_numpy(X), torch.from_numpy(y),  # CPU tensors
                                             eval_set=[(torch.from_numpy(Xe), torch.from_numpy(ye))], **fit)
    _same_model(a, b)
    _same_model(a, c)
    _same_model(a, d)
    got = a.predict(up(Xe))
    assert isinstance(got, torch.Tensor) and got.device == DEV
    assert torch.equal(got, up(c.predict(wide[2])))
    assert torch.equal(c.predict(up(Xe)), got)  # a model trained on the host predicts on the device too
    assert isinstance(a.predict(Xe), np.ndarray) and np.array_equal(a.predict(wide[2]), c.predict(wide[2]))


def test_refit_rebuilds_the_device_forest_and_pickle_drops_it():
    import pickle

    X, y, Xe, _ = _reg_data()
    m = XGBRegressor(device="gpu", n_estimators=5).fit(X, y)
    first = m.predict(up(Xe))
    assert m._dev_forest and "_dev_forest" not in m.__getstate__()
    back = pickle.loads(pickle.dumps(m))
    assert torch.equal(back.predict(up(Xe)), first) and np.array_equal(back.predict(Xe), first.cpu().numpy())
    m.fit(X, -y)
    assert torch.equal(m.predict(up(Xe)), up(m.predict(Xe))) and not torch.equal(m.predict(up(Xe)), first)


def test_classifier_on_device_tensors_planted_rule():
    r = np.random.default_rng(9)
    n = 2000
    X = r.integers(0, 10, (n, 5)).astype(np.float64)
    y = np.where((X[:, 0] >= 5) & (X[:, 1] >= 5), "b", "a")
    keep = np.concatenate([np.flatnonzero(y == "a")[:300], np.flatnonzero(y == "b")[:300]])
    X, y = X[keep], y[keep]
    kw = dict(n_estimators=20, max_depth=2, learning_rate=0.3)
    a = XGBClassifier(device="gpu", **kw).fit(up(X), y, eval_set=[(up(X), y)])
    b = XGBClassifier(device="gpu", **kw).fit(X, y, eval_set=[(X, y)])
    h = XGBClassifier(device="cpu", fixed_point=True, **kw).fit(X, y, eval_set=[(X, y)])
    for other in (b, h):
        for ta, tb in zip(a._trees, other._trees):
            assert all(np.array_equal(u, v) for u, v in zip(ta, tb))
        assert a.evals_result_ == other.evals_result_ and a.n_trees_ == other.n_trees_ == 20
    ynum = up((y == "b").astype(np.float64))  # labels as a device tensor
    e = XGBClassifier(device="gpu", **kw).fit(up(X), ynum, eval_set=[(up(X), ynum)])
    assert e.evals_result_ == a.evals_result_ and list(e.classes_) == [0.0, 1.0]
    margin = a._margin(up(X))
    assert np.array_equal(bits(margin.cpu().numpy()), bits(h._margin(X)))
    labels = a.predict(up(X))
    assert isinstance(labels, np.ndarray) and (labels == y).all() and (labels == h.predict(X)).all()
    proba = a.predict_proba(up(X))
    assert isinstance(proba, torch.Tensor) and proba.device == DEV and tuple(proba.shape) == (len(y), 2)
    err = np.abs(proba.cpu().numpy() - h.predict_proba(X)).max()
    print(f"predict_proba, torch on the device against numpy on the host: max |d| {err:.3g} (bound 1e-12)")
    assert err <= 1e-12  # torch's exp against numpy's, not a kernel tolerance
    assert a.evals_result_["validation_0"]["logloss"][-1] < math.log(2)


def test_gpu_fit_from_numpy_never_calls_the_host_cuts_or_bins(monkeypatch):
    def refuse(*a):
        raise AssertionError("the host preparation was called on the device path")

    lib = xgb._lib()
    X, y, Xe, ye = _reg_data()
    want = XGBRegressor(device="cpu", fixed_point=True, n_estimators=8).fit(X, y, eval_set=[(Xe, ye)])
    monkeypatch.setattr(lib, "mifx_gbdt_cuts", refuse)
    monkeypatch.setattr(lib, "mifx_gbdt_bin", refuse)
    got = XGBRegressor(device="gpu", n_estimators=8).fit(X, y, eval_set=[(Xe, ye)])
    assert got.evals_result_ == want.evals_result_
    for ta, tb in zip(got._trees, want._trees):
        assert all(np.array_equal(u, v) for u, v in zip(ta, tb))
    assert np.array_equal(got.predict(Xe), want.predict(Xe))


def test_device_tensors_on_the_wrong_device_raise():
    X, y, Xe, ye = _reg_data()
    for model in (XGBRegressor(n_estimators=2), XGBRegressor(device="cpu", n_estimators=2),
                  XGBClassifier(n_estimators=2)):
        with pytest.raises(ValueError, match='device="gpu"'):
            model.fit(up(X), y)
        with pytest.raises(ValueError, match='device="gpu"'):
            model.fit(X, y, eval_set=[(up(Xe), ye)])
    with pytest.raises(ValueError, match="max_bins"):  # the limits still come before any launch
        XGBRegressor(device="gpu", max_bins=257).fit(up(X), up(y))
    with pytest.raises(ValueError, match="max_depth"):
        XGBRegressor(device="gpu", max_depth=13).fit(up(X), up(y))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a tensor on another GPU than device=")
def test_device_tensors_on_another_gpu_raise():
    X, y, _, _ = _reg_data()
    other = torch.from_numpy(X).to(torch.device("cuda", 1))
    with pytest.raises(ValueError, match="cuda:1"):
        XGBRegressor(device="cuda:0", n_estimators=2).fit(other, y)
    with pytest.raises(ValueError, match="cuda:0"):
        XGBRegressor(device="cuda:1", n_estimators=2).fit(up(X), y)
