"""Node statistics and feature contributions on the device: the grower's gain and cover (csrc/gbdt_gpu.hip) against
the host fixed-point twin, and the contribution kernel (csrc/gbdt_prep.hip, k_contribs) against the host function
mifx_gbdt_contribs -- exact equality of the bit patterns for any chunk size, either accumulation route, float32 and
float64 tables; then XGB*(device="gpu") end to end."""
import numpy as np
import pytest
import torch

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, XGBRegressor, shap, xgb
from mifx.gbdt import sample as S
from test_gbdt_contribs_cpu import grow_stats, leaf_scale, max_depth_of, probe_rows, table

pytestmark = pytest.mark.gpu

NS = [1, 2, 63, 65, 257, 5000]
DEV = torch.device("cuda", 0)


def _G():
    from mifx.ops import gbdt_gpu

    return gbdt_gpu


def _P():
    from mifx.ops import gbdt_prep

    return gbdt_prep


def same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


# ---- the grower's statistics

@pytest.mark.parametrize("n,f", [(n, f) for n in NS for f in C.FS])
def test_device_grower_statistics_equal_host_twin(n, f):
    G = _G()
    seed = n * 17 + f
    bins, nbins = C.make_bins(n, f, seed)
    g, h = C.float_grads(n, seed)
    for depth in (0, 1, 6):
        bst = G.Booster(bins, nbins, depth, DEV)
        calls = [dict(), dict(_rows_per_wg=64, _feat_tile=1), dict(_rows_per_wg=5000, _feat_tile=12)]
        if depth > 0:
            rnd = 1 if n > 2 else next(r for r in range(64) if S.row_mask(seed, r, 0.5, n).any())
            calls.append(dict(subsample=0.5, seed=seed, round=rnd,
                              level_mask=S.level_mask(seed, rnd, f, depth, 0.7, 0.7)))
        for kw in calls:
            what = f"depth {depth} {sorted(kw)}"
            plain = G.grow_numpy(bins, nbins, g, h, depth, _booster=bst, **kw)
            got = G.grow_numpy(bins, nbins, g, h, depth, _booster=bst, stats=True, **kw)
            C.assert_same_tree(got[:7], plain, what + ": with and without stats")
            rows = xgb.sample_rows(kw["seed"], kw["round"], 0.5, n) if "subsample" in kw else None
            want = grow_stats(bins, nbins, g, h, depth, fixed=True, rows=rows, mask=kw.get("level_mask"))
            C.assert_same_tree(got[:7], want[:7], what)
            assert same_bits(got[7], want[7]), what + ": gain"
            assert same_bits(got[8], want[8]), what + ": cover"


# ---- the contribution kernel

def _forests():
    """Host-trained models (the kernel reads any model's table) and the table each was trained on."""
    out = {}
    X, y = table(1000, 6, 21)
    out["f6"] = (XGBRegressor(n_estimators=8, max_depth=6).fit(X[:700], y[:700], eval_set=[(X[700:], y[700:])]), X)
    out["f6"][0].best_iteration = 4  # a tree limit below the forest, as early stopping leaves it
    r = np.random.default_rng(22)
    X = r.normal(size=(1000, 11))
    y = np.sin(3 * X[:, 0]) * X[:, 1] + np.abs(X[:, 2] - X[:, 3]) + np.cos(X[:, 4] * X[:, 5]) + X[:, 6:].sum(1)
    X[r.random(X.shape) < 0.1] = np.nan
    out["depth12"] = (XGBRegressor(n_estimators=2, max_depth=12).fit(X, y), X)
    X = r.normal(size=(300, 300))
    y = X[:, :40].sum(1) + X[:, 299] * X[:, 150]
    X[r.random(X.shape) < 0.1] = np.nan
    out["f300"] = (XGBRegressor(n_estimators=3, max_depth=4).fit(X, y), X)
    X, y = table(600, 5, 23)
    out["k3"] = (XGBClassifier(n_estimators=3, max_depth=4).fit(X, np.digitize(y, [-0.4, 0.6])), X)
    X, y = table(900, 4, 24)
    labels = np.digitize(y, np.quantile(y, np.linspace(0, 1, 18)[1:-1]))  # 17 classes of equal size
    out["k17"] = (XGBClassifier(n_estimators=2, max_depth=3).fit(X, labels), X)
    return out


@pytest.fixture(scope="module")
def forests():
    return _forests()


@pytest.fixture(scope="module")
def host_contribs(forests):
    """The host function's result for every forest on its probe rows, computed once."""
    return {k: m.predict_contribs(_rows(X, 1000)) for k, (m, X) in forests.items()}


def _rows(X, n):
    """n rows: ordinary ones (~10 % NaN), and among the first 60 an all-NaN, an all-+inf and an all--inf row."""
    P = np.resize(X, (n, X.shape[1])).copy()
    for i, v in zip((min(n - 1, 7), min(n - 1, 31), min(n - 1, 59)), (np.nan, np.inf, -np.inf)):
        P[i] = v
    return P


def test_forests_are_the_cases_meant(forests):
    P = _P()
    m = forests["f6"][0]
    assert shap.PathTable(m._trees, [s[1] for s in m._node_stats], 6).n_recs(8) > 2 * P.RECS_PER_CHUNK
    assert max(max_depth_of(t) for t in forests["depth12"][0]._trees) == 12
    assert P.contrib_lds_threads(6) == 256 and P.contrib_lds_threads(300) == 0
    assert forests["k3"][0]._num_class() == 3 and forests["k17"][0]._num_class() == 17 > P._fns()["reg_classes"]()


@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_kernel_equals_host_function_bit_for_bit(forests, n, dtype):
    m, X = forests["f6"]
    rows = torch.from_numpy(_rows(X, n)).to(dtype)
    want = m.predict_contribs(rows.numpy())
    assert want.shape == (n, 7)
    got = m.predict_contribs(rows.to(DEV))
    assert isinstance(got, torch.Tensor) and got.device == DEV and got.dtype == torch.float64
    assert same_bits(got, want)
    for route in ("lds", "output"):
        for chunk in (13, 100, None):
            assert same_bits(m.predict_contribs(rows.to(DEV), _recs_per_chunk=chunk, _route=route), want), \
                f"route {route} chunk {chunk}"


@pytest.mark.parametrize("name", ["depth12", "f300", "k3", "k17"])
def test_kernel_on_deep_wide_and_multiclass_forests(forests, host_contribs, name):
    m, X = forests[name]
    want = host_contribs[name]
    K, f = m._num_class(), X.shape[1]
    assert want.shape == ((1000, f + 1) if K == 1 else (1000, K, f + 1))
    rows = torch.from_numpy(_rows(X, 1000)).to(DEV)
    assert same_bits(m.predict_contribs(rows), want)
    assert same_bits(m.predict_contribs(rows, _recs_per_chunk=13), want), "the smallest chunk: one leaf at a time"
    assert same_bits(m.predict_contribs(rows, _route="output"), want)
    if name == "f300":
        with pytest.raises(ValueError, match="LDS"):
            m.predict_contribs(rows, _route="lds")
    with pytest.raises(ValueError, match="geometry"):
        m.predict_contribs(rows, _recs_per_chunk=12)


def test_kernel_tree_limits(forests):
    P = _P()
    m, X = forests["f6"]
    rows = _rows(X, 257)
    tab = shap.PathTable(m._trees, [s[1] for s in m._node_stats], 6)
    paths = P.DevicePaths(tab, DEV)
    Xd = torch.from_numpy(rows).to(DEV)
    results = []
    for n_trees in (0, m._tree_limit(), len(m._trees)):
        want = np.empty((257, 7))
        shap.contribs(tab, rows, n_trees, m._base_margin, want, 4)
        got = torch.full((257, 7), np.nan, dtype=torch.float64, device=DEV)
        P.contribs(paths, Xd, m._base_margin, got, n_trees)
        assert same_bits(got, want), f"{n_trees} trees"
        results.append(want)
    assert not results[0][:, :6].any() and (results[0][:, 6] == m._base_margin).all()
    assert same_bits(m.predict_contribs(Xd), results[1]) and not np.array_equal(results[1], results[2])
    with pytest.raises(ValueError, match="n_trees"):
        P.contribs(paths, Xd, 0.0, got, 9)
    for route in ("lds", "output"):  # smaller workgroups (wide tables accumulate in LDS with them)
        for threads in (64, 128):
            got.fill_(np.nan)
            P.contribs(paths, Xd, m._base_margin, got, None, 40, route, threads)
            assert same_bits(got, results[2]), f"route {route}, {threads} threads"
    with pytest.raises(ValueError, match="LDS"):
        P.contribs(paths, Xd, 0.0, got, None, None, "lds", 96)


def test_wide_table_accumulates_in_lds_with_a_smaller_workgroup():
    """f = 40: 256 threads' sums do not fit beside the chunk, 128 threads' do; the default takes them."""
    P = _P()
    r = np.random.default_rng(41)
    X = r.normal(size=(400, 40))
    y = X[:, :10].sum(1) + X[:, 39] * X[:, 20]
    X[r.random(X.shape) < 0.1] = np.nan
    m = XGBRegressor(n_estimators=3, max_depth=5).fit(X, y)
    assert P.contrib_lds_threads(40) == 128
    want = m.predict_contribs(X)
    Xd = torch.from_numpy(X).to(DEV)
    assert same_bits(m.predict_contribs(Xd), want) and same_bits(m.predict_contribs(Xd, _route="output"), want)


# ---- end to end

def _fit_pair(cls, X, y, **kw):
    a = cls(device="gpu", **kw).fit(X, y)
    b = cls(device="cpu", fixed_point=True, **kw).fit(X, y)
    assert a.n_trees_ == b.n_trees_ > 0
    for ta, tb in zip(a._trees, b._trees):
        for u, v in zip(ta, tb):
            assert np.array_equal(u, v)
    return a, b


@pytest.mark.parametrize("kind", ["regressor", "three_classes"])
def test_gpu_model_end_to_end(kind):
    X, y = table(1000, 6, 31)
    if kind == "regressor":
        a, b = _fit_pair(XGBRegressor, X, y, n_estimators=10, subsample=0.8, random_state=5)
    else:
        a, b = _fit_pair(XGBClassifier, X, np.digitize(y, [-0.4, 0.6]), n_estimators=10)
    K = a._num_class()
    assert len(a._node_stats) == a.n_trees_ == 10 * K
    for (ga, ca), (gb, cb) in zip(a._node_stats, b._node_stats):
        assert same_bits(ga, gb) and same_bits(ca, cb)
    for kind_ in ("weight", "gain", "cover", "total_gain", "total_cover"):
        assert a.get_score(kind_) == b.get_score(kind_)
    assert np.array_equal(a.feature_importances_, b.feature_importances_) and a.feature_importances_.sum() > 0.99
    P = probe_rows(X, 997)
    Pd = torch.from_numpy(P).to(DEV)
    got = a.predict_contribs(Pd)
    assert isinstance(got, torch.Tensor) and got.device == DEV
    assert got.shape == ((1000, 7) if K == 1 else (1000, 3, 7))
    assert same_bits(got, a.predict_contribs(P))
    assert same_bits(b.predict_contribs(Pd), a.predict_contribs(P)), "a host-trained model on the device"
    margins = (a._margins(Pd) if K > 1 else a._margin(Pd)[None]).cpu().numpy()
    c = got.cpu().numpy().reshape(1000, K, 7)
    for k in range(K):
        err = np.abs(c[:, k].sum(-1) - margins[k]).max()
        bound = 1e-12 * leaf_scale(a._trees[k::K])
        print(f"{kind} class {k}: max |sum(phi) - margin| = {err:.3g} (bound {bound:.3g})")
        assert err <= bound
    assert a._dev_paths is not None and "_dev_paths" not in a.__getstate__()
