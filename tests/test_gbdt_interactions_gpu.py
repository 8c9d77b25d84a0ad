"""predict_interactions on the device (csrc/gbdt_interactions.hip, k_interactions) against the host function
mifx_gbdt_interactions: exact equality of the bit patterns for float32 and float64 tables, any tree limit, chunk
size, workgroup size and accumulation route; then a model fitted on the device end to end."""
import numpy as np
import pytest
import torch

from mifx.gbdt import XGBClassifier, XGBRegressor, shap
from test_gbdt_contribs_cpu import max_depth_of, probe_rows, table

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def same_bits(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


def rows_of(X, n):
    """n rows: ordinary ones (~10 % NaN), then all-NaN, all-+inf and all--inf where there is room."""
    return np.resize(probe_rows(X, max(1, n - 3)), (n, X.shape[1]))


@pytest.fixture(scope="module")
def forests():
    """Host-trained models, the table each was trained on, and the host's result on 70 rows of it."""
    out = {}
    X, y = table(1000, 6, 3)
    out["f6"] = XGBClassifier(n_estimators=4, max_depth=8, fixed_point=True).fit(X, y > 0.2), X
    r = np.random.default_rng(22)
    X = r.normal(size=(1000, 14))
    y = np.sin(3 * X[:, 0]) * X[:, 1] + np.abs(X[:, 2] - X[:, 3]) + np.cos(X[:, 4] * X[:, 5]) + X[:, 6:].sum(1)
    X[r.random(X.shape) < 0.1] = np.nan
    out["deep"] = XGBRegressor(n_estimators=2, max_depth=12).fit(X, y), X
    X = r.normal(size=(300, 300))
    y = X[:, :40].sum(1) + X[:, 299] * X[:, 150]
    X[r.random(X.shape) < 0.1] = np.nan
    out["wide"] = XGBRegressor(n_estimators=3, max_depth=4).fit(X, y), X
    X, y = table(600, 5, 23)
    out["k3"] = XGBClassifier(n_estimators=3, max_depth=4).fit(X, np.digitize(y, [-0.4, 0.6])), X
    return {k: (m, X, m.predict_interactions(rows_of(X, 70))) for k, (m, X) in out.items()}


def test_forests_are_the_cases_meant(forests):
    from mifx.ops import gbdt_prep as P

    deep = forests["deep"][0]._path_tables(2)[0]
    assert deep.recs["i"][deep.leaf_off[:-1]].max() == shap.MAX_PATH and max_depth_of(forests["deep"][0]._trees[0]) == 12
    off = forests["wide"][0]._path_tables(3)[0].feature_leaves()[0]
    assert P.contrib_lds_threads(300) == 0 and (np.diff(off) == 0).sum() > 150  # output rows only; mostly empty lists
    assert P.contrib_lds_threads(6) == 256 and forests["k3"][0]._num_class() == 3
    off, _, _, rec = forests["f6"][0]._path_tables(4)[0].feature_leaves()
    assert np.diff(rec[off]).min() > P.RECS_PER_CHUNK  # every list spans chunks, even at the default size


@pytest.mark.parametrize("n", [1, 63, 65, 257])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_kernel_equals_host_function_bit_for_bit(forests, n, dtype):
    m, X, _ = forests["f6"]
    rows = torch.from_numpy(rows_of(X, n)).to(dtype)
    want = m.predict_interactions(rows.numpy())
    got = m.predict_interactions(rows.to(DEV))
    assert isinstance(got, torch.Tensor) and got.device == DEV and got.dtype == torch.float64
    assert want.shape == (n, 7, 7) and same_bits(got, want)


@pytest.mark.parametrize("name", ["deep", "wide", "k3"])
def test_kernel_on_deep_wide_and_multiclass_forests(forests, name):
    m, X, want = forests[name]
    K, w = m._num_class(), X.shape[1] + 1
    assert want.shape == ((70, w, w) if K == 1 else (70, K, w, w))
    rows = torch.from_numpy(rows_of(X, 70)).to(DEV)
    assert same_bits(m.predict_interactions(rows), want)
    assert same_bits(m.predict_interactions(rows, _recs_per_chunk=13), want), "the smallest chunk: one leaf at a time"
    if name == "wide":
        with pytest.raises(ValueError, match="LDS"):
            m.predict_interactions(rows, _route="lds")


@pytest.mark.parametrize("n_trees", [0, 1, 4])
def test_kernel_tree_limits(forests, n_trees):
    from mifx.ops import gbdt_prep as P

    m, X, _ = forests["f6"]
    rows = rows_of(X, 65)
    tab = m._path_tables(4)[0]
    want = np.empty((65, 7, 7))
    shap.interactions(tab, rows, n_trees, m._base_margin, want, 4)
    got = torch.full((65, 7, 7), np.nan, dtype=torch.float64, device=DEV)
    P.interactions(P.DevicePaths(tab, DEV), torch.from_numpy(rows).to(DEV), m._base_margin, got, n_trees)
    assert same_bits(got, want)
    assert n_trees or (not want[:, :6].any() and (want[:, 6, 6] == m._base_margin).all())


@pytest.mark.parametrize("route", ["lds", "output"])
@pytest.mark.parametrize("threads", [64, 128, 256])
@pytest.mark.parametrize("chunk", [13, None])
def test_geometry_does_not_change_a_bit(forests, route, threads, chunk):
    m, X, want = forests["f6"]
    rows = torch.from_numpy(rows_of(X, 70)).to(DEV)
    assert same_bits(m.predict_interactions(rows, _recs_per_chunk=chunk, _route=route, _threads=threads), want)


def test_gpu_model_end_to_end():
    X, y = table(1000, 6, 31)
    m = XGBRegressor(device="gpu", n_estimators=6, subsample=0.8, random_state=5).fit(X, y)
    P = probe_rows(X, 297)
    got = m.predict_interactions(torch.from_numpy(P).to(DEV))
    assert isinstance(got, torch.Tensor) and got.device == DEV and got.shape == (300, 7, 7)
    assert same_bits(got, m.predict_interactions(P))
    assert "_dev_paths" not in m.__getstate__() and "_paths" not in m.__getstate__()
