"""What the device preparation / prediction of mifx.gbdt must leave alone on a host without a GPU: the default path
does not import torch, a pickled model predicts from numpy, and the forest validator of mifx/ops/gbdt_prep.py accepts
every tree the host learner grows and refuses the ones a kernel could not walk."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, XGBRegressor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_importing_the_package_does_not_import_torch():
    code = "import sys; import mifx.gbdt; from mifx.gbdt import XGBRegressor; XGBRegressor(); " \
           "sys.exit(1 if 'torch' in sys.modules else 0)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def _data():
    r = np.random.default_rng(3)
    X = r.normal(size=(400, 5))
    y = X[:, 0] * X[:, 1] + r.normal(0, 0.1, 400)
    X[r.random(X.shape) < 0.1] = np.nan
    return X, y


def test_pickled_model_has_no_device_cache_and_predicts_from_numpy():
    X, y = _data()
    for m in (XGBRegressor(n_estimators=5).fit(X, y), XGBClassifier(n_estimators=5).fit(X, y > 0)):
        m._dev_forest = {0: object()}  # what a device predict leaves behind; never pickled
        state = m.__getstate__()
        assert "_dev_forest" not in state and "_trees" in state
        back = pickle.loads(pickle.dumps(m))
        assert not hasattr(back, "_dev_forest") and np.array_equal(back.predict(X), m.predict(X))
        m.fit(X, y > 0 if isinstance(m, XGBClassifier) else y)
        assert m._dev_forest is None  # a fit drops the stale device copy


def test_cpu_tensors_take_the_host_path():
    import torch

    X, y = _data()
    a = XGBRegressor(n_estimators=5).fit(X, y)
    b = XGBRegressor(n_estimators=5).fit(torch.from_numpy(X), torch.from_numpy(y))
    got = b.predict(torch.from_numpy(X))
    assert isinstance(got, np.ndarray) and np.array_equal(got, a.predict(X))


def _forest(seed, fixed):
    trees, nfeat = [], 0
    for n, f in C.SHAPES:
        bins, nbins = C.make_bins(n, f, seed + n + f)
        g, h = C.float_grads(n, seed + n)
        for depth, mcw, gamma in C.PARAMS:
            fe, sb, dl, le, ri, val, _ = C.host_grow(bins, nbins, g, h, depth, mcw, gamma, fixed=fixed)
            trees.append((fe, sb.astype(np.float64), dl, le, ri, val))
            nfeat = max(nfeat, f)
    return trees, nfeat


def test_validator_accepts_what_the_host_learner_grows():
    from mifx.ops import gbdt_prep as P

    for fixed in (False, True):
        trees, nfeat = _forest(1, fixed)
        assert max(len(t[0]) for t in trees) > 15
        P.validate_forest(trees, nfeat)
    X, y = _data()
    m = XGBRegressor(n_estimators=4, max_depth=12, min_child_weight=0).fit(X, y)
    P.validate_forest(m._trees, 5)
    P.validate_forest([], 5)


def test_validator_rejects_malformed_trees():
    from mifx.ops import gbdt_prep as P

    i32, f64 = np.int32, np.float64
    good = (np.array([0, -1, -1], i32), np.zeros(3, f64), np.zeros(3, np.uint8), np.array([1, -1, -1], i32),
            np.array([2, -1, -1], i32), np.zeros(3, f64))
    P.validate_forest([good], 1)

    def with_(idx, k, v):
        t = [a.copy() for a in good]
        t[idx][k] = v
        return tuple(t)

    bad = [with_(3, 0, 3), with_(4, 0, 3), with_(4, 0, -1), with_(3, 0, 0), with_(4, 0, 0), with_(0, 0, 1),
           with_(0, 2, 0),  # an inner node whose children (-1, -1) are not after it
           tuple(a[:0] for a in good), (good[0],) + tuple(a[:2] for a in good[1:])]
    for t in bad:
        with pytest.raises(ValueError, match="tree 1"):
            P.validate_forest([good, t], 1)
