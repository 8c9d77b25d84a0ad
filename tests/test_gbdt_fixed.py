"""Fixed-point GBDT on the host: the twin mifx_gbdt_grow_fixed against the double learner on exactly representable
gradients, the quantisation exponent, XGBRegressor(device="cpu", fixed_point=True) end to end, the device / fixed_point
interface without a GPU, and the stand-alone sanitizer harness of the twin."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gbdt_cases as C
from mifx.gbdt import XGBClassifier, XGBRegressor, xgb

ROOT = os.path.join(os.path.dirname(__file__), "..")


@pytest.mark.parametrize("n,f", C.SHAPES)
def test_fixed_twin_equals_double_learner_on_dyadic_gradients(n, f):
    bins, nbins = C.make_bins(n, f, seed=n * 31 + f)
    g, h = C.dyadic_grads(n, seed=n * 31 + f)
    for depth, mcw, gamma in C.PARAMS:
        want = C.host_grow(bins, nbins, g, h, depth, mcw, gamma, fixed=False)
        got = C.host_grow(bins, nbins, g, h, depth, mcw, gamma, fixed=True)
        C.assert_same_tree(got, want, f"depth {depth} mcw {mcw} gamma {gamma}")


def test_fixed_twin_level_of_leaves_before_max_depth():
    """Every node of level 1 turns leaf (two rows: one split, then single-row children) far above max_depth; and a
    tree whose root has no gain at all (g = 0)."""
    bins = np.array([[0, 1]], np.uint16)
    nbins = np.array([2], np.int32)
    g, h = np.array([-1.0, 1.0], np.float32), np.ones(2, np.float32)
    a = C.host_grow(bins, nbins, g, h, 6, 0.0, 0.0, fixed=True)
    C.assert_same_tree(a, C.host_grow(bins, nbins, g, h, 6, 0.0, 0.0, fixed=False))
    assert len(a[0]) == 3 and a[0][0] == 0
    bins, nbins = C.make_bins(300, 3, seed=1)
    z = C.host_grow(bins, nbins, np.zeros(300, np.float32), np.ones(300, np.float32), 6, 1.0, 0.0, fixed=True)
    assert len(z[0]) == 1 and z[5][0] == 0.0 and not z[6].any()


def test_quant_exp_formula_and_sum_bound():
    lib = xgb._lib()
    for amax in [0.0, float("inf"), float("nan")]:
        assert lib.mifx_gbdt_quant_exp(amax, 1000) == 0
    for amax in [1.0, 0.75, 4.0, 3.999, 1e-30, 1e30, float(np.float32(1e-45)), float(np.finfo(np.float32).max)]:
        for n in [1, 2, 3, 4096, 5000, 2 ** 31 - 1]:
            assert lib.mifx_gbdt_quant_exp(amax, n) == C.quant_exp_ref(amax, n), (amax, n)
    assert lib.mifx_gbdt_quant_exp(1.0, 1) == 60 - 1 - 1 and lib.mifx_gbdt_quant_exp(4.0, 4096) == 60 - 13 - 3
    # n rows all equal to amax: the quantised sum stays below 2^61 (python integers: no overflow in the check itself)
    n = 4096
    for a in [np.float32(1e-30), np.float32(1e30)]:
        e = lib.mifx_gbdt_quant_exp(float(a), n)
        q = int(np.rint(np.ldexp(np.float64(a), e)))
        assert 0 < n * q < 2 ** 61 and n * q >= 2 ** 58  # and no more than 3 bits of headroom are wasted
    # the twin at 1e30: with h = 1 and lambda = 1 the huge gains split as deep as allowed, and a power-of-two
    # rescaling of g changes no decision (every G scales exactly), only the leaf values, by exactly that factor
    bins, nbins = C.make_bins(n, 3, seed=7)
    g, h = C.float_grads(n, seed=7)[0], np.ones(n, np.float32)
    ref = C.host_grow(bins, nbins, g, h, 3, 1.0, 0.0, fixed=True)
    big = C.host_grow(bins, nbins, g * np.float32(2.0 ** 100), h, 3, 1.0, 0.0, fixed=True)
    for k in (0, 1, 2, 3, 4, 6):
        assert np.array_equal(big[k], ref[k])
    assert np.array_equal(big[5], ref[5] * 2.0 ** 100) and len(ref[0]) > 3
    # all-zero g: exponent 0, one leaf of value 0
    z = C.host_grow(bins, nbins, np.zeros(n, np.float32), h, 3, 1.0, 0.0, fixed=True)
    assert len(z[0]) == 1 and z[5][0] == 0.0


def test_regressor_fixed_point_cpu_thread_independent_and_accurate():
    r = np.random.default_rng(5)  # the data of test_gbdt_deterministic_across_threads_and_binned
    X = r.normal(size=(30000, 12))
    y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + r.normal(0, 0.1, 30000)
    a = XGBRegressor(n_estimators=20, max_bins=64, n_jobs=1, device="cpu", fixed_point=True).fit(X, y)
    b = XGBRegressor(n_estimators=20, max_bins=64, n_jobs=8, device="cpu", fixed_point=True).fit(X, y)
    for ta, tb in zip(a._trees, b._trees):
        assert all(np.array_equal(u, v) for u, v in zip(ta, tb))
    assert np.array_equal(a.predict(X[:1000]), b.predict(X[:1000]))
    rmse = float(np.sqrt(np.mean((a.predict(X) - y) ** 2)))
    assert rmse < 0.35 * y.std()


def test_device_and_fixed_point_interface():
    for cls in (XGBRegressor, XGBClassifier):
        with pytest.raises(ValueError, match="fixed point"):
            cls(device="gpu", fixed_point=False)
        with pytest.raises(ValueError, match="device"):
            cls(device="tpu")
        assert cls()._fixed() is False and cls(device="cpu")._fixed() is False
        assert cls(device="cuda:0")._fixed() is True and cls(fixed_point=True)._gpu_index() is None
    X, y = np.random.default_rng(0).normal(size=(50, 2)), np.arange(50.0)
    if torch.cuda.is_available():
        assert XGBRegressor(n_estimators=2, device="gpu").fit(X, y).n_trees_ == 2
    else:
        with pytest.raises(RuntimeError, match="no GPU"):
            XGBRegressor(n_estimators=2, device="gpu").fit(X, y)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_gbdt_fixed_twin_sanitizers(tmp_path, san):
    """tools/sanitize/gbdt_fixed_fuzz.cpp: a stand-alone program over mifx_gbdt_grow_fixed (thread-count identity,
    identity with mifx_gbdt_grow on dyadic gradients, exact-size buffers) under ASan + UBSan and under TSan."""
    exe = str(tmp_path / "gbdt_fixed_fuzz")
    subprocess.run(["g++", "-O1", "-g", f"-fsanitize={san}", "-fno-omit-frame-pointer", "-std=c++17", "-pthread",
                    os.path.join(ROOT, "tools", "sanitize", "gbdt_fixed_fuzz.cpp"),
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
