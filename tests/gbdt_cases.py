"""Shared inputs of the fixed-point GBDT tests (tests/test_gbdt_fixed.py on the host, tests/test_gbdt_gpu.py on the
device): the shape grid, binned matrices with mixed bin counts and missing values, the gradients, and ctypes calls of
the two host growers."""
import itertools

import numpy as np

from mifx.gbdt import xgb

# rows: 1, 2, around a wave, around a workgroup, 1000, and 5000 > one workgroup's row chunk of a single node
NS = [1, 2, 63, 65, 257, 1000, 5000]
FS = [1, 3, 11]  # 11 > the device learner's feature tile (8)
SHAPES = list(itertools.product(NS, FS))
PARAMS = list(itertools.product([0, 1, 3, 6], [0.0, 1.0, 5.0], [0.0, 0.25]))  # max_depth, min_child_weight, gamma
BIN_KINDS = [5, 256, 1, 2, 64]  # 1: a constant feature without a candidate


def make_bins(n, f, seed):
    """Column-major [f, n] uint16 bins: bin counts cycle through BIN_KINDS, ~10 % missing, and with f >= 3 the last
    feature is missing in every row."""
    r = np.random.default_rng(seed)
    bins = np.empty((f, n), np.uint16)
    nbins = np.empty(f, np.int32)
    for j in range(f):
        nb = BIN_KINDS[(j + n) % len(BIN_KINDS)]
        col = r.integers(0, nb, n).astype(np.uint16)
        col[r.random(n) < 0.1] = 0xFFFF
        if f >= 3 and j == f - 1:
            nb, col[:] = 1, 0xFFFF
        bins[j], nbins[j] = col, nb
    return bins, nbins


def dyadic_grads(n, seed):
    """g = k / 256 with |k| <= 1024 and h = k / 64 with 1 <= k <= 64: every double sum over n <= 5000 rows and every
    quantisation is exact, so the double learner and the fixed-point ones must agree bit for bit."""
    r = np.random.default_rng(seed + 1)
    return ((r.integers(-1024, 1025, n) / 256.0).astype(np.float32),
            (r.integers(1, 65, n) / 64.0).astype(np.float32))


def float_grads(n, seed, scale=1.0):
    r = np.random.default_rng(seed + 2)
    return ((r.standard_normal(n) * scale).astype(np.float32),
            (r.uniform(0.1, 1.0, n) * scale).astype(np.float32))


def host_grow(bins, nbins, g, h, max_depth, mcw, gamma, fixed, threads=1, lam=1.0, eta=0.3):
    """(feature, split_bin, default_left, left, right, value, leaf_of_row) from mifx_gbdt_grow[_fixed]."""
    lib = xgb._lib()
    f, n = bins.shape
    cap = 2 ** (max_depth + 1)
    fe, sb, le, ri = (np.empty(cap, np.int32) for _ in range(4))
    dl, val, leaf = np.empty(cap, np.uint8), np.empty(cap, np.float64), np.empty(n, np.int32)
    fn = lib.mifx_gbdt_grow_fixed if fixed else lib.mifx_gbdt_grow
    p = xgb._p
    cnt = fn(p(bins, xgb._U16), n, f, p(nbins, xgb._I), p(g, xgb._F), p(h, xgb._F), max_depth, float(mcw), float(lam),
             float(gamma), float(eta), threads, cap, p(fe, xgb._I), p(sb, xgb._I), p(dl, xgb._U8), p(le, xgb._I),
             p(ri, xgb._I), p(val, xgb._D), p(leaf, xgb._I))
    assert cnt > 0
    return fe[:cnt].copy(), sb[:cnt].copy(), dl[:cnt].copy(), le[:cnt].copy(), ri[:cnt].copy(), val[:cnt].copy(), leaf


NAMES = ("feature", "split_bin", "default_left", "left", "right", "value", "leaf_of_row")


def assert_same_tree(a, b, what=""):
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), f"{what}: {name} differs"


def quant_exp_ref(amax, n):
    if not (amax > 0.0) or not np.isfinite(amax):
        return 0
    return 60 - int(n).bit_length() - int(np.frexp(amax)[1])  # frexp's exponent is ilogb(amax) + 1
