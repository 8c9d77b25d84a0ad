"""Shared by test_gbdt_quantile_cpu.py and test_gbdt_quantile_gpu.py: the leaf-refresh cases and their reference, a
plain numpy / Python-int function that uses none of the code under test."""
import math

import numpy as np

ETA = 0.3


def reference_refresh(resid, h, leaf, value, alpha, eta=ETA):
    """value with every leaf of positive integer weight set to eta * (weighted lower alpha-quantile of its rows'
    residuals): sort the leaf's residuals (-0.0 before +0.0), accumulate the integer weights, take the first residual
    at which they reach T = ceil(alpha * float(Q)) clamped to [1, Q]."""
    out, rows = value.copy(), np.flatnonzero(leaf >= 0)
    amax = float(np.abs(h[rows]).max()) if len(rows) else 0.0
    e = 60 - len(rows).bit_length() - math.frexp(amax)[1] if amax > 0 else 0
    for lf in np.unique(leaf[rows]):
        idx = sorted(np.flatnonzero(leaf == lf), key=lambda i: (resid[i], not np.signbit(resid[i])))
        q = [round(math.ldexp(float(h[i]), e)) for i in idx]  # round half even, as llrint
        total = sum(q)
        if total == 0:
            continue
        t, run = min(max(math.ceil(alpha * float(total)), 1), total), 0
        for i, qi in zip(idx, q):
            run += qi
            if run >= t:
                out[lf] = eta * resid[i]
                break
    return out


def _case(resid, leaf, nodes, h=None, alpha=0.5, rows_per_wg=None):
    resid = np.ascontiguousarray(resid, np.float64)
    h = np.ones(len(resid), np.float32) if h is None else np.ascontiguousarray(h, np.float32)
    value = 7.0 + np.arange(nodes, dtype=np.float64)  # what a leaf without weight must keep
    return resid, h, np.ascontiguousarray(leaf, np.int32), value, alpha, rows_per_wg


def _low_byte(rng, n):
    """n doubles that differ in their lowest byte only (and are mostly distinct)"""
    return (np.float64(1.2345).view(np.int64) & ~0xFF | rng.integers(0, 256, n)).view(np.float64)


def cases():
    rng = np.random.default_rng(7)
    big, hbig = rng.normal(size=5000), rng.uniform(0.5, 1.5, 5000)
    leaf3 = rng.integers(1, 4, 5000)
    deep = rng.integers(256, 511, 4000)                              # 255 leaves of a depth-8 tree
    lg = rng.permutation(127)[:64][rng.integers(0, 64, 3000)]        # 64 scattered leaf ids of a leaf-wise tree
    wide = rng.normal(size=3000).astype(np.float32).astype(np.float64)
    c = {
        "rows_1_2_3": _case([3.0, -1.0, 2.0, 5.0, 4.0, -6.0], [1, 2, 2, 3, 3, 3], 4),
        "all_equal": _case([2.5] * 5 + [1.0, 9.0], [1] * 5 + [2, 2], 3),
        "ties_at_rank": _case([1.0, 2.0, 2.0, 2.0, 3.0, 2.0, 0.5, 2.0], [0] * 8, 1),
        "signed_zeros": _case([0.0, -0.0, -1.5, 0.0, -0.0, 2.0, -0.0, 1e-300, -1e-300], [1, 1, 1, 1, 1, 1, 2, 2, 2], 3,
                              alpha=0.4),
        "zero_weights": _case(rng.normal(size=40), [1] * 20 + [2] * 10 + [3] * 10, 4,
                              h=np.r_[rng.integers(0, 2, 20), np.zeros(10), np.ones(10)]),  # leaf 2: Q = 0
        "weights_2^20": _case(rng.normal(size=300), rng.integers(0, 3, 300), 3, h=np.ldexp(1.0, -rng.integers(0, 21, 300))),
        "unsampled": _case(rng.normal(size=500), rng.integers(-1, 3, 500), 3, h=rng.uniform(0.1, 2.0, 500)),
        "float32_wide": _case(wide, rng.integers(1, 3, 3000), 3),
        "low_byte_only": _case(_low_byte(rng, 2000), rng.integers(1, 3, 2000), 3),
        "chunked": _case(big, leaf3, 4, h=hbig, rows_per_wg=512),
        "chunked_float32": _case(wide, rng.integers(1, 3, 3000), 3, alpha=0.25, rows_per_wg=512),
        "chunked_low_byte":_case(_low_byte(rng, 5000), leaf3, 4, rows_per_wg=512),
        "default_chunks": _case(big, leaf3, 4, h=hbig),                # the same data: the same bits
        "one_large_leaf": _case(big, np.zeros(5000), 1, h=hbig, alpha=0.9),  # more rows than LDS holds, one chunk
        "depth8_255": _case(rng.normal(size=4000), deep, 511),
        "lossguide_64": _case(rng.normal(size=3000), lg, 127, h=rng.uniform(0.0, 1.0, 3000)),
    }
    for a in (0.01, 0.5, 0.99):  # T clamps to 1 and reaches Q in the small leaves
        c[f"alpha_{a}"] = _case(rng.normal(size=200), np.r_[[1, 2, 2], rng.integers(3, 6, 197)], 6, alpha=a)
    return c


CASES = cases()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)
