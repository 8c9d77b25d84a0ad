"""HIP analyzer kernels (csrc/analyzers.hip: column moments, bucketize, sliced-metric histograms, histograms) against
exact or extended-precision references, on every table regime and branch of the kernels.

References. np.searchsorted / np.histogram / np.unique are used as they are. The two that are not plain numpy are
pinned by unmarked CPU tests first: the host segment_hist against a per-row Python loop
(test_host_segment_hist_matches_row_loop), and the moments tolerance against a float64 transcription of the kernel's
own combine order (test_chan_transcription_error_bounds). The CPU Transform's NaN semantics, which the GPU Transform
path must reproduce, are pinned by test_cpu_transform_nan_semantics.

Which kernel path a case reaches:
  segment_hist_k   nbins = ns * nb * 2 <= 32768 -> LDS table (zero-fill, ds atomics, flush); above -> global atomics.
                   (1, 1000) 8 KB LDS; (1, 10000) 80 KB LDS, needs the > 64 KB hipFuncSetAttribute, the Evaluator's
                   own shape; (16, 1024) exactly 32768 bins = 128 KB, the last LDS size; (2, 10000) 40000 bins, the
                   first global-atomic size; (24, 1000) 48000 bins. n = 50000 is 196 blocks, n = 100 fewer rows than
                   one block's threads.
  bucketize_k      nb = 0 (no search trip), 1, 9, 255 (one staging trip, partial), 256 (exactly one), 1024 (four trips,
                   the kernel's limit); nb = 1025 is the wrapper's host fallback. n = 1, 255 (< one block), 300001
                   (1172 blocks, the last partial).
  col_moments_p1/2 n = 1, 63 (< one wave), 64 (one wave), 257 (two blocks); 262144 = 1024 blocks x 256 threads is the
                   grid cap: at 262143 the last thread is empty, at 262145 thread 0 takes a second grid-stride trip.
  hist_k mode 0    nb = 255 / 256 (edge staging loop `i <= nb`: one trip / a second trip for the last edge), 4096 (the
                   limit, 17 trips); 4097 is the host fallback.
  hist_k mode 1    int_value_counts over a range of 16384 (the last LDS size, 64 KB) and 16385 (global atomics)."""
import functools
import math

import numpy as np
import pytest

from mifx.ops import analyzers as an

gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------- segment_hist
SEG_CASES = [(1, 1000), (1, 10000), (16, 1024), (2, 10000), (24, 1000)]


def _seg_id(c):
    ns, nb = c
    return f"ns{ns}-nb{nb}-" + ("lds" if ns * nb * 2 <= 32768 else "global")


@functools.lru_cache(maxsize=None)
def _seg_case(n, ns, nb):
    """Inputs + the host result (computed once per case, the result read-only). Segment ids in [-1, ns] (both ends
    ignored), segment ns // 2 left empty when ns > 1; labels {0, 1} and a few 0.5 (negative); float32 probabilities
    in [-0.1, 1.1] plus 0, 1, 0.5, 1e-7 and float32(k / nb) for a handful of k, each with both labels."""
    r = np.random.default_rng(1000 * ns + nb + n)
    seg = r.integers(-1, ns + 1, n).astype(np.int32)
    if ns > 1:
        seg[seg == ns // 2] = -1
    y = (r.random(n) < 0.3).astype(np.float32)
    y[::53] = 0.5
    p = (r.random(n) * 1.2 - 0.1).astype(np.float32)
    ks = [0, 1, 2, 7, nb // 3, nb // 2, nb - 1, nb]
    special = np.array([0.0, 1.0, 0.5, 1e-7] + [k / nb for k in ks], dtype=np.float32)
    special = np.concatenate([special, special])
    m = special.size
    p[:m] = special
    y[:m] = np.repeat([0.0, 1.0], m // 2)
    seg[:m] = 0
    seg[m], seg[m + 1] = -1, ns
    sums, hist = an.segment_hist(seg, y, p, ns, nb, device=None)
    for a in (sums, hist):
        a.setflags(write=False)
    return seg, y, p, sums, hist


def _segment_hist_loop(seg, y, p, ns, nb):
    """One row at a time, the definition: float32 clip to [1e-7, 1 - 1e-7], bucket = floor of the fp64 product of
    the float32 probability with nb (the last bucket closed), label positive iff > 0.5, sums with math.fsum."""
    lo, hi = np.float32(1e-7), np.float32(1 - 1e-7)
    hist = np.zeros((ns, nb, 2), np.int64)
    cols = [[[] for _ in range(5)] for _ in range(ns)]
    for s, yi, pi in zip(seg.tolist(), y, p):
        if not 0 <= s < ns:
            continue
        pf = min(max(np.float32(pi), lo), hi)
        assert pf.dtype == np.float32
        pd, yd = float(pf), float(yi)
        b = min(int(pd * nb), nb - 1)
        hist[s, b, 1 if yd > 0.5 else 0] += 1
        loss = -(yd * math.log(pd) + (1.0 - yd) * math.log(1.0 - pd))
        for j, v in enumerate((1.0, yd, pd, loss, float((pd > 0.5) == (yd > 0.5)))):
            cols[s][j].append(v)
    return np.array([[math.fsum(c) for c in row] for row in cols]), hist


@pytest.mark.parametrize("ns,nb", [(1, 1000), (3, 10), (2, 10000)])
def test_host_segment_hist_matches_row_loop(ns, nb):
    """The GPU tests' reference, segment_hist(device=None), against the per-row definition on 200 rows. The upper
    clip bound is the float32 nearest to 1 - 1e-7, which is also what the kernel's `1.f - 1e-7f` evaluates to."""
    assert np.float32(1 - 1e-7) == np.float32(1) - np.float32(1e-7)
    seg, y, p, sums, hist = _seg_case(200, ns, nb)
    want_sums, want_hist = _segment_hist_loop(seg, y, p, ns, nb)
    assert np.array_equal(hist, want_hist)
    assert np.array_equal(sums[:, [0, 1, 4]], want_sums[:, [0, 1, 4]])
    np.testing.assert_allclose(sums[:, 2:4], want_sums[:, 2:4], rtol=1e-13, atol=0)
    inr = (seg >= 0) & (seg < ns)
    assert hist.sum() == inr.sum() == sums[:, 0].sum()
    assert sums[0, 0] >= 24  # the special probabilities all sit in segment 0


@gpu
@pytest.mark.parametrize("n", [50_000, 100])
@pytest.mark.parametrize("ns,nb", SEG_CASES, ids=[_seg_id(c) for c in SEG_CASES])
def test_segment_hist_every_table_regime(ns, nb, n):
    """segment_hist_k on the LDS path (including the 80 KB and 128 KB tables behind hipFuncSetAttribute) and the
    global-atomic path; see the module docstring for which (ns, nb) is which. Counts are exact. sums[:, 2:4]
    (prediction and loss sums) are fp64 atomics applied in arbitrary order, so they keep rtol = 1e-9: that order is
    non-deterministic by design and not pinned here."""
    seg, y, p, ref_sums, ref_hist = _seg_case(n, ns, nb)
    sums, hist = an.segment_hist(seg, y, p, ns, nb, device="cuda")
    inr = (seg >= 0) & (seg < ns)
    assert hist.shape == (ns, nb, 2) and hist.dtype == np.int64
    assert np.array_equal(hist, ref_hist)
    assert hist.sum() == inr.sum()
    assert np.array_equal(sums[:, 0], ref_sums[:, 0])
    assert np.array_equal(sums[:, 4], ref_sums[:, 4])
    label_sum = np.zeros(ns)
    np.add.at(label_sum, seg[inr], y[inr].astype(np.float64))  # dyadic labels: exact in any order
    assert np.array_equal(sums[:, 1], label_sum)
    np.testing.assert_allclose(sums[:, 2:4], ref_sums[:, 2:4], rtol=1e-9, atol=0)
    if ns > 1:
        assert not sums[ns // 2].any() and not hist[ns // 2].any()  # the empty segment stays empty


@gpu
def test_segment_hist_matches_numpy():
    r = np.random.default_rng(2)
    n, ns = 200_000, 24
    seg = r.integers(0, ns, n)
    y = (r.random(n) < 0.3).astype(np.float32)
    p = np.clip(r.random(n) * 0.6 + y * 0.3, 0, 1).astype(np.float32)
    s_g, h_g = an.segment_hist(seg, y, p, ns, 1000, device="cuda")
    s_c, h_c = an.segment_hist(seg, y, p, ns, 1000, device=None)
    assert np.array_equal(h_g, h_c)
    assert np.allclose(s_g, s_c, rtol=1e-9)
    auc = an.auc_from_hist(h_c[0])
    assert 0.5 < auc < 1.0


# ---------------------------------------------------------------------------------------------------- bucketize
def _bucketize_case(nb, n):
    """Sorted boundaries with a duplicated pair and a 0.0; values = NaN, +-inf, -0.0, 0.0, then (as far as n allows)
    every boundary and its two neighbouring doubles, then N(0, 1.5)."""
    r = np.random.default_rng(100 * nb + n % 97)
    b = np.sort(r.normal(size=nb))
    if nb:
        b[nb // 2] = 0.0
    if nb >= 4:
        b[nb // 4] = b[nb // 4 + 1]
    b = np.sort(b)
    edge = np.concatenate([b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf)])
    pool = np.concatenate([[np.nan, np.inf, -np.inf, -0.0, 0.0], r.permutation(edge)])
    x = r.normal(0, 1.5, n)
    k = min(n, pool.size)
    x[:k] = pool[:k]
    return x, b


def test_searchsorted_reference_sends_nan_to_nb():
    """The reference's own convention (TF Bucketize's upper_bound agrees): NaN sorts after every boundary."""
    assert np.searchsorted([1.0, 2.0, 3.0], np.nan, "right") == 3
    x, b = _bucketize_case(9, 255)
    assert np.isnan(x[0]) and np.searchsorted(b, x, "right")[0] == 9
    at_zero = int((b <= 0.0).sum())  # -0.0 compares equal to the 0.0 boundary: the upper bucket, like +0.0
    assert np.signbit(x[3]) and 0.0 in b and np.searchsorted(b, x[3:5], "right").tolist() == [at_zero, at_zero]


@gpu
@pytest.mark.parametrize("n", [1, 255, 300_001])
@pytest.mark.parametrize("nb", [0, 1, 9, 255, 256, 1024, 1025])
def test_bucketize_boundaries_limits_nonfinite(nb, n):
    """bucketize_k for every boundary count that changes its staging loop or search depth (module docstring), with
    duplicate boundaries, values on and one ulp either side of every boundary, -0.0 against a 0.0 boundary, +-inf
    and NaN. NaN goes to nb like np.searchsorted(side="right") and tf Bucketize; a `b[mid] <= v` comparison sent it
    to bucket 0. n = 1 is the NaN alone. nb = 1025 goes through the wrapper's host fallback."""
    x, b = _bucketize_case(nb, n)
    got = an.bucketize(x, b, device="cuda")
    assert got.dtype == np.int64
    assert np.array_equal(got, np.searchsorted(b, x, "right"))
    assert got[0] == nb  # the NaN


@gpu
def test_bucketize_matches_searchsorted():
    r = np.random.default_rng(1)
    x = r.normal(size=300_001)
    b = np.quantile(x, np.arange(1, 10) / 10)
    x[:10] = b[:10 - 1].tolist() + [b[-1]]  # exact boundary hits go to the upper bucket
    assert np.array_equal(an.bucketize(x, b, device="cuda"), np.searchsorted(b, x, side="right"))


def _nan_column(n=5000):
    r = np.random.default_rng(8)
    x = r.normal(41.9, 0.05, n)
    x[[0, n - 1]] = np.nan
    x[r.integers(0, n, 40)] = np.nan
    return x


def _same_entries(a, b):
    np.testing.assert_equal(a, b)  # NaN == NaN, everything else exact


def _bucket_fn(inputs):
    import mifx.transform as mt

    return {"fixed": mt.apply_buckets(inputs["x"], [41.85, 41.9, 41.95]), "quant": mt.bucketize(inputs["x"], 10)}


def _zscore_fn(inputs):
    import mifx.transform as mt

    return {"z": mt.scale_to_z_score(inputs["x"])}


def test_cpu_transform_nan_semantics():
    """What the one-process CPU Transform does with missing values, which the GPU path has to reproduce: a NaN lands
    in the last bucket (nb), and any NaN poisons mean / var / min / max while count still includes it -- the same as
    mifx.transform.parallel's merge of per-shard accumulators."""
    import mifx.transform as mt
    from mifx.transform import parallel

    x = _nan_column()
    out, st = mt.analyze(_bucket_fn, {"x": x}, device=None)
    nanrows = np.isnan(x)
    assert (out["fixed"][nanrows] == 3).all() and (out["quant"][nanrows] == 9).all()
    assert (out["quant"][~nanrows] <= 9).all() and out["quant"].max() == 9
    out, st = mt.analyze(_zscore_fn, {"x": x}, device=None)
    e = st.entries[0]["values"]
    assert all(math.isnan(e[k]) for k in ("mean", "var", "min", "max")) and e["count"] == x.size
    assert np.isnan(out["z"]).all()
    merged = parallel._moments_merge([parallel._moments_acc(x[:2000]), parallel._moments_acc(x[2000:])])
    _same_entries(merged, e)


@gpu
def test_transform_buckets_with_nan_equal_host(monkeypatch):
    """apply_buckets and bucketize inside analyze() on a NaN-bearing column: the device path (bucketize_k + the
    histogram-narrowed quantiles) gives the output and state of the host path -- missing values in bucket nb on both,
    or a Transform analysed on the GPU and replayed on few rows on the CPU would skew."""
    import mifx.transform as mt
    import mifx.transform.api as tapi

    x = _nan_column()
    monkeypatch.setattr(tapi, "GPU_MIN_ROWS", 0)
    out_g, st_g = mt.analyze(_bucket_fn, {"x": x}, device="cuda")
    out_c, st_c = mt.analyze(_bucket_fn, {"x": x}, device=None)
    for k in ("fixed", "quant"):
        assert np.array_equal(out_g[k], out_c[k]), k
    assert (out_g["fixed"][np.isnan(x)] == 3).all()
    _same_entries(st_g.entries, st_c.entries)


@gpu
def test_transform_moments_with_nan_equal_host(monkeypatch):
    """scale_to_z_score inside analyze() on a NaN-bearing column: column_moments skips NaNs (TFDV statistics want
    that), the Transform's moments do not -- the device branch must return the poisoned entry of the host branch."""
    import mifx.transform as mt
    import mifx.transform.api as tapi

    x = _nan_column()
    monkeypatch.setattr(tapi, "GPU_MIN_ROWS", 0)
    out_g, st_g = mt.analyze(_zscore_fn, {"x": x}, device="cuda")
    out_c, st_c = mt.analyze(_zscore_fn, {"x": x}, device=None)
    _same_entries(st_g.entries, st_c.entries)
    e = st_g.entries[0]["values"]
    assert all(math.isnan(e[k]) for k in ("mean", "var", "min", "max"))
    assert e["count"] == x.size
    np.testing.assert_equal(out_g["z"], out_c["z"])
    # without NaNs the device branch still is the kernel's result, not the poisoned one
    out_g, st_g = mt.analyze(_zscore_fn, {"x": np.nan_to_num(x, nan=41.9)}, device="cuda")
    assert np.isfinite(out_g["z"]).all() and st_g.entries[0]["values"]["count"] == x.size


# ----------------------------------------------------------------------------------------------- column moments
ZERO = {"count": 0, "mean": 0.0, "std": 0.0, "min": 0.0, "max": 0.0, "zeros": 0}
KEYS = ("count", "mean", "std", "min", "max", "zeros")


def _ld_moments(x):
    """Two-pass mean and population std in np.longdouble (64-bit significand on x86), NaNs skipped."""
    v = np.asarray(x, np.float64)
    v = v[~np.isnan(v)].astype(np.longdouble)
    mean = v.sum() / v.size
    return mean, np.sqrt(((v - mean) ** 2).sum() / v.size)


def _rel(got, want):
    err = abs(np.longdouble(got) - want)
    return float(err / abs(want)) if want != 0 else float(err)


def _chan(a, b):
    """combine() of csrc/analyzers.hip on arrays of (n, mean, m2)."""
    (an_, am, a2), (bn, bm, b2) = a, b
    n = an_ + bn
    with np.errstate(invalid="ignore", divide="ignore"):
        d = bm - am
        mean = am + d * (bn / n)
        m2 = a2 + b2 + d * d * (an_ * bn / n)
    ea, eb = an_ == 0, bn == 0
    return tuple(np.where(ea, q, np.where(eb, p, r)) for p, q, r in ((an_, bn, n), (am, bm, mean), (a2, b2, m2)))


def _block_reduce(m):
    """block_reduce() on arrays shaped [..., 256]: the shuffle-down tree within each wave of 64 (lane 0's operands
    only), then thread 0's left-to-right combine of the four wave results."""
    m = tuple(v.reshape(v.shape[:-1] + (4, 64)) for v in m)
    o = 32
    while o:
        m = _chan(tuple(v[..., :o] for v in m), tuple(v[..., o:2 * o] for v in m))
        o >>= 1
    r = tuple(v[..., 0, 0] for v in m)
    for w in range(1, 4):
        r = _chan(r, tuple(v[..., w, 0] for v in m))
    return r


def _chan_transcription(x):
    """float64 numpy transcription of col_moments_p1 + col_moments_p2 (same grid, same per-thread grid-stride
    order, same trees; numpy neither contracts to FMA nor reorders) -> (mean, population std)."""
    x = np.asarray(x, np.float64)
    grid = max(1, min(1024, (x.size + 255) // 256))
    t = grid * 256
    pad = np.full(-(-x.size // t) * t, np.nan)
    pad[:x.size] = x
    m = tuple(np.zeros(t) for _ in range(3))
    for row in pad.reshape(-1, t):  # every thread's k-th grid-stride element
        ok = ~np.isnan(row)
        one = (ok.astype(np.float64), np.where(ok, row, 0.0), np.zeros(t))
        m = _chan(m, one)
    part = _block_reduce(tuple(v.reshape(grid, 256) for v in m))  # [grid]
    npad = -(-grid // 256) * 256
    acc = tuple(np.zeros(256) for _ in range(3))
    for k in range(npad // 256):  # p2: thread i combines partial[i], partial[i + 256], ...
        nxt = tuple(np.concatenate([v, np.zeros(npad - grid)])[k * 256:(k + 1) * 256] for v in part)
        acc = _chan(acc, nxt)
    n, mean, m2 = _block_reduce(acc)
    return float(mean), float(np.sqrt(m2 / n))


@functools.lru_cache(maxsize=None)
def _cond_case(name):
    r = np.random.default_rng(42)
    x = {"well": lambda: r.normal(3.0, 2.0, 1_000_003),
         "1e9": lambda: 1e9 + r.normal(0.0, 1.0, 1_000_003),
         "1e6": lambda: 1e6 + r.normal(0.0, 1e-3, 300_001)}[name]()
    return x, _ld_moments(x)


# bounds on |got - longdouble| / |longdouble| for (mean, std). "well": fp64 Chan on N(3, 2) is good to a few ulp.
# The ill-conditioned ones lose log10(mean / std) = 9 digits of every delta to the rounding of the running mean;
# 1e-9 on std / 1e-15 on mean is 3.5 to 10 x what the transcription below shows, the slack covering the device's
# FMA contraction and division rounding.
COND_BOUNDS = {"well": (1e-13, 1e-13), "1e9": (1e-15, 1e-9), "1e6": (1e-15, 1e-9)}


@pytest.mark.parametrize("name", list(COND_BOUNDS))
def test_chan_transcription_error_bounds(name):
    """Where the moments tolerances come from: the kernel's combine order transcribed to float64 numpy, measured
    against the two-pass longdouble reference. Relative errors (mean / std) of the transcription on these inputs:
    well 2.1e-17 / 1.7e-16, 1e9 4.1e-17 / 2.8e-10, 1e6 5.0e-17 / 1.0e-10 (run with -s to print them again). The
    ill-conditioned std error is what theory gives: each delta carries the running mean's rounding, ulp(mean) / std
    relative, and n of them average to about 2 ulp(mean) / (std sqrt(n)) = 2.4e-10 and 4.2e-10."""
    x, (mean, std) = _cond_case(name)
    got_mean, got_std = _chan_transcription(x)
    em, es = _rel(got_mean, mean), _rel(got_std, std)
    print(f"transcription {name}: mean rel {em:.2e} std rel {es:.2e}")
    bm, bs = COND_BOUNDS[name]
    assert em <= bm and es <= bs


def test_chan_transcription_small_and_nan():
    r = np.random.default_rng(3)
    for n in (1, 63, 64, 257, 70_000):
        x = r.normal(3.0, 2.0, n)
        if n > 2:
            x[[0, -1]] = np.nan
        v = x[~np.isnan(x)]
        mean, std = _chan_transcription(x)
        assert mean == pytest.approx(v.mean(), rel=1e-14) and std == pytest.approx(v.std(), rel=1e-13, abs=0)


@gpu
@pytest.mark.parametrize("name", list(COND_BOUNDS))
def test_column_moments_conditioning(name):
    """column_moments against the two-pass longdouble reference: N(3, 2) x 1,000,003; 1e9 + N(0, 1) x 1,000,003;
    1e6 + N(0, 1e-3) x 300,001 (bounds: COND_BOUNDS). Run twice: the six outputs must be bit-equal, the kernel
    combines in a fixed order. Measured on an MI355X, relative error of mean / std: well 2.1e-17 / 1.7e-16,
    1e9 4.1e-17 / 2.8e-10, 1e6 5.0e-17 / 1.0e-10 -- the same figures as the CPU transcription of the combine order,
    3.5 x and 10 x inside the std bound."""
    x, (mean, std) = _cond_case(name)
    got = an.column_moments(x, device="cuda")
    again = an.column_moments(x, device="cuda")
    em, es = _rel(got["mean"], mean), _rel(got["std"], std)
    print(f"gpu {name}: mean rel {em:.2e} std rel {es:.2e}")
    assert got["count"] == x.size and got["zeros"] == 0
    assert got["min"] == x.min() and got["max"] == x.max()
    assert [got[k] for k in KEYS] == [again[k] for k in KEYS]
    bm, bs = COND_BOUNDS[name]
    assert em <= bm and es <= bs


@gpu
@pytest.mark.parametrize("edge_nan", [False, True], ids=["", "nan-first-last"])
@pytest.mark.parametrize("n", [1, 63, 64, 257, 262_143, 262_144, 262_145])
def test_column_moments_sizes(n, edge_nan):
    """n below one wave, one wave, two blocks, and either side of the 1024 x 256 grid cap (module docstring), with
    zeros sprinkled in and optionally NaN at the first and last position (for n <= 2 that is the all-NaN column).
    count / zeros / min / max exact; mean and std to the well-conditioned bound against longdouble."""
    r = np.random.default_rng(n)
    x = r.normal(3.0, 2.0, n)
    x[::7] = 0.0
    if edge_nan:
        x[[0, -1]] = np.nan
    got = an.column_moments(x, device="cuda")
    v = x[~np.isnan(x)]
    if v.size == 0:
        assert got == ZERO
        return
    mean, std = _ld_moments(x)
    assert got["count"] == v.size and got["zeros"] == (v == 0).sum()
    assert got["min"] == v.min() and got["max"] == v.max()
    assert _rel(got["mean"], mean) <= 1e-13
    if v.size == 1:
        assert got["std"] == 0.0
    else:
        assert _rel(got["std"], std) <= 1e-13
    assert got == an.column_moments(x, device="cuda")


@gpu
@pytest.mark.parametrize("n", [1, 300, 262_145])
def test_column_moments_all_nan_is_zero_dict(n):
    got = an.column_moments(np.full(n, np.nan), device="cuda")
    assert got == ZERO and got == an.column_moments(np.full(n, np.nan), device=None)


@gpu
@pytest.mark.parametrize("n", [1, 64, 100_001, 262_145])
def test_column_moments_constant_column(n):
    """A constant 0.1: Chan's update never sees a non-zero delta, on any thread or tree level, so std is exactly 0
    and mean is exactly the value -- nothing weaker is accepted."""
    got = an.column_moments(np.full(n, 0.1), device="cuda")
    assert got == {"count": n, "mean": 0.1, "std": 0.0, "min": 0.1, "max": 0.1, "zeros": 0}


@gpu
def test_column_moments_infinities():
    """+-inf pins count, zeros, min and max only: numpy's mean / std are inf / nan there and the combine order
    legitimately decides which."""
    r = np.random.default_rng(6)
    x = r.normal(size=5000)
    x[[3, 4000]] = np.inf
    x[77] = -np.inf
    x[[5, 6]] = 0.0
    x[9] = np.nan
    got = an.column_moments(x, device="cuda")
    assert (got["count"], got["zeros"], got["min"], got["max"]) == (4999, 2, -np.inf, np.inf)
    x[77] = 1.0
    got = an.column_moments(x, device="cuda")
    assert (got["count"], got["zeros"], got["min"], got["max"]) == (4999, 2, np.nanmin(x), np.inf)


@gpu
def test_column_moments_matches_numpy():
    r = np.random.default_rng(0)
    x = r.normal(3.0, 2.0, 1_000_003)
    x[::97] = np.nan
    x[::101] = 0.0
    got = an.column_moments(x, device="cuda")
    ref = an.column_moments(x, device=None)
    assert got["count"] == ref["count"] and got["zeros"] == ref["zeros"]
    for k in ("mean", "std", "min", "max"):
        assert got[k] == pytest.approx(ref[k], rel=1e-10, abs=1e-12), k


# --------------------------------------------------------------------------------------------------- histograms
def _edge_case(nb):
    r = np.random.default_rng(nb)
    e = np.cumsum(r.random(nb + 1) + 0.01) - 50.0
    out = [e[0] - 1.0, e[-1] + 1.0, np.nextafter(e[0], -np.inf), np.nextafter(e[-1], np.inf), np.inf, -np.inf, np.nan]
    x = np.concatenate([e, r.choice(e, 20_000), out, out])  # every value sits on an edge, or is dropped
    return r.permutation(x), e


def test_numpy_histogram_drops_outside_and_closes_last_bin():
    x, e = _edge_case(255)
    h = np.histogram(x[~np.isnan(x)], bins=e)[0]
    assert h.sum() == 255 + 1 + 20_000 and h[-1] >= 2  # both e[-2] and e[-1] land in the last bin
    assert np.array_equal(h, an.histogram(x, e, device=None))


@gpu
@pytest.mark.parametrize("nb", [255, 256, 4096, 4097])
def test_histogram_values_on_every_edge(nb):
    """hist_k mode 0 with every value on an edge (the upper bin takes it, the last bin is closed), values outside
    [e0, e_nb] by one ulp and by far, +-inf and NaN dropped. nb = 255 / 256 / 4096: one, two and 17 trips of the
    edge staging loop; 4097 is the wrapper's host fallback."""
    x, e = _edge_case(nb)
    got = an.histogram(x, e, device="cuda")
    assert got.dtype == np.int64 and np.array_equal(got, np.histogram(x[~np.isnan(x)], bins=e)[0])


@gpu
@pytest.mark.parametrize("span", [16_384, 16_385], ids=["16384-lds", "16385-global"])
def test_int_value_counts_at_the_lds_limit(span):
    """hist_k mode 1 with nb = span unit bins: 16384 is the last LDS-privatised size, 16385 the first that counts
    with global atomics. Both ends of the range occur, so the range is exactly span."""
    r = np.random.default_rng(span)
    ints = r.integers(-5000, -5000 + span, 50_000)
    ints[:2] = [-5000, -5000 + span - 1]
    u, c = an.int_value_counts(ints, device="cuda")
    uu, cc = np.unique(ints, return_counts=True)
    assert np.array_equal(u, uu) and np.array_equal(c, cc)
