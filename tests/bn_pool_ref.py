"""Plain fp64 / exact references, derived error bounds and shared input grids for the BatchNorm+ReLU kernels
(csrc/bn_relu.hip) and the 3x3/2 max pool (csrc/pool.hip). Everything here runs in torch on the CPU in float64 and
makes no GPU call; tests/test_bn_pool_ref.py checks these references against PyTorch's own operators.

Error model (every tolerance used by test_bn_relu_exact.py is one of these formulas, none is a tuned number):

  U32 = 2^-24 is the unit roundoff of fp32: one fp32 operation returns its exact result v with an error <= U32 |v|.

  half_ulp(v, T): half the spacing of type T at |v|, 2^(floor(log2 |v|) - p) with p = 24 significand bits for fp32 and
  8 for bf16 -- the error of one round-to-nearest store of v as T. (Between 2^-(p+1) |v| and 2^-p |v|; the upper end
  is reached just above a power of two, so the exact spacing is used, not a fraction of |v|.)

  store_tol(ref, E, T): a value within E of ref, then stored as T. fp32 results are already fp32 values, so their
  store is exact: E. bf16: E + half_ulp(|ref| + E, bf16).

  sum_tol(k, pre, S): a per-channel sum whose terms have absolute sum S, accumulated in fp32 along a chain of k
  additions, each term produced by `pre` fp32 operations: 2 (k + pre) U32 S. A chain of k additions is off by at most
  k U32 S to first order, every operation on a term by one more U32 |term|; the factor 2 is the margin for the
  second-order terms. chain(M, C, nb) gives k for the direct passes: rows per thread of the largest block + row
  slices per block (the two fp32 chains of bn_stats / bn_bwd_reduce) + 2 for the finalize (its fp64 combine, and the
  fp32 store of the combined sum).

  fp64 work in the kernels (combines, Chan merges) is bounded by C64(n) = 8 n 2^-53 relative to the magnitudes
  merged: n merges of at most 8 operations each.
"""
from __future__ import annotations

import torch

U32 = 2.0 ** -24
U64 = 2.0 ** -53
_SIG = {torch.float32: 24, torch.bfloat16: 8}
F64 = torch.float64


def f32(v: float) -> float:
    """The fp32 value a Python float becomes when passed to a kernel as `float`."""
    return float(torch.tensor(v, dtype=torch.float32))


def half_ulp(v: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    a = v.abs().to(F64)
    _, e = torch.frexp(a)  # a = m 2^e with m in [0.5, 1): floor(log2 a) = e - 1
    hu = torch.ldexp(torch.ones_like(a), e - 1 - _SIG[dtype])
    return torch.where(a > 0, hu, torch.zeros_like(a))


def store_tol(ref: torch.Tensor, E: torch.Tensor, dtype) -> torch.Tensor:
    if dtype == torch.float32:
        return E
    return E + half_ulp(ref.abs() + E, dtype)


def sum_tol(k: int, pre: int, abs_sum: torch.Tensor) -> torch.Tensor:
    return 2.0 * (k + pre) * U32 * abs_sum


def c64(n: int) -> float:
    return 8.0 * n * U64


def chain(M: int, C: int, nb: int) -> int:
    """k of sum_tol for bn_stats / bn_bwd_reduce over [M, C] in nb blocks (see the module docstring)."""
    rpb = 256 // (C // 8)  # row slices per block
    rows = -(-M // nb)  # rows of the largest block (block_rows splits M evenly, up to one row)
    rpt = -(-rows // rpb)  # rows per thread
    return rpt + rpb + 2


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU: fp64 truth
# ---------------------------------------------------------------------------------------------------------------
def bn_ref(x, w, b, eps, relu=True, dy=None, dres=None) -> dict:
    """Training BatchNorm (+ ReLU) of x [M, C] (already rounded to its storage type) and its backward, all in fp64.
    M = 1 is allowed: unbiased variance := biased variance there, as the kernel defines it. eps is used as the fp32
    value the kernel receives."""
    x, w, b = x.to(F64), w.to(F64), b.to(F64)
    M = x.shape[0]
    eps = f32(eps)
    mean = x.mean(0)
    d = x - mean
    var = (d * d).mean(0)
    var_u = var * M / (M - 1) if M > 1 else var.clone()
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = w * rstd
    shift = b - mean * scale
    xhat = d * rstd
    t = xhat * w + b
    out = dict(mean=mean, var=var, var_unbiased=var_u, rstd=rstd, scale=scale, shift=shift,
               y=torch.clamp_min(t, 0.0) if relu else t)
    if dy is not None:
        g = dy.to(F64)
        if relu:
            g = torch.where(t > 0, g, torch.zeros_like(g))
        dbeta = g.sum(0)
        dgamma = (g * xhat).sum(0)
        dx = scale * (g - dbeta / M - xhat * dgamma / M)
        if dres is not None:
            dx = dx + dres.to(F64)
        out.update(dgamma=dgamma, dbeta=dbeta, dx=dx)
    return out


def running_ref(r0, v, momentum):
    m = f32(momentum)
    return (1.0 - m) * r0.to(F64) + m * v


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU: bounds of the per-channel outputs
# ---------------------------------------------------------------------------------------------------------------
def derived_bounds(ref: dict, E_mean, E_var, E_var_u, w, b, eps) -> dict:
    """Tolerances of the fp32 outputs [mean, rstd, scale, shift] and the unbiased variance, given that the kernel's
    fp64 mean / variances are within E_mean / E_var / E_var_u of ref's before they are stored:
      mean   : E_mean + half_ulp
      rstd   : 1 / sqrt(v + eps) is monotone, so the error is at most the distance to its value at v -+ E_var
               (v - E_var clamped at 0 like the kernel's variance), + half_ulp
      scale  : fp32 w * rstd: |w| tol_rstd + half_ulp
      shift  : fp32 b - mean * scale: the product is off by |mean| tol_scale + |scale| tol_mean + tol_mean tol_scale
               and rounded once (not at all if the compiler fuses it), the difference is rounded once."""
    w, b, eps = w.to(F64), b.to(F64), f32(eps)
    t = {}
    t["mean"] = E_mean + half_ulp(ref["mean"].abs() + E_mean)
    v = ref["var"]
    hi = 1.0 / torch.sqrt(torch.clamp_min(v - E_var, 0.0) + eps)
    lo = 1.0 / torch.sqrt(v + E_var + eps)
    E = torch.maximum(hi - ref["rstd"], ref["rstd"] - lo) + c64(1) * ref["rstd"]  # + the fp64 add, sqrt, divide
    t["rstd"] = E + half_ulp(ref["rstd"] + E)
    E = w.abs() * t["rstd"]
    t["scale"] = E + half_ulp(ref["scale"].abs() + E)
    Ep = ref["mean"].abs() * t["scale"] + ref["scale"].abs() * t["mean"] + t["mean"] * t["scale"]
    hp = half_ulp((ref["mean"] * ref["scale"]).abs() + Ep)
    t["shift"] = Ep + hp + half_ulp(ref["shift"].abs() + Ep + hp)
    t["var_unbiased"] = E_var_u + half_ulp(ref["var_unbiased"] + E_var_u)
    return t


def direct_stats_bounds(x, ref: dict, w, b, eps, k: int) -> dict:
    """bn_stats accumulates d = x - K (K = row 0; one fp32 subtraction: pre = 1) and d^2 (the error of d twice, the
    square once: pre = 3) in fp32; finalize forms mean = K + S/M and var = Q/M - (S/M)^2 in fp64. So
      E_mean = tol_S / M,   E_var = tol_Q / M + (2 |S/M| + E_mean) E_mean,   E_var_u = E_var M / (M - 1)."""
    x = x.to(F64)
    M = x.shape[0]
    d = x - x[0]
    tS = sum_tol(k, 1, d.abs().sum(0))
    tQ = sum_tol(k, 3, (d * d).sum(0))
    dm = d.sum(0) / M
    E_mean = tS / M
    E_var = tQ / M + (2.0 * dm.abs() + E_mean) * E_mean
    E_var_u = E_var * M / (M - 1) if M > 1 else E_var
    return derived_bounds(ref, E_mean, E_var, E_var_u, w, b, eps)


def running_tol(r0, v, tol_v, momentum):
    """run = (1 - m) * run + m * v in fp32, v already an fp32 value within tol_v of the truth: 1 - m, the two
    products and the sum are rounded once each (fewer if fused). (1 + U32)^2 covers roundings of rounded values."""
    m = f32(momentum)
    r0, v = r0.to(F64), v.to(F64)
    r = (1.0 - m) * r0 + m * v
    E = m * tol_v + (1.0 + U32) ** 2 * U32 * (2.0 * ((1.0 - m) * r0).abs() + (m * v).abs() + m * tol_v)
    return E + half_ulp(r.abs() + E)


# ---------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU: staged references from the kernel's own per-channel outputs
# ---------------------------------------------------------------------------------------------------------------
def preact(x, stats):
    """x * scale + shift in fp64 from the kernel's fp32 scale / shift. The product of two fp32 values is exact in
    fp64 and rounding never changes the sign of a nonzero sum, so `preact > 0` IS the kernel's ReLU mask."""
    return x.to(F64) * stats[2].to(F64) + stats[3].to(F64)


def stage_fwd(x, stats, relu, dtype):
    """(y_stage, tol): y = relu(fmaf(x, scale, shift)) is one fp32 rounding of the exact value (U32 |y|; relu of a
    value of the right sign adds none), U64 |y| for this reference's own fp64 sum, then the store."""
    t = preact(x, stats)
    y = torch.clamp_min(t, 0.0) if relu else t
    return y, store_tol(y, (U32 + U64) * y.abs(), dtype)


def masked_grad(x, dy, stats, relu):
    g = dy.to(F64)
    return torch.where(preact(x, stats) > 0, g, torch.zeros_like(g)) if relu else g


def stage_bwd_sums(x, dy, stats, relu, k: int):
    """(dbeta, dgamma, tol_dbeta, tol_dgamma) with the exact mask and the kernel's fp32 mean / rstd. dbeta sums g
    itself (pre = 0); dgamma sums g * ((x - mean) * rstd): three fp32 operations per term (pre = 3)."""
    g = masked_grad(x, dy, stats, relu)
    gx = g * ((x.to(F64) - stats[0].to(F64)) * stats[1].to(F64))
    return g.sum(0), gx.sum(0), sum_tol(k, 0, g.abs().sum(0)), sum_tol(k, 3, gx.abs().sum(0))


def stage_kbuf(M, w, stats, dgamma, dbeta):
    """(ref [3, C], tol [3, C]) of bn_finalize_bwd's coefficients A = w rstd, B = -A rstd q / M,
    Cc = -A s / M - B mean, from the kernel's fp32 dgamma = fl(q), dbeta = fl(s): q and s are known to half an ulp,
    the fp64 arithmetic to c64(1), and each coefficient is stored once as fp32."""
    w, mean, rstd = w.to(F64), stats[0].to(F64), stats[1].to(F64)
    q, s = dgamma.to(F64), dbeta.to(F64)
    A = w * rstd
    B = -A * rstd * (q / M)
    Cc = -A * (s / M) - B * mean
    EB = (A * rstd / M).abs() * half_ulp(q) + c64(1) * B.abs()
    EC = (A / M).abs() * half_ulp(s) + mean.abs() * EB + c64(1) * ((A * s / M).abs() + (B * mean).abs())
    tol = torch.stack([half_ulp(A), EB + half_ulp(B.abs() + EB), EC + half_ulp(Cc.abs() + EC)])
    return torch.stack([A, B, Cc]), tol


def stage_bwd(x, dy, stats, kbuf, relu, dres, dtype):
    """(dx_stage, tol): dx = fmaf(A, g, fmaf(B, x, Cc)) (+ dres), from the kernel's fp32 A, B, Cc. Each fused
    multiply-add and the dres addition round once, relative to the value they produce; (1 + U32)^2 covers roundings
    of rounded values, U64 per operation this reference's own fp64 arithmetic; then the store."""
    A, B, Cc = (kbuf[i].to(F64) for i in range(3))
    g = masked_grad(x, dy, stats, relu)
    inner = B * x.to(F64) + Cc
    outer = A * g + inner
    mags = inner.abs() + outer.abs()
    tot = outer
    if dres is not None:
        tot = outer + dres.to(F64)
        mags = mags + tot.abs()
    E = ((1.0 + U32) ** 2 * U32 + 2.0 * U64) * mags
    return tot, store_tol(tot, E, dtype)


# ---------------------------------------------------------------------------------------------------------------
# Tile statistics (the GEMM epilogues' per-tile partials)
# ---------------------------------------------------------------------------------------------------------------
def tile_parts(x, nt: int) -> torch.Tensor:
    """[2, T, C] fp32: each nt-row tile's column mean and sum of squared deviations, computed in fp64."""
    xt = x.to(F64).view(-1, nt, x.shape[1])
    mt = xt.mean(1)
    return torch.stack([mt, ((xt - mt[:, None]) ** 2).sum(1)]).float()


def tile_stats_bounds(part, nt: int, ref: dict, w, b, eps) -> dict:
    """The kernel merges the fp32 tile records in fp64, so against the fp64 truth of x only the fp32 rounding of the
    records (and of the outputs, derived_bounds) counts. With e_t = half_ulp(mean_t), the mean (1/T) sum mean_t is off
    by E_mean = mean(e_t); M2 = sum M2_t + nt sum (mean_t - mean)^2 by
      sum half_ulp(M2_t) + nt sum (2 |mean_t - mean| (e_t + E_mean) + (e_t + E_mean)^2);
    the fp64 merges (T records, 16 slices, <= 32 groups) add c64(T + 48) of the magnitudes merged."""
    mt, m2 = part[0].to(F64), part[1].to(F64)
    T = mt.shape[0]
    M = T * nt
    et = half_ulp(mt)
    slack = c64(T + 48)
    E_mean = et.mean(0) + slack * mt.abs().amax(0)
    dev = (mt - ref["mean"]).abs()
    ee = et + E_mean
    E_M2 = half_ulp(m2).sum(0) + nt * (2.0 * dev * ee + ee * ee).sum(0) + slack * (m2.sum(0) + nt * (dev * dev).sum(0))
    return derived_bounds(ref, E_mean, E_M2 / M, E_M2 / (M - 1) if M > 1 else E_M2 / M, w, b, eps)


def tile_bwd_parts(x, dy, stats, nt: int) -> torch.Tensor:
    """[2, T, C] fp32: per-tile sum g and sum g xhat (ReLU mask on), computed in fp64 from the kernel's stats."""
    g = masked_grad(x, dy, stats, True)
    gx = g * ((x.to(F64) - stats[0].to(F64)) * stats[1].to(F64))
    C = x.shape[1]
    return torch.stack([g.view(-1, nt, C).sum(1), gx.view(-1, nt, C).sum(1)]).float()


def tile_bwd_tol(p32: torch.Tensor, total: torch.Tensor) -> torch.Tensor:
    """Tolerance of the fp64 combine of fp32 tile sums p32 [T, C] against the fp64 sum over all rows: every record
    was rounded once (half_ulp each), the combine is fp64 (c64(T) of the absolute sum), the result is stored once."""
    E = half_ulp(p32).sum(0) + c64(p32.shape[0]) * p32.to(F64).abs().sum(0)
    return E + half_ulp(total.abs() + E)


# ---------------------------------------------------------------------------------------------------------------
# 3x3 / stride 2 max pool, exactly the rules in the header of csrc/pool.hip
# ---------------------------------------------------------------------------------------------------------------
NONE = 255


def pool_ref(x, pt: int, pl: int, OH: int, OW: int, relu: bool = False, dy=None):
    """x [N, C, H, W] -> (y fp64 [N, C, OH, OW], pos uint8 [N, OH, OW, C], dx bf16 [N, C, H, W] or None).
    Window (oh, ow) covers rows 2 oh - pt .. + 2 and columns 2 ow - pl .. + 2; taps are visited in window order
    kh * 3 + kw. Padding never wins; the first in-image tap starts the window, after it only a strictly greater value
    or a NaN replaces the held one (so ties keep the first, and the last NaN keeps the position). relu: a window whose
    max is not > 0 outputs 0 (NaN stays NaN), holds position 255 and routes no gradient. dx is the fp64 sum of the
    routed gradients rounded once to bf16."""
    x = x.to(F64)
    N, C, H, W = x.shape
    oh, ow = torch.arange(OH), torch.arange(OW)
    m = torch.full((N, C, OH, OW), float("-inf"), dtype=F64)
    k = torch.zeros((N, C, OH, OW), dtype=torch.uint8)
    first = torch.ones((OH, OW), dtype=torch.bool)
    taps = []
    for kh in range(3):
        ih = 2 * oh - pt + kh
        okh = (ih >= 0) & (ih < H)
        ihc = ih.clamp(0, H - 1)
        for kw in range(3):
            iw = 2 * ow - pl + kw
            okw = (iw >= 0) & (iw < W)
            iwc = iw.clamp(0, W - 1)
            ok = okh[:, None] & okw[None, :]
            v = x[:, :, ihc[:, None], iwc[None, :]]
            take = ok & (first | (v > m) | torch.isnan(v))
            m = torch.where(take, v, m)
            k = torch.where(take, torch.full_like(k, kh * 3 + kw), k)
            first = first & ~ok
            taps.append((kh * 3 + kw, ihc, iwc, ok))
    assert not bool(first.any()), "a window holds no tap of the image"
    if relu:
        dead = ~(m > 0)
        k = torch.where(dead, torch.full_like(k, NONE), k)
        m = torch.where(dead & ~torch.isnan(m), torch.zeros_like(m), m)
    dx = None
    if dy is not None:
        dy = dy.to(F64)
        acc = torch.zeros((N, C, H, W), dtype=F64)
        nn, cc = torch.arange(N)[:, None, None, None], torch.arange(C)[None, :, None, None]
        for tap, ihc, iwc, ok in taps:
            contrib = torch.where(ok & (k == tap), dy, torch.zeros_like(dy))
            acc.index_put_((nn.expand(N, C, OH, OW), cc.expand(N, C, OH, OW),
                            ihc[None, None, :, None].expand(N, C, OH, OW),
                            iwc[None, None, None, :].expand(N, C, OH, OW)), contrib, accumulate=True)
        dx = acc.to(torch.bfloat16)
    return m, k.permute(0, 2, 3, 1).contiguous(), dx


def same_or_both_nan(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Exact equality everywhere, a NaN matching a NaN (and -0 == 0)."""
    a, b = a.to(F64), b.to(F64)
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ---------------------------------------------------------------------------------------------------------------
# Shared inputs: the same bits in the test process and in the A/B child (tests/bn_pool_child.py)
# ---------------------------------------------------------------------------------------------------------------
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def bn_data(kind: str, M: int, C: int, dtype, seed: int = 0) -> torch.Tensor:
    """[M, C] of `dtype`: 'normal' N(0, 1); 'mean100' mean 100 + c, std 1; 'const' N(0, 1) with one constant channel
    (variance 0); 'outlier' N(0, 1) with row 0 at +8 std (K is taken from row 0). 'outlier1000': row 0 at +1000."""
    x = torch.randn(M, C, generator=_gen(seed), dtype=F64)
    if kind == "mean100":
        x = x + 100.0 + torch.arange(C, dtype=F64)
    elif kind == "const":
        x[:, C // 2] = 1.5
    elif kind == "outlier":
        x[0] = 8.0
    elif kind == "outlier1000":
        x[0] = 1000.0
    elif kind != "normal":
        raise ValueError(kind)
    return x.to(dtype)


def bn_params(C: int, seed: int = 1):
    """(w, b, run_mean0, run_var0) fp32."""
    g = _gen(seed)
    return (torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2, torch.randn(C, generator=g),
            torch.rand(C, generator=g) + 0.5)


def pool_planes(N: int, C: int, H: int, W: int, seed: int, offset: int = 128) -> torch.Tensor:
    """bf16 [N, C, H, W] channels_last, every (n, c) plane a permutation of distinct integers in [-offset, 256 -
    offset) (bf16-exact, H * W <= 256): no ties, both signs."""
    assert H * W <= 256
    g = _gen(seed)
    p = torch.stack([torch.randperm(256, generator=g)[:H * W] for _ in range(N * C)]).view(N, C, H, W)
    return (p - offset).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


def pool_dy(shape, seed: int) -> torch.Tensor:
    """bf16 integers in [-32, 32]: every sum of up to four is exact in bf16."""
    return torch.randint(-32, 33, shape, generator=_gen(seed)).to(torch.bfloat16).contiguous(
        memory_format=torch.channels_last)


def same_pads(H: int):
    """TF 'SAME' 3/2 pooling: (output size, top / left padding)."""
    out = -(-H // 2)
    return out, max((out - 1) * 2 + 3 - H, 0) // 2


def max_out(H: int, p: int) -> int:
    """Most windows the entry point accepts: the last one still holds an image row, 2 (OH - 1) - p < H."""
    return (H - 1 + p) // 2 + 1


PAD1_HW = [(1, 1), (2, 2), (3, 3), (4, 6), (5, 7), (6, 5), (8, 10)]
SAME_HW = [1, 2, 3, 4, 7, 8]


def pool_grid():
    """Every (name, x, pt, pl, OH, OW, relu, dy) of the exact pool tests, in a fixed order."""
    seed = 0
    for H, W in PAD1_HW:
        for C in (8, 24):
            for N in (1, 3):
                seed += 1
                OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                yield (f"pad1-{N}x{C}x{H}x{W}", pool_planes(N, C, H, W, seed), 1, 1, OH, OW, False,
                       pool_dy((N, C, OH, OW), seed + 1000))
    for H in SAME_HW:
        for W in SAME_HW:
            for relu in (False, True):
                seed += 1
                (OH, pt), (OW, pl) = same_pads(H), same_pads(W)
                yield (f"same-{H}x{W}-relu{int(relu)}", pool_planes(2, 8, H, W, seed), pt, pl, OH, OW, relu,
                       pool_dy((2, 8, OH, OW), seed + 1000))
    for pt in (0, 1, 2):
        for pl in (0, 1, 2):
            for relu in (False, True):
                seed += 1
                OH, OW = max_out(5, pt), max_out(5, pl)
                yield (f"direct-pt{pt}-pl{pl}-relu{int(relu)}", pool_planes(2, 16, 5, 5, seed), pt, pl, OH, OW, relu,
                       pool_dy((2, 16, OH, OW), seed + 1000))


TILE_T = [1, 5, 16, 130, 384, 800, 1000, 6200]
TILE_C = [64, 72, 264]
TILE_NT = 2


def tile_case(T: int, C: int, kind: str, dtype):
    """(name, x [T * 2, C], part [2, T, C]) of one tile-statistics case; the bits depend on the arguments only."""
    seed = T * 1000 + C + 7 * ("normal", "mean100").index(kind)
    x = bn_data(kind, T * TILE_NT, C, dtype, seed)
    return f"T{T}-C{C}-{kind}-{str(dtype)[6:]}", x, tile_parts(x, TILE_NT)


def tile_grid(dtypes=(torch.float32, torch.bfloat16)):
    """Every case of the tile-statistics tests, in a fixed order."""
    for T in TILE_T:
        for C in TILE_C:
            for kind in ("normal", "mean100"):
                for dtype in dtypes:
                    yield tile_case(T, C, kind, dtype)


# ---------------------------------------------------------------------------------------------------------------
# Comparison
# ---------------------------------------------------------------------------------------------------------------
WORST: dict = {}  # name -> largest |got - ref| / tol seen in this process (profiles/bn_pool_exact.md)


def close(name: str, got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> None:
    """Assert |got - ref| <= tol at EVERY element (a NaN fails) and record the worst error as a fraction of its bound."""
    got, ref, tol = got.detach().to(F64), ref.to(F64), tol.to(F64).expand_as(ref)
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    err = (got - ref).abs()
    ratio = torch.where(tol > 0, err / tol, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    WORST[name] = max(WORST.get(name, 0.0), worst if worst == worst else float("inf"))
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int(torch.where(bad.flatten(), ratio.flatten().nan_to_num(float("inf")), torch.zeros(())).argmax())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound; worst at flat index {i}: "
                             f"got {got.flatten()[i].item()!r} ref {ref.flatten()[i].item()!r} "
                             f"tol {tol.flatten()[i].item():.3e} ({worst:.3g} x bound)")
