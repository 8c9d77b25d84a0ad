"""The pixel gathers of the implicit-GEMM convolutions (csrc/gemm8.hip CV 1: forward / stride-1 input gradient /
strided 1x1 "centre tap"; CV 2: grouped split-K weight gradient) against an exact reference, OFF the tile grid: at
ResNet-50's own 56 / 28 / 14 / 7 images (OH OW = 3136 / 784 / 196 / 49), non-square and all-border ones, tiles, K-tiles
and token chunks start mid-row and mid-image, straddle several images, and the multiply-high divisions by OW and OH OW
do not degenerate to shifts.

Why the comparisons need no tolerance: the operands are integer-valued bf16 (activations and dY uniform in [-3, 3],
weights in [-2, 2]), so every product and every partial sum is an integer below 2^24 -- forward |sum| <= 6 * 9 * 256 =
13,824, weight gradient <= 9 T with T <= 6272 tokens plus the integer initial gradient -- and fp32 accumulation is
exact in ANY order. bf16 outputs must equal the fp64 result cast to bf16 (round-to-nearest-even; most sums are bf16
integers, the rest exercise the rounding), fp32 weight gradients the fp64 result cast to fp32, bit for bit.

The reference is a sum over taps of (shifted, strided window of the zero-padded fp64 input) @ w[:, r, s, :]^T -- plain
indexing and matmul, pinned on the CPU against torch.nn.functional.conv2d and its autograd weight gradient.

Which kernel path a case reaches:
  test_conv3x3_exact / _pad / _c256   gemm8_conv<BM, BN, EPI_NONE / EPI_STATS> (CV 1), every (BM, BN) build
  test_conv3x3_bnbwd_exact            gemm8_conv<BM, BN, EPI_BNBWD> (CV 1)
  test_strided_1x1_exact              the same kernels with tap0 = 4, one tap (K = C; C = 64: a single K-tile)
  test_wgrad_gather_exact             gemm8_tn_grouped CONV problems (CV 2): 256 x 256 (C = Cout = 256), 128 x 128
                                      (128), narrow 256 x 64 (C = 64, Cout = 256); 3x3 and centre-tap geometry;
                                      2048- and 192-pixel chunks, the last 2048-pixel one short. (Nothing in the
                                      model records a narrow or 128-wide CONV problem; the narrow one staged the
                                      next K-tile's rows over the A half until its DMAs were folded like the plain
                                      narrow tiles')
  test_wgrad_mixed_launch             two CONV problems + a plain fp32 TN + a bf16 TN problem in one launch"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

# (H, W, stride), pad 1: the workload's own + one odd stride-2 size; non-square (an H / W swap shows); one image
# spanning many tiles; every pixel on a border
GEOMS = [(7, 7, 1), (14, 14, 1), (28, 28, 1), (56, 56, 1), (14, 14, 2), (13, 13, 2), (28, 28, 2), (56, 56, 2),
         (6, 10, 1), (5, 12, 2), (24, 24, 1), (3, 3, 1), (1, 7, 1)]
S2 = [g for g in GEOMS if g[2] == 2]
NCFG = 6  # csrc/gemm8.hip builds: (256, 256) (256, 128) (128, 256) (128, 128) (256, 64) (128, 64)
COUT_MAX = 512  # 2 x the widest BN: a case's weight is the first 2 BN rows of one shared weight


def _gid(g):
    return "x".join(map(str, g[:2])) + f"s{g[2]}" + (f"p{g[3]}" if len(g) > 3 else "")


def out_hw(h, w, stride, pad=1):
    return (h + 2 * pad - 3) // stride + 1, (w + 2 * pad - 3) // stride + 1


# ---------------------------------------------------------------------------------------------- the reference (fp64)
def _padded(x, pad):
    nb, h, w, c = x.shape
    xp = torch.zeros(nb, h + 2 * pad, w + 2 * pad, c, dtype=torch.float64, device=x.device)
    xp[:, pad:pad + h, pad:pad + w] = x.double()
    return xp


def _window(xp, r, s, stride, oh, ow):
    """Tap (r, s)'s input pixel of every output pixel: [Nb, OH, OW, C] out of the zero-padded input."""
    return xp[:, r:r + stride * (oh - 1) + 1:stride, s:s + stride * (ow - 1) + 1:stride]


def ref_conv3x3(x, w, stride, pad=1):
    """x [Nb, H, W, C], w [Cout, 3, 3, C] -> fp64 [Nb, OH, OW, Cout]."""
    oh, ow = out_hw(x.shape[1], x.shape[2], stride, pad)
    xp, wd = _padded(x, pad), w.double()
    y = torch.zeros(x.shape[0], oh, ow, w.shape[0], dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            y += torch.matmul(_window(xp, r, s, stride, oh, ow), wd[:, r, s, :].t())
    return y


def ref_conv3x3_wgrad(dy, x, stride, pad=1):
    """dy [Nb, OH, OW, Cout], x [Nb, H, W, C] -> fp64 [Cout, 3, 3, C] = per tap dY^T @ X_tap."""
    oh, ow = out_hw(x.shape[1], x.shape[2], stride, pad)
    assert tuple(dy.shape[1:3]) == (oh, ow)
    xp, d2 = _padded(x, pad), dy.double().reshape(-1, dy.shape[-1])
    dw = torch.zeros(dy.shape[-1], 3, 3, x.shape[-1], dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            dw[:, r, s, :] = torch.matmul(d2.t(), _window(xp, r, s, stride, oh, ow).reshape(-1, x.shape[-1]))
    return dw


def ref_center1x1(x, w, stride):
    """Strided 1x1 = the centre tap of a pad-1 3x3: x [Nb, H, W, C], w [Cout, C] -> fp64 [Nb, OH, OW, Cout]."""
    oh, ow = out_hw(x.shape[1], x.shape[2], stride, 1)
    return torch.matmul(_window(_padded(x, 1), 1, 1, stride, oh, ow), w.double().t())


def ref_center1x1_wgrad(dy, x, stride):
    """-> fp64 [Cout, C]."""
    oh, ow = out_hw(x.shape[1], x.shape[2], stride, 1)
    assert tuple(dy.shape[1:3]) == (oh, ow)
    return torch.matmul(dy.double().reshape(-1, dy.shape[-1]).t(),
                        _window(_padded(x, 1), 1, 1, stride, oh, ow).reshape(-1, x.shape[-1]))


def _ints(shape, lo, hi, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.bfloat16).to(device)


@pytest.mark.parametrize("geom", GEOMS + [(7, 7, 1, 0), (7, 7, 1, 2)], ids=_gid)
@pytest.mark.parametrize("c,cout", [(3, 4), (2, 3)])
def test_reference_matches_conv2d_float64(geom, c, cout):
    """The tap-sum reference == F.conv2d in float64 and its autograd weight gradient (integer operands: both exact)."""
    h, w, stride = geom[:3]
    pad = geom[3] if len(geom) > 3 else 1
    oh, ow = out_hw(h, w, stride, pad)
    x = _ints((2, h, w, c), -3, 3, 1).double()
    wt = _ints((cout, 3, 3, c), -2, 2, 2).double()
    dy = _ints((2, oh, ow, cout), -3, 3, 3).double()
    wa = wt.permute(0, 3, 1, 2).clone().requires_grad_()
    y = F.conv2d(x.permute(0, 3, 1, 2), wa, stride=stride, padding=pad)
    assert tuple(y.shape[2:]) == (oh, ow)
    assert torch.equal(ref_conv3x3(x, wt, stride, pad), y.detach().permute(0, 2, 3, 1))
    (y * dy.permute(0, 3, 1, 2)).sum().backward()
    assert torch.equal(ref_conv3x3_wgrad(dy, x, stride, pad), wa.grad.permute(0, 2, 3, 1))
    if pad == 1:  # the strided 1x1 (any stride: the centre tap of the pad-1 3x3 of the same output size)
        w1 = wt[:, 1, 1, :].clone()
        wb = w1[:, :, None, None].clone().requires_grad_()
        y1 = F.conv2d(x.permute(0, 3, 1, 2), wb, stride=stride)
        assert torch.equal(ref_center1x1(x, w1, stride), y1.detach().permute(0, 2, 3, 1))
        (y1 * dy.permute(0, 3, 1, 2)).sum().backward()
        assert torch.equal(ref_center1x1_wgrad(dy, x, stride), wb.grad[:, :, 0, 0])


# ---------------------------------------------------------------------------------------------- helpers
def _assert_off_grid(oh, ow, bm):
    """The geometry is really off the tile grid (keeps this list from being simplified back onto it)."""
    ohw = oh * ow
    assert (ohw % bm != 0 and bm % ohw != 0) or bm % ow != 0, (oh, ow, bm)


def _assert_rows_equal(y, want, oh, ow, bm, what):
    """Bit equality of [Nb OH OW, N] outputs; a failure names the first (image, oh, ow, channel) and the tile row."""
    assert y.shape == want.shape and y.dtype == want.dtype, (y.shape, want.shape, y.dtype, want.dtype)
    if torch.equal(y, want):
        return
    bad = (y != want).nonzero()
    rows = []
    for m, n in bad[:6].tolist():
        rows.append(f"(image {m // (oh * ow)}, oh {m % (oh * ow) // ow}, ow {m % ow}, channel {n}; tile row m % BM = "
                    f"{m % bm}, tile {m // bm}): got {y[m, n].item()} want {want[m, n].item()}")
    raise AssertionError(f"{what}: {bad.shape[0]} of {y.numel()} elements differ, first:\n" + "\n".join(rows))


def _assert_wgrad_equal(dw, want, c, tm, tn, what):
    """Bit equality of fp32 [Cout, taps C] weight gradients; a failure names the first (cout, tap, c)."""
    assert dw.shape == want.shape and dw.dtype == want.dtype == torch.float32
    if torch.equal(dw, want):
        return
    bad = (dw != want).nonzero()
    rows = [f"(cout {m}, tap {n // c}, c {n % c}; tile row m % {tm} = {m % tm}, tile column n % {tn} = {n % tn}): "
            f"got {dw[m, n].item()} want {want[m, n].item()}" for m, n in bad[:6].tolist()]
    raise AssertionError(f"{what}: {bad.shape[0]} of {dw.numel()} elements differ, first:\n" + "\n".join(rows))


def _check_stats(y, part, bm):
    """EPI_STATS: per-tile (mean, M2) of the STORED output, per tile and combined (the tolerances of
    test_conv3x3_forward_stats_backward)."""
    M, N = y.shape
    T = M // bm
    assert part.shape == (2, T, N)
    yd = y.double()
    yt = yd.view(T, bm, N)
    tmean = yt.mean(1)
    tm2 = ((yt - tmean[:, None, :]) ** 2).sum(1)
    pm, pm2 = part[0].double(), part[1].double()
    torch.testing.assert_close(pm, tmean, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(pm2 / bm, tm2 / bm, rtol=1e-4, atol=1e-5)
    mean = pm.mean(0)
    var = (pm2.sum(0) + bm * ((pm - mean) ** 2).sum(0)) / M
    torch.testing.assert_close(mean, yd.mean(0), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(var, yd.var(0, unbiased=False), rtol=1e-4, atol=1e-5)


@functools.lru_cache(maxsize=None)
def _fwd_case(kind, h, w, stride, pad, c):
    """Integer operands and the exact result (cast to bf16) at the batch of the 256-row tiles and COUT_MAX channels;
    a 128-row-tile case uses the first images, a narrower configuration the first 2 BN output channels."""
    oh, ow = out_hw(h, w, stride, pad)
    nb = 256 // math.gcd(256, oh * ow)
    x = _ints((nb, h, w, c), -3, 3, 11, "cuda")
    if kind == "3x3":
        wt = _ints((COUT_MAX, 3, 3, c), -2, 2, 12, "cuda")
        ref = ref_conv3x3(x, wt, stride, pad)
    else:
        wt = _ints((COUT_MAX, c), -2, 2, 13, "cuda")
        ref = ref_center1x1(x, wt, stride)
    ref = ref.reshape(-1, COUT_MAX)
    assert ref.abs().max().item() <= 6 * 9 * 256 and torch.equal(ref, ref.round())
    return x, wt, ref.to(torch.bfloat16)


def _run_fwd(kind, geom, pad, c, ci, epi, extra=None):
    from mifx.ops import gemm as hg

    cfgs = hg.gemm8_configs()
    assert len(cfgs) == NCFG
    bm, bn = cfgs[ci]
    h, w, stride = geom
    oh, ow = out_hw(h, w, stride, pad)
    _assert_off_grid(oh, ow, bm)
    nb = bm // math.gcd(bm, oh * ow)  # the smallest batch the kernel accepts
    M, cout = nb * oh * ow, 2 * bn  # (a tile with n0 != 0 exists)
    assert M % bm == 0 and M // bm >= 2 and cout <= COUT_MAX and c >= 64 and c & (c - 1) == 0
    x, wt, ref = _fwd_case(kind, h, w, stride, pad, c)
    xs, ws, want = x[:nb], wt[:cout].reshape(cout, -1), ref[:M, :cout].contiguous()
    what = f"{kind} {h}x{w} stride {stride} pad {pad} C {c} Cout {cout} tile {bm}x{bn} epi {epi}"
    if kind == "3x3":
        kw = extra(M, cout) if extra is not None else {}
        y, part = hg.gemm8_conv3x3(xs, ws, stride, pad, epi, cfg=ci, **kw)
    else:
        y, part = hg.gemm8_conv1x1_strided(xs, ws, stride, epi, cfg=ci)
    _assert_rows_equal(y, want, oh, ow, bm, what)
    if epi == 5:
        _check_stats(y, part, bm)
    return y, part, bm


# ---------------------------------------------------------------------------------------------- CV 1
@gpu
@pytest.mark.parametrize("epi", [0, 5])
@pytest.mark.parametrize("ci", range(NCFG))
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=[_gid(g) for g in GEOMS])
def test_conv3x3_exact(gi, ci, epi):
    """gemm8_conv3x3 at every geometry x every tile configuration, C alternating 64 / 128 (cshift 6 / 7)."""
    _run_fwd("3x3", GEOMS[gi], 1, 64 if (gi + ci) % 2 == 0 else 128, ci, epi)


@gpu
@pytest.mark.parametrize("ci", [0, 3])
def test_conv3x3_exact_c256(ci):
    _run_fwd("3x3", (14, 14, 1), 1, 256, ci, 5)


@gpu
@pytest.mark.parametrize("ci", [0, 3])
@pytest.mark.parametrize("pad", [0, 2])
def test_conv3x3_exact_pad(pad, ci):
    """pad 0 and pad 2 (the host check accepts them): 7x7 -> 5x5 / 9x9."""
    _run_fwd("3x3", (7, 7, 1), pad, 64 if ci else 128, ci, 0)


@gpu
@pytest.mark.parametrize("ci", range(NCFG))
@pytest.mark.parametrize("geom", [(28, 28, 1), (5, 12, 2)], ids=_gid)
def test_conv3x3_bnbwd_exact(geom, ci):
    """EPI_BNBWD on the gathered operand: the stored dY bit-exact, the per-tile (sum g, sum g xhat) against fp64 sums
    of the stored values (test_gemm8_bnbwd_epilogue_partials' check and tolerances). The BatchNorm input and
    statistics are small dyadic numbers, so the mask and xhat are exact too."""
    held = {}

    def extra(M, cout):
        g = torch.Generator().manual_seed(21)
        pick = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (cout,), generator=g)].cuda()  # noqa: E731
        mean, beta = pick([-1.0, -0.5, -0.25, 0.0, 0.25, 0.75]), pick([-0.5, -0.25, 0.0, 0.25, 0.5])
        rstd, gamma = pick([0.5, 1.0, 2.0]), pick([-1.0, -0.5, 0.5, 1.0, 2.0])
        held["u"] = _ints((M, cout), -3, 3, 22, "cuda")
        held["stats"] = torch.stack([mean, rstd, gamma * rstd, beta - mean * gamma * rstd]).contiguous()
        return {"bias": held["u"], "z": held["stats"]}

    y, part, bm = _run_fwd("3x3", geom, 1, 128 if ci % 2 else 64, ci, 8, extra)
    M, N = y.shape
    T = M // bm
    assert part.shape == (2, T, N)
    u, st = held["u"].double(), held["stats"].double()
    gg = torch.where(u * st[2] + st[3] > 0, y.double(), torch.zeros((), dtype=torch.float64, device=y.device))
    xhat = (u - st[0]) * st[1]
    torch.testing.assert_close(part[0].double(), gg.view(T, bm, N).sum(1), rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(part[1].double(), (gg * xhat).view(T, bm, N).sum(1), rtol=1e-4, atol=1e-3)


@gpu
@pytest.mark.parametrize("epi", [0, 5])
@pytest.mark.parametrize("ci", range(NCFG))
@pytest.mark.parametrize("gi", range(len(S2)), ids=[_gid(g) for g in S2])
def test_strided_1x1_exact(gi, ci, epi):
    """gemm8_conv1x1_strided (centre tap) at the stride-2 geometries x every configuration; C = 64 is one K-tile."""
    _run_fwd("1x1", S2[gi], 1, 64 if (gi + ci) % 2 == 0 else 128, ci, epi)


# ---------------------------------------------------------------------------------------------- CV 2
WG_PATHS = [(256, 256, 256, 256), (128, 128, 128, 128), (64, 256, 256, 64)]  # (C, Cout, tile rows, tile columns)


def _wgrad_nb(ohw):
    """The smallest batch >= 2 whose token count is a multiple of the 64-row K-tile and makes the 2048-pixel
    production chunk give at least two chunks, the last one short."""
    step = 64 // math.gcd(64, ohw)
    nb = step
    while nb < 2 or nb * ohw <= 2048 or nb * ohw % 2048 == 0:
        nb += step
    return nb


@functools.lru_cache(maxsize=None)
def _wgrad_case(h, w, stride, center, c, cout):
    oh, ow = out_hw(h, w, stride, 1)
    nb = _wgrad_nb(oh * ow)
    x = _ints((nb, h, w, c), -3, 3, 31, "cuda")
    dy = _ints((nb, oh, ow, cout), -3, 3, 32, "cuda")
    ref = ref_center1x1_wgrad(dy, x, stride) if center else ref_conv3x3_wgrad(dy, x, stride)
    ref = ref.reshape(cout, -1)
    init = _ints(tuple(ref.shape), -8, 8, 33, "cuda").float()
    assert ref.abs().max().item() + 8 < 2 ** 24 and torch.equal(ref, ref.round())
    return x, dy.reshape(-1, cout), ref.float(), init


def _run_wgrad(geom, center, path, chunk):
    from mifx.ops import gemm as hg

    h, w, stride = geom
    c, cout, tm, tn = path
    oh, ow = out_hw(h, w, stride, 1)
    _assert_off_grid(oh, ow, 64)  # (64: the K-tile of token rows)
    x, dy2, ref, init = _wgrad_case(h, w, stride, center, c, cout)
    T, taps = dy2.shape[0], 1 if center else 9
    assert T % 64 == 0 and T == x.shape[0] * oh * ow and T > 2048 and T % 2048 and chunk % 64 == 0
    geo = hg.conv_geo(x.shape[0], h, w, c, stride, 1, x.device, center1x1=center)
    assert geo.mifx_taps == taps
    items = (cout // tm) * (taps * c // tn) * -(-T // chunk)  # (the tile path the host selected)
    what = (f"{'centre-tap 1x1' if center else '3x3'} weight gradient {h}x{w} stride {stride} C {c} Cout {cout} "
            f"T {T} chunk {chunk} tiles {tm}x{tn}")
    outs = []
    for _ in range(2):
        dst = torch.full_like(ref, float("nan"))
        assert hg.gemm8_tn_grouped([(dy2, x, dst, geo, chunk)], accumulate=False) == items
        outs.append(dst)
    _assert_wgrad_equal(outs[0], ref, c, tm, tn, what + " (overwrite)")
    assert torch.equal(outs[0], outs[1]), what + ": two calls differ"
    dst = init.clone()
    assert hg.gemm8_tn_grouped([(dy2, x, dst, geo, chunk)], accumulate=True) == items
    _assert_wgrad_equal(dst, ref + init, c, tm, tn, what + " (accumulate)")


@gpu
@pytest.mark.parametrize("chunk", [2048, 192])
@pytest.mark.parametrize("path", WG_PATHS, ids=["256x256", "128x128", "narrowN"])
@pytest.mark.parametrize("gi", range(len(GEOMS)), ids=[_gid(g) for g in GEOMS])
def test_wgrad_gather_exact(gi, path, chunk):
    _run_wgrad(GEOMS[gi], False, path, chunk)


@gpu
@pytest.mark.parametrize("chunk", [2048, 192])
@pytest.mark.parametrize("path", WG_PATHS, ids=["256x256", "128x128", "narrowN"])
@pytest.mark.parametrize("gi", range(len(S2)), ids=[_gid(g) for g in S2])
def test_wgrad_center_tap_exact(gi, path, chunk):
    _run_wgrad(S2[gi], True, path, chunk)


@gpu
def test_wgrad_mixed_launch():
    """Two conv problems of different geometry, tile path and chunk around a plain fp32 TN and a bf16 TN problem in
    ONE launch: the per-problem geometry and first token do not leak between problems."""
    from mifx.ops import gemm as hg

    xa, dya, refa, inita = _wgrad_case(14, 14, 1, False, 256, 256)
    xb, dyb, refb, _ = _wgrad_case(13, 13, 2, True, 128, 128)
    ga = hg.conv_geo(xa.shape[0], 14, 14, 256, 1, 1, xa.device)
    gb = hg.conv_geo(xb.shape[0], 13, 13, 128, 2, 1, xb.device, center1x1=True)
    a1, b1 = _ints((1088, 128), -3, 3, 41, "cuda"), _ints((1088, 256), -3, 3, 42, "cuda")
    a2, b2 = _ints((448, 128), -3, 3, 43, "cuda"), _ints((448, 128), -2, 2, 44, "cuda")
    ref1 = (a1.double().t() @ b1.double()).float()
    ref2 = (a2.double().t() @ b2.double()).to(torch.bfloat16)
    outs = []
    for _ in range(2):
        ca, cb = inita.clone(), torch.full_like(refb, float("nan"))
        c1 = torch.full_like(ref1, float("nan"))
        c2 = torch.full_like(ref2, float("nan"))
        hg.gemm8_tn_grouped([(dya, xa, ca, ga, 2048), (a1, b1, c1, None, 320), (dyb, xb, cb, gb, 192), (a2, b2, c2)],
                            accumulate=[True, False, False, False])
        outs.append((ca, c1, cb, c2))
    ca, c1, cb, c2 = outs[0]
    _assert_wgrad_equal(ca, refa + inita, 256, 256, 256, "mixed launch: 3x3 14x14 (accumulate)")
    _assert_wgrad_equal(cb, refb, 128, 128, 128, "mixed launch: centre tap 13x13 stride 2")
    assert torch.equal(c1, ref1), "mixed launch: plain fp32 TN problem"
    assert torch.equal(c2, ref2), "mixed launch: bf16 TN problem"
    for p, q in zip(*outs):
        assert torch.equal(p, q)


# ---------------------------------------------------------------------------------------------- random operands
# Derived bounds: a bf16 output is one rounding of the accumulated sum (2^-9 relative, taken with a factor 2) on top
# of fp32 accumulation of K exact bf16 x bf16 products in any order (<= K 2^-24 A, A = sum |x||w|); an fp32 weight
# gradient is the accumulation alone over T tokens.
def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).cuda()


@gpu
@pytest.mark.parametrize("kind", ["3x3", "1x1"])
def test_forward_random_operands_derived_bound(kind):
    from mifx.ops import gemm as hg

    ci = hg.gemm8_configs().index((128, 128))
    if kind == "3x3":
        (h, w, stride), c, cout = (14, 14, 1), 128, 256
        x, wt = _rand((32, h, w, c), 51), _rand((cout, 3, 3, c), 52, (9 * c) ** -0.5)
        y, _ = hg.gemm8_conv3x3(x, wt.reshape(cout, -1), stride, 1, 0, cfg=ci)
        ref, A, K = ref_conv3x3(x, wt, stride), ref_conv3x3(x.abs(), wt.abs(), stride), 9 * c
    else:
        (h, w, stride), c, cout = (13, 13, 2), 128, 256
        x, wt = _rand((128, h, w, c), 53), _rand((cout, c), 54, c ** -0.5)
        y, _ = hg.gemm8_conv1x1_strided(x, wt, stride, 0, cfg=ci)
        ref, A, K = ref_center1x1(x, wt, stride), ref_center1x1(x.abs(), wt.abs(), stride), c
    ref, A = ref.reshape(-1, cout), A.reshape(-1, cout)
    err, bound = (y.double() - ref).abs(), 2.0 ** -8 * ref.abs() + K * 2.0 ** -24 * A
    assert (err <= bound).all(), (err - bound).max().item()


@gpu
@pytest.mark.parametrize("center", [False, True])
def test_wgrad_random_operands_derived_bound(center):
    from mifx.ops import gemm as hg

    (h, w, stride), c, cout, chunk = ((13, 13, 2), 128, 128, 192) if center else ((14, 14, 1), 256, 256, 2048)
    oh, ow = out_hw(h, w, stride, 1)
    nb = _wgrad_nb(oh * ow)
    x, dy = _rand((nb, h, w, c), 61), _rand((nb, oh, ow, cout), 62)
    fn = ref_center1x1_wgrad if center else ref_conv3x3_wgrad
    ref, A = fn(dy, x, stride).reshape(cout, -1), fn(dy.abs(), x.abs(), stride).reshape(cout, -1)
    T = nb * oh * ow
    dw = torch.full(tuple(ref.shape), float("nan"), device="cuda")
    geo = hg.conv_geo(nb, h, w, c, stride, 1, x.device, center1x1=center)
    hg.gemm8_tn_grouped([(dy.reshape(T, cout), x, dw, geo, chunk)], accumulate=False)
    err, bound = (dw.double() - ref).abs(), T * 2.0 ** -24 * A
    assert (err <= bound).all(), (err - bound).max().item()
