"""Fused BatchNorm + ReLU kernels (csrc/bn_relu.hip) against the fp64 references and derived bounds of
tests/bn_pool_ref.py. Per-channel outputs (mean, rstd, scale, shift, running statistics) are held to the fp64 truth of
the stored input; elementwise outputs and gradient sums to staged references built from the kernel's own fp32
per-channel outputs, with the ReLU mask reproduced exactly -- every element is compared. No tolerance here is a number
of its own: each comes from a formula in bn_pool_ref.py. Every launch is repeated and must return the same bits.

Shapes follow blocks_for / block_rows / the `r + 3 * rpb < r1` loops / combine2 / tile_groups of the source; the
one-launch tile finalize runs in tests/test_bn_pool_variants.py."""
import pytest
import torch

import bn_pool_ref as R
import mifx.ops.bn_relu as bnr
from bn_pool_child import EPS, run_tile_case
from mifx.ops._lib import check, ptr, stream_handle

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
# (M, C): M = 1 | fewer rows than row slices | around four rows per slice at rpb = 256 (x3) | rpb = 85, one idle
# thread, uneven block_rows | the ResNet 28x28 case | rpb = 1, tail loop | nb = 129: combine2's unrolled loop once, then
# its tail | nb clamps to 512, uneven blocks
SHAPES = [(1, 8), (3, 8), (1023, 8), (1024, 8), (1025, 8), (700, 24), (784, 64), (19, 2048), (4100, 1024),
          (16500, 1024)]
KINDS = ["normal", "mean100", "const", "outlier"]


def cpu(t):
    return t.detach().cpu()


def same_bits(*pairs):
    for a, b in pairs:
        assert a.dtype == b.dtype and torch.equal(a, b), "two runs of the same launch differ"


def raw_bwd(dy, x, w32, stats, relu, dres):
    """mifx_bn_relu_bwd as bnr._bwd launches it, keeping kbuf (the per-channel dx coefficients)."""
    M, C = x.shape
    nb = bnr._fns()["blocks"](M, C)
    part = torch.empty(2, nb, C, device=x.device, dtype=torch.float32)
    kbuf = torch.empty(3, C, device=x.device, dtype=torch.float32)
    dgb = torch.empty(2, C, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    check(bnr._fns()["bwd"](bnr._dt(x), ptr(dy), ptr(x), ptr(dres), M, C, ptr(w32), ptr(stats), int(relu), ptr(part),
                            ptr(kbuf), ptr(dx), ptr(dgb[0]), ptr(dgb[1]), stream_handle(x.device)), "mifx_bn_relu_bwd")
    return dx, dgb, kbuf


def raw_bwd_tiles(dy, x, w32, stats, dres, part, act):
    M, C = x.shape
    kbuf = torch.empty(3, C, device=x.device, dtype=torch.float32)
    dgb = torch.empty(2, C, device=x.device, dtype=torch.float32)
    dx = torch.empty_like(x)
    check(bnr._fns()["bwd_tiles"](bnr._dt(x), ptr(dy), ptr(x), ptr(dres), M, C, ptr(w32), ptr(stats), 1, ptr(part[0]),
                                  ptr(part[1]), part.shape[1], ptr(kbuf), ptr(dx), ptr(dgb[0]), ptr(dgb[1]), ptr(act),
                                  stream_handle(x.device)), "mifx_bn_relu_bwd_tiles")
    return dx, dgb, kbuf


def check_stats(tag, stats, truth, tol):
    st = cpu(stats)
    for i, key in enumerate(("mean", "rstd", "scale", "shift")):
        R.close(f"{tag}/{key}", st[i], truth[key], tol[key])
    return st


def check_running(tag, rm, rv, rm0, rv0, truth, tol, momentum):
    R.close(f"{tag}/run_mean", cpu(rm), R.running_ref(rm0, truth["mean"], momentum),
            R.running_tol(rm0, truth["mean"], tol["mean"], momentum))
    R.close(f"{tag}/run_var", cpu(rv), R.running_ref(rv0, truth["var_unbiased"], momentum),
            R.running_tol(rv0, truth["var_unbiased"], tol["var_unbiased"], momentum))


def check_backward(tag, xc, dyc, dresc, st, w, relu, k, dtype, dx, dgb, kbuf):
    """dgamma / dbeta against fp64 sums with the exact mask, the finalize coefficients, dx against its staged value."""
    dbeta, dgamma, tb, tg = R.stage_bwd_sums(xc, dyc, st, relu, k)
    R.close(f"{tag}/dbeta", cpu(dgb[1]), dbeta, tb)
    R.close(f"{tag}/dgamma", cpu(dgb[0]), dgamma, tg)
    check_coeffs_and_dx(tag, xc, dyc, dresc, st, w, relu, dtype, dx, dgb, kbuf)


def check_coeffs_and_dx(tag, xc, dyc, dresc, st, w, relu, dtype, dx, dgb, kbuf):
    kref, ktol = R.stage_kbuf(xc.shape[0], w, st, cpu(dgb[0]), cpu(dgb[1]))
    R.close(f"{tag}/kbuf", cpu(kbuf), kref, ktol)
    dx_ref, dx_tol = R.stage_bwd(xc, dyc, st, cpu(kbuf), relu, dresc, dtype)
    R.close(f"{tag}/dx", cpu(dx), dx_ref, dx_tol)


# ---------------------------------------------------------------------------------------------------------------
# direct passes
# ---------------------------------------------------------------------------------------------------------------
def test_shape_refusals():
    blocks = bnr._fns()["blocks"]
    for C in (4, 12, 2056):
        assert blocks(100, C) == -1
    assert blocks(0, 64) == -1 and blocks(16500, 1024) == 512 and blocks(4100, 1024) == 129 and blocks(784, 64) == 2
    assert not bnr.native_ok(torch.zeros(4, 2056, device="cuda"))
    assert bnr.native_ok(torch.zeros(4, 2048, device="cuda"))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("M,C", SHAPES)
def test_direct_forward_backward(M, C, kind, dtype):
    xc = R.bn_data(kind, M, C, dtype, seed=M + C)
    dyc = R.bn_data("normal", M, C, dtype, seed=M + C + 1)
    dresc = R.bn_data("normal", M, C, dtype, seed=M + C + 2)
    w, b, rm0, rv0 = R.bn_params(C)
    x, dy, dres, wg, bg = (t.cuda() for t in (xc, dyc, dresc, w, b))
    assert bnr.native_ok(x)
    k = R.chain(M, C, bnr._fns()["blocks"](M, C))
    truth = R.bn_ref(xc, w, b, EPS)
    tol = R.direct_stats_bounds(xc, truth, w, b, EPS, k)
    tag = f"direct-{IDS[DTYPES.index(dtype)]}"
    kept = None
    for relu, momentum, with_dres in ((True, 0.1, True), (False, 1.0, False)):
        runs = []
        for _ in range(2):
            rm, rv = rm0.cuda(), rv0.cuda()
            y, s, w32, stats = bnr._fwd(x, None, wg, bg, rm, rv, momentum, EPS, relu)
            runs.append((y, stats, rm, rv))
        assert s is x
        same_bits(*zip(*runs))
        y, stats, rm, rv = runs[0]
        st = check_stats(tag, stats, truth, tol)
        check_running(tag, rm, rv, rm0, rv0, truth, tol, momentum)
        y_ref, y_tol = R.stage_fwd(xc, st, relu, dtype)
        R.close(f"{tag}/y", cpu(y), y_ref, y_tol)
        kept = stats if relu else kept
        dr = dres if with_dres else None
        dx, dgb = bnr._bwd(dy, x, w32, stats, relu, dr)
        dx2, dgb2, kbuf = raw_bwd(dy, x, w32, stats, relu, dr)
        same_bits((dx, dx2), (dgb[0], dgb2[0]), (dgb[1], dgb2[1]))
        check_backward(tag, xc, dyc, dresc if with_dres else None, st, w, relu, k, dtype, dx, dgb, kbuf)
    # no running statistics: the same batch statistics, bit for bit
    _, _, _, stats = bnr._fwd(x, None, wg, bg, None, None, 0.1, EPS, True)
    same_bits((stats, kept))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_zero_preactivation_is_masked(dtype):
    """Hand-made stats (scale 1, shift -0.5, mean 0.5, rstd 1): x = 0.5 gives a pre-activation of exactly 0, which
    the forward outputs as 0 and the backward masks (`t <= 0`); its neighbours one bf16 step either side do not tie."""
    M, C = 96, 16
    xc = R.bn_data("normal", M, C, dtype, seed=5)
    xc[::3] = 0.5
    xc[1::12] = 0.5 + 2.0 ** -8
    xc[2::12] = 0.5 - 2.0 ** -9
    dyc = R.bn_data("normal", M, C, dtype, seed=6)
    dyc[::3] = 1000.0  # an unmasked zero would move dbeta by 1000 per element
    stats = torch.stack([torch.full((C,), 0.5), torch.ones(C), torch.ones(C), torch.full((C,), -0.5)])
    w = torch.ones(C)
    assert int((R.preact(xc, stats) == 0).sum()) == (M // 3) * C
    x, dy, sg, wg = xc.cuda(), dyc.cuda(), stats.cuda(), w.cuda()
    y = torch.empty_like(x)
    check(bnr._fns()["apply"](bnr._dt(x), ptr(x), M, C, ptr(sg[2]), ptr(sg[3]), 1, ptr(y), stream_handle(x.device)),
          "mifx_bn_relu_apply")
    y_ref, y_tol = R.stage_fwd(xc, stats, True, dtype)
    R.close("zero/y", cpu(y), y_ref, y_tol)
    assert not cpu(y)[::3].any() and bool((cpu(y)[1::12] > 0).all())
    dx, dgb = bnr._bwd(dy, x, wg, sg, True, None)
    dx2, dgb2, kbuf = raw_bwd(dy, x, wg, sg, True, None)
    same_bits((dx, dx2), (dgb[0], dgb2[0]), (dgb[1], dgb2[1]))
    check_backward("zero", xc, dyc, None, stats, w, True, R.chain(M, C, 1), dtype, dx, dgb, kbuf)
    g = R.masked_grad(xc, dyc, stats, True)
    assert not g[::3].any() and float(cpu(dgb[1]).abs().max()) < 1000.0


# ---------------------------------------------------------------------------------------------------------------
# residual-add forms
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("M,C", [(1, 8), (3, 8), (1025, 8), (700, 24), (784, 64), (19, 2048)])
def test_add_forward_stores_rounded_sum_and_measures_it(M, C, dtype):
    ac = R.bn_data("normal", M, C, dtype, seed=M)
    bc = R.bn_data("mean100", M, C, dtype, seed=M + 1)
    sc = (ac.float() + bc.float()).to(dtype)  # round_T(a + b)
    w, b, rm0, rv0 = R.bn_params(C)
    runs = []
    for _ in range(2):
        rm, rv = rm0.cuda(), rv0.cuda()
        y, s, w32, stats = bnr._fwd(ac.cuda(), bc.cuda(), w.cuda(), b.cuda(), rm, rv, 0.1, EPS, True)
        runs.append((y, s, stats, rm, rv))
    same_bits(*zip(*runs))
    y, s, stats, rm, rv = runs[0]
    assert torch.equal(cpu(s), sc), "s is not round_T(a + b) bit for bit"
    truth = R.bn_ref(sc, w, b, EPS)
    tol = R.direct_stats_bounds(sc, truth, w, b, EPS, R.chain(M, C, bnr._fns()["blocks"](M, C)))
    st = check_stats("add", stats, truth, tol)
    check_running("add", rm, rv, rm0, rv0, truth, tol, 0.1)
    y_ref, y_tol = R.stage_fwd(sc, st, True, dtype)
    R.close("add/y", cpu(y), y_ref, y_tol)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("M,C", [(5, 24), (5, 64), (37, 8), (700, 24)])
def test_inference_apply_over_sum(M, C, relu, dtype):
    """mifx_bn_add_relu_apply through the inference code's binding: M = 5 leaves the x2 branch's single-row loop as the
    only loop. s_out is round_T(x + x2) bit for bit, y the staged value of the stored sum; without x2 the same rows go
    through the four-row loop."""
    from mifx.models.resnet_infer import _bn_fns

    ac = R.bn_data("normal", M, C, dtype, seed=M + 3)
    bc = R.bn_data("outlier", M, C, dtype, seed=M + 4)
    sc = (ac.float() + bc.float()).to(dtype)
    w, b, _, _ = R.bn_params(C)
    stats = torch.stack([torch.zeros(C), torch.ones(C), w, b])
    a, bb, scale, shift = ac.cuda(), bc.cuda(), w.cuda(), b.cuda()
    outs = []
    for _ in range(2):
        y, s = torch.empty_like(a), torch.empty_like(a)
        check(_bn_fns()(bnr._dt(a), ptr(a), ptr(bb), ptr(s), M, C, ptr(scale), ptr(shift), relu, ptr(y),
                        stream_handle(a.device)), "mifx_bn_add_relu_apply")
        outs.append((y, s))
    same_bits(*zip(*outs))
    y, s = outs[0]
    assert torch.equal(cpu(s), sc), "s_out is not round_T(x + x2) bit for bit"
    y_ref, y_tol = R.stage_fwd(sc, stats, bool(relu), dtype)
    R.close("apply/y_sum", cpu(y), y_ref, y_tol)
    y1 = torch.empty_like(a)
    check(_bn_fns()(bnr._dt(a), ptr(s), None, None, M, C, ptr(scale), ptr(shift), relu, ptr(y1),
                    stream_handle(a.device)), "mifx_bn_add_relu_apply")
    same_bits((y1, y))  # one fused multiply-add per element on either branch
    assert _bn_fns()(bnr._dt(a), ptr(a), ptr(bb), None, M, C, ptr(scale), ptr(shift), relu, ptr(y),
                     stream_handle(a.device)) == -1  # x2 without s_out


# ---------------------------------------------------------------------------------------------------------------
# tile statistics
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", R.TILE_C)
@pytest.mark.parametrize("T", R.TILE_T)
def test_tile_statistics_forward(T, C):
    """T tiles of 2 rows: 1, 5 leave slices empty; 130 runs the 8-tile unrolled loop and its tail; 384 two groups;
    800 the 4-unrolled group merge; 1000 unrolled + tail; 6200 the 32-group clamp. C = 72, 264 have `c >= C` lanes in
    the last 64-channel block, 264 a second block of bn_tiles_final."""
    assert bnr._fns()["tiles_ws"](T, C) == min(max(T // 192, 1), 32) * C * 3
    w, b, rm0, rv0 = R.bn_params(C)
    for kind, momentum in (("normal", 0.1), ("mean100", 1.0)):
        for dtype in DTYPES:
            name, xc, part = R.tile_case(T, C, kind, dtype)
            tag = f"tiles-{IDS[DTYPES.index(dtype)]}"
            truth = R.bn_ref(xc, w, b, EPS)
            tol = R.tile_stats_bounds(part, R.TILE_NT, truth, w, b, EPS)
            y, stats, rm, rv = run_tile_case(xc, part, momentum)
            y2, stats2, rm2, rv2 = run_tile_case(xc, part, momentum)
            same_bits((y, y2), (stats, stats2), (rm, rm2), (rv, rv2))
            y3, stats3, rm3, rv3 = run_tile_case(xc, part, momentum, apply=False)
            assert y3 is None
            same_bits((stats, stats3), (rm, rm3), (rv, rv3))
            st = check_stats(tag, stats, truth, tol)
            check_running(tag, rm, rv, rm0, rv0, truth, tol, momentum)
            y_ref, y_tol = R.stage_fwd(xc, st, True, dtype)
            R.close(f"{tag}/y", cpu(y), y_ref, y_tol)
    yn, statsn, _, _ = run_tile_case(xc, part, 0.1, relu=False)
    y_ref, y_tol = R.stage_fwd(xc, cpu(statsn), False, dtype)
    R.close("tiles/y_norelu", cpu(yn), y_ref, y_tol)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [24, 264])
@pytest.mark.parametrize("T", [1, 33, 129])
def test_tile_backward(T, C, dtype):
    """mifx_bn_relu_bwd_tiles: combine2 over T tile records (129: its unrolled loop once, then the tail), the apply
    pass, and `act`, which must be the forward's y bit for bit."""
    nt = R.TILE_NT
    M = T * nt
    xc = R.bn_data("normal", M, C, dtype, seed=T + C)
    dyc = R.bn_data("normal", M, C, dtype, seed=T + C + 1)
    dresc = R.bn_data("normal", M, C, dtype, seed=T + C + 2)
    w, _, _, _ = R.bn_params(C)
    y, stats, _, _ = run_tile_case(xc, R.tile_parts(xc, nt))
    st = cpu(stats)
    bpart = R.tile_bwd_parts(xc, dyc, st, nt)
    x, dy, dres, pg, wg = xc.cuda(), dyc.cuda(), dresc.cuda(), bpart.cuda(), w.cuda()
    g = R.masked_grad(xc, dyc, st, True)
    dbeta = g.sum(0)
    dgamma = (g * ((xc.double() - st[0].double()) * st[1].double())).sum(0)
    for dr, drc in ((None, None), (dres, dresc)):
        act = torch.empty_like(x)
        dx, dgb = bnr._bwd_tiles(dy, x, wg, stats, dr, pg, act=act)
        act2 = torch.empty_like(x)
        dx2, dgb2, kbuf = raw_bwd_tiles(dy, x, wg, stats, dr, pg, act2)
        same_bits((dx, dx2), (dgb[0], dgb2[0]), (dgb[1], dgb2[1]), (act, act2))
        same_bits((act, y))
        R.close("tiles-bwd/dbeta", cpu(dgb[1]), dbeta, R.tile_bwd_tol(bpart[0], dbeta))
        R.close("tiles-bwd/dgamma", cpu(dgb[0]), dgamma, R.tile_bwd_tol(bpart[1], dgamma))
        check_coeffs_and_dx("tiles-bwd", xc, dyc, drc, st, w, True, dtype, dx, dgb, kbuf)
    dx3, dgb3 = bnr._bwd_tiles(dy, x, wg, stats, None, pg)  # act is optional
    dx4, _, _ = raw_bwd_tiles(dy, x, wg, stats, None, pg, None)
    same_bits((dx3, dx4))
