"""The references of tests/bn_pool_ref.py against PyTorch's own float64 operators (CPU only, no GPU needed)."""
import math

import pytest
import torch
import torch.nn.functional as F

import bn_pool_ref as R
from mifx.models.cnn import _same_pad

F64 = torch.float64


@pytest.mark.parametrize("M,C", [(2, 8), (37, 24), (300, 16)])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("kind", ["normal", "mean100", "outlier"])
def test_bn_reference_matches_autograd_fp64(M, C, relu, kind):
    x = R.bn_data(kind, M, C, torch.float32, seed=M).to(F64).requires_grad_()
    w, b, _, _ = (t.to(F64) for t in R.bn_params(C))
    w.requires_grad_(), b.requires_grad_()
    dy = R.bn_data("normal", M, C, F64, seed=7)
    dres = R.bn_data("normal", M, C, F64, seed=8)
    eps = R.f32(1e-5)
    rm, rv = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
    y = F.batch_norm(x, rm, rv, w, b, True, 1.0, eps)
    y = F.relu(y) if relu else y
    y.backward(dy)
    ref = R.bn_ref(x.detach(), w.detach(), b.detach(), 1e-5, relu, dy, dres)
    kw = dict(rtol=1e-10, atol=1e-10)  # fp64 against fp64: two orders of evaluation of the same formulas
    torch.testing.assert_close(ref["y"], y.detach(), **kw)
    torch.testing.assert_close(ref["mean"], rm, **kw)
    torch.testing.assert_close(ref["var_unbiased"], rv, **kw)
    torch.testing.assert_close(ref["var"], x.detach().var(0, unbiased=False), **kw)
    torch.testing.assert_close(ref["shift"], b.detach() - ref["mean"] * ref["scale"], **kw)
    torch.testing.assert_close(ref["dgamma"], w.grad, **kw)
    torch.testing.assert_close(ref["dbeta"], b.grad, **kw)
    torch.testing.assert_close(ref["dx"], x.grad + dres, **kw)


def test_bn_reference_single_row():
    """M = 1 (PyTorch refuses it in training): variance 0, unbiased := biased, rstd = 1 / sqrt(eps), y = relu(b)."""
    x = R.bn_data("normal", 1, 8, torch.float32)
    w, b, _, _ = R.bn_params(8)
    ref = R.bn_ref(x, w, b, 1e-5, True, torch.ones(1, 8))
    assert torch.equal(ref["mean"], x[0].to(F64)) and not ref["var"].any() and not ref["var_unbiased"].any()
    torch.testing.assert_close(ref["rstd"], torch.full((8,), 1.0 / math.sqrt(R.f32(1e-5)), dtype=F64))
    assert torch.equal(ref["y"][0], torch.clamp_min(b.to(F64), 0.0))
    assert not ref["dx"].any()


def test_half_ulp_is_the_rounding_error_bound():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.99, 2.0, 3e-3, 100.25, 0.0], dtype=F64)
    assert R.half_ulp(v, torch.bfloat16).tolist()[:4] == [2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7]
    assert R.half_ulp(v)[0] == 2.0 ** -24 and R.half_ulp(v)[-1] == 0
    g = torch.Generator().manual_seed(0)
    r = torch.randn(100000, generator=g, dtype=F64) * 50
    for dt in (torch.bfloat16, torch.float32):
        err = (r.to(dt).to(F64) - r).abs()
        assert bool((err <= R.half_ulp(r, dt)).all()) and bool((err > 0.49 * R.half_ulp(r, dt)).any())


def _torch_pool(x, pad_fn, relu, dy):
    xt = x.to(F64).requires_grad_()
    h = torch.relu(xt) if relu else xt
    y = F.max_pool2d(pad_fn(h), 3, 2)
    y.backward(dy.to(F64))
    return y.detach(), xt.grad


@pytest.mark.parametrize("H,W", R.PAD1_HW + [(7, 8), (9, 9)])
def test_pool_reference_matches_max_pool2d_pad1(H, W):
    x = R.pool_planes(3, 8, H, W, seed=H * 16 + W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = R.pool_dy((3, 8, OH, OW), 5)
    y, pos, dx = R.pool_ref(x, 1, 1, OH, OW, False, dy)
    yt, dxt = _torch_pool(x, lambda t: F.pad(t, (1, 1, 1, 1), value=-math.inf), False, dy)
    assert torch.equal(y, yt)
    assert torch.equal(dx.to(F64), dxt)  # integer gradients: the sums are exact, bf16 rounding changes nothing
    assert int(pos.max()) <= 8


@pytest.mark.parametrize("H", R.SAME_HW)
@pytest.mark.parametrize("W", R.SAME_HW)
@pytest.mark.parametrize("relu", [False, True])
def test_pool_reference_matches_max_pool2d_tf_same(H, W, relu):
    x = R.pool_planes(2, 8, H, W, seed=H * 16 + W)
    (OH, pt), (OW, pl) = R.same_pads(H), R.same_pads(W)
    dy = R.pool_dy((2, 8, OH, OW), 6)
    y, pos, dx = R.pool_ref(x, pt, pl, OH, OW, relu, dy)
    yt, dxt = _torch_pool(x, lambda t: _same_pad(t, 3, 2, value=-math.inf), relu, dy)
    assert y.shape == yt.shape and torch.equal(y, yt)
    assert torch.equal(dx.to(F64), dxt)
    assert bool(((pos == R.NONE).permute(0, 3, 1, 2) == (y <= 0)).all()) if relu else int(pos.max()) <= 8


def test_pool_reference_rules():
    """Ties keep the first in-image tap, the last NaN keeps the position, padding never wins, relu kills a window."""
    x = torch.zeros(1, 1, 3, 3)
    y, pos, dx = R.pool_ref(x, 1, 1, 2, 2, False, torch.ones(1, 1, 2, 2))
    assert pos.flatten().tolist() == [4, 3, 1, 0]  # first in-image tap of each window (pad 1)
    assert dx.flatten().tolist() == [1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0]
    x = torch.arange(9.0).view(1, 1, 3, 3)
    x[0, 0, 0, 1] = x[0, 0, 1, 0] = float("nan")
    y, pos, dx = R.pool_ref(x, 1, 1, 2, 2, False, torch.ones(1, 1, 2, 2))
    assert math.isnan(y[0, 0, 0, 0]) and pos[0, 0, 0, 0] == 7 and dx[0, 0, 1, 0] == 2 and dx[0, 0, 0, 1] == 1
    x = torch.full((1, 1, 2, 2), -math.inf)
    y, pos, _ = R.pool_ref(x, 0, 0, 1, 1, False)
    assert y.item() == -math.inf and pos.item() == 0
    y, pos, dx = R.pool_ref(-torch.ones(1, 1, 2, 2), 0, 0, 1, 1, True, torch.ones(1, 1, 1, 1))
    assert y.item() == 0 and pos.item() == R.NONE and not dx.any()
