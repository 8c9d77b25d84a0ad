"""3x3 / stride 2 max pool (csrc/pool.hip) against the exact reference of tests/bn_pool_ref.py: the output, the saved
uint8 window positions and the input gradient must be equal EVERYWHERE. Inputs make that possible: every (n, c) plane
holds distinct bf16-exact integers (or hand-placed ties / NaN / -inf), gradients are integers in [-32, 32] whose sums
of up to four are exact in bf16. tests/test_bn_pool_ref.py shows the reference alone equals F.max_pool2d on them.

The default process runs maxpool_fwd2 and, on even pad-1 images, maxpool_bwd_even; maxpool_fwd and the general gather
on even images run in tests/test_bn_pool_variants.py. The `long long` index instantiations need more than 4e9 work
items and stay untested."""
import math

import pytest
import torch

import bn_pool_ref as R
from bn_pool_child import run_pool_case

pytestmark = pytest.mark.gpu

CASES = {c[0]: c[1:] for c in R.pool_grid()}
NAN, INF = float("nan"), math.inf


def check_case(x, pt, pl, OH, OW, relu, dy):
    y, pos, dx = run_pool_case(x, pt, pl, OH, OW, relu, dy)
    ry, rpos, rdx = R.pool_ref(x, pt, pl, OH, OW, relu, dy)
    assert y.dtype == torch.bfloat16 and y.is_contiguous(memory_format=torch.channels_last)
    assert R.same_or_both_nan(y.cpu(), ry), "forward output differs"
    assert pos.dtype == torch.uint8 and torch.equal(pos.cpu(), rpos), "window positions differ"
    assert dx.shape == x.shape and R.same_or_both_nan(dx.cpu(), rdx), "input gradient differs"
    return y.cpu(), pos.cpu(), dx.cpu()


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("pad1-")])
def test_pad1_matches_reference_everywhere(name):
    from mifx.ops.pool import max_pool3s2

    x, pt, pl, OH, OW, relu, dy = CASES[name]
    y, _, dx = check_case(x, pt, pl, OH, OW, relu, dy)
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    yp = max_pool3s2(xg)  # the public entry computes the same OH, OW
    yp.backward(dy.cuda())
    assert type(yp.grad_fn).__name__.startswith("_MaxPool3s2")
    assert torch.equal(yp.detach().cpu(), y) and torch.equal(xg.grad.cpu(), dx)


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("same-")])
def test_tf_same_matches_reference_everywhere(name):
    from mifx.ops.pool import max_pool3s2_same

    x, pt, pl, OH, OW, relu, dy = CASES[name]
    y, _, dx = check_case(x, pt, pl, OH, OW, relu, dy)
    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    yp = max_pool3s2_same(xg, relu=relu)
    assert yp is not None and yp.shape == y.shape
    yp.backward(dy.cuda())
    assert torch.equal(yp.detach().cpu(), y) and torch.equal(xg.grad.cpu(), dx)


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("direct-")])
def test_direct_entry_paddings_match_reference_everywhere(name):
    check_case(*CASES[name])


def test_uncovered_rows_get_zero_gradient():
    """Fewer windows than the image allows: pixels in no window receive exactly 0."""
    x = R.pool_planes(2, 8, 7, 7, seed=3)
    _, _, dx = check_case(x, 1, 0, 2, 2, False, R.pool_dy((2, 8, 2, 2), 4))
    assert not dx[:, :, 4:, :].any() and not dx[:, :, :, 5:].any()


def test_entry_point_refusals():
    from mifx.ops._lib import ptr, stream_handle
    from mifx.ops.pool import _fns

    x = torch.zeros(1, 16, 5, 5, device="cuda", dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y = torch.zeros(1, 16, 8, 8, device="cuda", dtype=torch.bfloat16)
    idx = torch.zeros(1, 8, 8, 16, device="cuda", dtype=torch.uint8)
    st = stream_handle(x.device)

    def fwd(C=16, pt=1, pl=1, OH=3, OW=3):
        return _fns()["fwd"](ptr(x), 1, 5, 5, C, pt, pl, OH, OW, 0, ptr(y), ptr(idx), st)

    def bwd(C=16, pt=1, pl=1):
        return _fns()["bwd"](ptr(y), ptr(idx), 1, 5, 5, C, pt, pl, 3, 3, ptr(x), st)

    assert fwd() == 0 and bwd() == 0
    assert fwd(C=12) == -1 and bwd(C=12) == -1  # C % 8
    assert fwd(pt=3) == -1 and fwd(pl=3) == -1 and bwd(pt=3) == -1 and bwd(pl=3) == -1
    assert fwd(pt=-1) == -1
    assert fwd(OH=4) == -1 and fwd(OW=4) == -1  # last window starts at row 2 * 3 - 1 = 5 >= H: no image tap
    assert fwd(pt=2, OH=4) == 0 and fwd(pt=0, OH=3) == 0 and fwd(pt=0, OH=4) == -1
    torch.cuda.synchronize()


def _plane(vals, C=8, N=1):
    t = torch.tensor(vals, dtype=torch.float32)
    return t.expand(N, C, *t.shape).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (4, 6), (5, 7)])
def test_constant_plane_routes_to_first_in_image_tap(H, W):
    """Every window is one big tie: position and gradient go to its first in-image tap in window order."""
    x = torch.full((2, 8, H, W), 3.0).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = R.pool_dy((2, 8, OH, OW), 9)
    _, pos, dx = check_case(x, 1, 1, OH, OW, False, dy)
    want = torch.tensor([[(1 if oh == 0 else 0) * 3 + (1 if ow == 0 else 0) for ow in range(OW)] for oh in range(OH)])
    assert torch.equal(pos[0, :, :, 0].long(), want)
    (OHs, pt), (OWs, pl) = R.same_pads(H), R.same_pads(W)
    check_case(x, pt, pl, OHs, OWs, True, R.pool_dy((2, 8, OHs, OWs), 10))


def test_two_equal_maxima_keep_the_first():
    x = _plane([[1, 9, 2, 0, 7],
                [9, 3, 9, 7, 1],
                [0, 9, 4, 5, 7],
                [6, 6, 6, 6, 6],
                [8, 2, 8, 2, 8]], C=24, N=2)
    for pt, pl in ((1, 1), (0, 0), (2, 1)):
        OH, OW = R.max_out(5, pt), R.max_out(5, pl)
        _, pos, dx = check_case(x, pt, pl, OH, OW, False, R.pool_dy((2, 24, OH, OW), 11 + pt))
    _, pos, dx = check_case(x, 0, 0, 2, 2, False, torch.ones(2, 24, 2, 2))
    # window (0,0): the 9 at tap 1 before those at taps 3, 5, 7; (1,1): the 8 at tap 6 before the one at tap 8
    assert pos[0, :, :, 0].tolist() == [[1, 3], [1, 6]]
    assert dx[0, 0, 0, 1] == 1 and dx[0, 0, 1, 0] == 0 and dx[0, 0, 4, 2] == 1 and dx[0, 0, 4, 4] == 0


def test_nan_last_wins_and_relu_window_is_dead():
    x = R.pool_planes(1, 8, 6, 6, seed=12).float()
    x[0, :, 1, 1] = NAN
    x[0, :, 1, 2] = NAN
    x[0, :, 2, 1] = NAN
    x[0, :4, 4, 3] = NAN
    x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = R.pool_dy((1, 8, 3, 3), 13)
    y, pos, dx = check_case(x, 1, 1, 3, 3, False, dy)
    assert y[0, :, 0, 0].isnan().all()
    # the last NaN in window order: (0,0) holds one, (0,1) two (taps 6, 7), (1,0) two (2, 5), (1,1) three (0, 1, 3)
    assert pos[0, :2, :2, 0].tolist() == [[8, 7], [5, 3]]
    assert (dx[0, :, 2, 1].float() == dy[0, :, 1, 0].float() + dy[0, :, 1, 1].float()).all()
    y, pos, dx = check_case(x, 1, 1, 3, 3, True, dy)
    assert y[0, :, 0, 0].isnan().all() and (pos[0, 0, 0] == R.NONE).all()
    assert not dx[0, :, 1, 1].any() and not dx[0, :, 1, 2].any() and not dx[0, :, 2, 1].any()
    (OH, pt), (OW, pl) = R.same_pads(6), R.same_pads(6)
    check_case(x, pt, pl, OH, OW, True, dy)
    check_case(x, pt, pl, OH, OW, False, dy)


def test_all_minus_inf_plane_and_negative_relu_windows():
    x = R.pool_planes(2, 8, 5, 7, seed=14).float()
    x[0, 0] = -INF
    x[1, 3, :2] = -INF
    x[1, 4] = -x[1, 4].abs() - 1  # all negative: every relu window is dead
    x[1, 5] = 0.0  # max exactly 0 is not > 0
    x = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    dy = R.pool_dy((2, 8, 3, 4), 15)
    y, pos, dx = check_case(x, 1, 1, 3, 4, False, dy)
    assert (y[0, 0] == -INF).all()
    assert pos[0, :, :, 0].tolist() == [[4, 3, 3, 3], [1, 0, 0, 0], [1, 0, 0, 0]]
    (OH, pt), (OW, pl) = R.same_pads(5), R.same_pads(7)
    y, pos, dx = check_case(x, pt, pl, OH, OW, True, R.pool_dy((2, 8, OH, OW), 16))
    for n, c in ((0, 0), (1, 4), (1, 5)):
        assert (y[n, c] == 0).all() and (pos[n, :, :, c] == R.NONE).all() and not dx[n, c].any()
