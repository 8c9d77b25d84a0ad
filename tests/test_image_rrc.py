"""Random-resized-crop / eval-resize input path (csrc/image_ops.hip rrc_boxes + resample_flip_norm,
mifx.ops.image_ops.random_resized_crop_normalize): the device sampler against its host twin, the resample against
an fp64 reference written out here and against F.interpolate, the identity box against the existing crop kernel,
and the trainer / Transform / pipeline options on top."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mifx.ops import image_ops as io
from mifx.ops.image_ops import (center_box, crop_flip_normalize, crop_params, random_resized_crop_normalize,
                                rrc_params)

ROOT = os.path.dirname(os.path.dirname(__file__))
MEAN, STD = io.IMAGENET_MEAN, io.IMAGENET_STD


# ---------------------------------------------------------------------------------------------- references
def _axis64(n_in: int, n_out: int, flip: bool = False):
    """Taps of one axis in integers (half-pixel centres, clamped inside the box): i0, i1, exact fp64 fraction."""
    o = np.arange(n_out, dtype=np.int64)
    if flip:
        o = n_out - 1 - o
    num, den = (2 * o + 1) * n_in - n_out, 2 * n_out
    i = num // den  # floor
    frac = np.where(i < 0, 0.0, (num - i * den) / float(den))
    return np.clip(i, 0, n_in - 1), np.clip(i + 1, 0, n_in - 1), frac


def _ref64(images: torch.Tensor, idx, boxes, out_hw, mean=MEAN, std=STD) -> np.ndarray:
    """fp64 [B, Hout, Wout, C]: bilinear resample of each box, flip, then (v / 255 - mean32) * inv_std32 with the
    fp32-rounded constants the kernel receives."""
    im = images.numpy().astype(np.float64)
    m32 = np.asarray(mean, np.float32).astype(np.float64)
    inv32 = (np.float32(1.0) / np.asarray(std, np.float32)).astype(np.float64)
    Hout, Wout = out_hw
    out = []
    for b, (x0, y0, w, h, flip) in enumerate(np.asarray(boxes).tolist()):
        r0, r1, fy = _axis64(h, Hout)
        c0, c1, fx = _axis64(w, Wout, bool(flip))
        src = im[int(idx[b]), y0:y0 + h, x0:x0 + w]
        fx_, fy_ = fx[None, :, None], fy[:, None, None]
        top = src[r0][:, c0] * (1 - fx_) + src[r0][:, c1] * fx_
        bot = src[r1][:, c0] * (1 - fx_) + src[r1][:, c1] * fx_
        out.append(((top * (1 - fy_) + bot * fy_) / 255.0 - m32) * inv32)
    return np.stack(out)


def _interp64(images, idx, boxes, out_hw, mean=MEAN, std=STD) -> np.ndarray:
    """The same through F.interpolate in fp64 on the cropped tensor."""
    m32 = torch.tensor(mean, dtype=torch.float32).double()
    inv32 = (1.0 / torch.tensor(std, dtype=torch.float32)).double()
    out = []
    for b, (x0, y0, w, h, flip) in enumerate(np.asarray(boxes).tolist()):
        crop = images[int(idx[b]), y0:y0 + h, x0:x0 + w].double().permute(2, 0, 1)[None] / 255.0
        r = F.interpolate(crop, size=out_hw, mode="bilinear", align_corners=False, antialias=False)[0]
        r = r.permute(1, 2, 0)
        if flip:
            r = r.flip(1)
        out.append(((r - m32) * inv32).numpy())
    return np.stack(out)


def _bounds(ref: np.ndarray, std, dtype):
    """fp32: 2^-19 max(1 / std) (32 roundings of 2^-24 at the scale of 1 / std: about a dozen happen, fractions are
    exact); bf16: one round-to-nearest to 8 significant bits on top, 2^-8 |ref|."""
    b32 = 2.0 ** -19 * float(np.max(1.0 / np.asarray(std, np.float64)))
    return b32 if dtype == torch.float32 else 2.0 ** -8 * np.abs(ref) + b32


def _assert_close(x: torch.Tensor, ref: np.ndarray, std, dtype, what=""):
    d = x.permute(0, 2, 3, 1).double().cpu().numpy()
    err = np.abs(d - ref)
    bound = _bounds(ref, std, dtype)
    print(f"{what} {dtype}: max err {err.max():.3e}, max err / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), f"{what}: max err / bound {np.max(err / bound):.3f}"


# ---------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def draws():
    return rrc_params(200000, 256, 256, seed=7, step=3)


def test_sampler_twin_properties(draws):
    x0, y0, w, h, flip = draws
    H = W = 256
    slo, shi = io.RRC_SCALE
    rlo, rhi = io.RRC_RATIO
    assert ((x0 >= 0) & (y0 >= 0) & (w >= 1) & (h >= 1) & (x0 + w <= W) & (y0 + h <= H)).all()
    # the fallback at the defaults on a square image is the whole image (its ratio 1 is inside the range); counting
    # every whole-image box bounds its share from above
    assert ((w == W) & (h == H)).mean() < 1e-3
    wa, ha = w.astype(np.float64), h.astype(np.float64)
    # w = round(sqrt(area q)), h = round(sqrt(area / q)): each side within half a pixel of its real value; eps for
    # the fp32 roundings of area and q (the whole image satisfies both as well)
    eps = 1e-6
    assert ((wa + 0.5) * (ha + 0.5) >= slo * H * W * (1 - eps)).all()
    assert ((wa - 0.5) * (ha - 0.5) <= shi * H * W * (1 + eps)).all()
    assert ((wa + 0.5) / (ha - 0.5) >= rlo * (1 - eps)).all() and ((wa - 0.5) / (ha + 0.5) <= rhi * (1 + eps)).all()
    assert abs((w < h).mean() - 0.5) <= 0.02 and abs((w > h).mean() - 0.5) <= 0.02
    assert set(np.unique(flip)) == {0, 1}
    small = [np.stack(rrc_params(64, 256, 256, seed=s, step=t)) for s, t in ((7, 3), (7, 3), (7, 4), (8, 3))]
    assert np.array_equal(small[0], small[1])
    assert not np.array_equal(small[0][:4], small[2][:4]) and not np.array_equal(small[0][:4], small[3][:4])
    assert np.array_equal(small[0], np.stack(draws)[:, :64])
    for s, t in ((7, 3), (1 << 40 | 5, 2 ** 31 + 9)):
        assert np.array_equal(rrc_params(512, 256, 256, seed=s, step=t)[4],
                              crop_params(512, 256, 256, 224, 224, True, s, t)[2])


def test_sampler_fallback():
    x0, y0, w, h, _ = rrc_params(33, 40, 48, seed=2, step=5, scale=(1, 1), ratio=(1, 1))
    assert (x0 == 4).all() and (y0 == 0).all() and (w == 40).all() and (h == 40).all()
    x0, y0, w, h, _ = rrc_params(5, 48, 40, seed=2, step=5, scale=(1, 1), ratio=(1, 1))  # portrait image
    assert (x0 == 0).all() and (y0 == 4).all() and (w == 40).all() and (h == 40).all()
    for bad in (dict(scale=(0.0, 1.0)), dict(scale=(0.5, 0.4)), dict(scale=(0.5, 1.5)), dict(ratio=(1.1, 1.3)),
                dict(ratio=(0.5, 0.9))):
        with pytest.raises(ValueError):
            rrc_params(4, 40, 48, **bad)


@pytest.fixture(scope="module")
def small_set():
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, 256, (4, 40, 48, 3), dtype=torch.uint8, generator=g), torch.tensor([2, 0, 3, 1, 2, 0])


@pytest.mark.parametrize("out_hw", [(32, 32), (7, 5)])
def test_resample_semantics_cpu(small_set, out_hw):
    imgs, idx = small_set
    Hout, Wout = out_hw
    boxes = np.array([[5, 7, 1, 1, 0], [0, 0, 48, 40, 0], [0, 0, 48, 40, 1], [3, 2, Wout, Hout, 0],
                      [16, 8, Wout, Hout, 1], [10, 4, 20, 30, 1]])
    ref = _ref64(imgs, idx, boxes, out_hw)
    np.testing.assert_allclose(ref, _interp64(imgs, idx, boxes, out_hw), rtol=0, atol=1e-12)
    x = random_resized_crop_normalize(imgs, idx, out_hw, boxes=torch.from_numpy(boxes), dtype=torch.float32)
    assert x.shape == (6, 3, Hout, Wout)
    _assert_close(x, ref, STD, torch.float32, "cpu op")
    xb = random_resized_crop_normalize(imgs, idx, out_hw, boxes=torch.from_numpy(boxes), dtype=torch.bfloat16)
    _assert_close(xb, ref, STD, torch.bfloat16, "cpu op")
    # flipped = mirrored (box 2 is box 1 flipped)
    assert torch.equal(x[2], random_resized_crop_normalize(imgs, idx[2:3], out_hw, boxes=torch.from_numpy(boxes[1:2]),
                                                           dtype=torch.float32)[0].flip(2))
    # a box of the output size = crop_flip_normalize's pixels, exactly
    for b in (3, 4):
        crop = imgs[idx[b], boxes[b, 1]:boxes[b, 1] + Hout, boxes[b, 0]:boxes[b, 0] + Wout].float() / 255.0
        if boxes[b, 4]:
            crop = crop.flip(1)
        assert torch.equal(x[b].permute(1, 2, 0), (crop - torch.tensor(MEAN)) / torch.tensor(STD))


def test_identity_boxes_equal_crop_op_cpu(small_set):
    imgs, idx = small_set
    oy, ox, flip = crop_params(6, 40, 48, 32, 32, True, 5, 9)
    table = torch.from_numpy(np.stack([ox, oy, np.full(6, 32), np.full(6, 32), flip], 1))
    for dtype in (torch.float32, torch.bfloat16):
        assert torch.equal(random_resized_crop_normalize(imgs, idx, (32, 32), boxes=table, dtype=dtype),
                           crop_flip_normalize(imgs, idx, (32, 32), True, 5, 9, dtype=dtype))


def test_train_op_uses_twin_boxes_cpu(small_set):
    imgs, idx = small_set
    x, table = random_resized_crop_normalize(imgs, idx, (32, 32), True, 3, 11, dtype=torch.float32, return_boxes=True)
    want = np.stack(rrc_params(6, 40, 48, 3, 11), 1)
    assert np.array_equal(table.numpy(), want)
    _assert_close(x, _ref64(imgs, idx, want, (32, 32)), STD, torch.float32, "cpu train")
    y = random_resized_crop_normalize(imgs, idx, (32, 32), True, 3, 0, dtype=torch.float32,
                                      step_dev=torch.tensor([11]))
    assert torch.equal(x, y)


def test_center_box_and_eval():
    assert center_box(40, 48, (32, 32), 36) == (6, 2, 36, 36, 0)
    assert center_box(40, 48, (32, 32)) == (8, 4, 32, 32, 0)
    assert center_box(40, 48, (32, 32), 32) == (4, 0, 40, 40, 0)
    assert center_box(40, 48, (16, 32), 32) == (4, 10, 40, 20, 0)  # the rectangle of the output's aspect ratio
    assert center_box(256, 256, (224, 224), 256) == (16, 16, 224, 224, 0)
    from mifx.trainer.resnet_trainer import ResNetTrainer

    g = torch.Generator().manual_seed(4)
    imgs = torch.randint(0, 256, (12, 40, 48, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 5, (12,), generator=g)
    idx = torch.arange(12)
    x = random_resized_crop_normalize(imgs, idx, (32, 32), False, dtype=torch.float32, eval_resize=36)
    _assert_close(x, _ref64(imgs, idx, [[6, 2, 36, 36, 0]] * 12, (32, 32)), STD, torch.float32, "cpu eval")
    assert torch.equal(random_resized_crop_normalize(imgs, idx, (32, 32), False, dtype=torch.float32),
                       crop_flip_normalize(imgs, idx, (32, 32), False, dtype=torch.float32))
    with pytest.raises(ValueError):
        random_resized_crop_normalize(imgs, idx, (32, 32), False, eval_resize=31)

    def acc(**kw):
        torch.manual_seed(0)
        tr = ResNetTrainer(4, "cpu", imgs, labels, num_classes=5, warmup_steps=2, crop=32, **kw)
        seen = []
        orig = tr.model.forward
        tr.model.forward = lambda x: (seen.append(x.clone()), orig(x))[1]
        a = tr.evaluate(imgs, labels, batch=8)
        return a, torch.cat(seen)

    a0, x0 = acc()
    a1, x1 = acc(augment="random_resized_crop")  # eval_resize=None: today's eval input through the new op
    a2, x2 = acc(eval_resize=36)
    assert torch.equal(x0, x1) and a0 == a1 and 0.0 <= a2 <= 1.0
    assert torch.equal(x0, crop_flip_normalize(imgs, idx, (32, 32), False, dtype=torch.float32))
    assert torch.equal(x2, x) and not torch.equal(x2, x0)


def test_trainer_resume_default_path_and_validation(tmp_path, monkeypatch):
    from mifx.trainer import resnet_trainer as rt

    imgs, labels = rt.synthetic_imagenet(40, 40, 5, seed=3)

    def make(**kw):
        return rt.ResNetTrainer(4, "cpu", imgs, labels, num_classes=5, warmup_steps=2, crop=32, **kw)

    calls = {"crop": 0, "rrc": 0}

    def spy(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f

    monkeypatch.setattr(rt, "crop_flip_normalize", spy("crop", rt.crop_flip_normalize))
    monkeypatch.setattr(rt, "random_resized_crop_normalize", spy("rrc", rt.random_resized_crop_normalize))
    d = make()
    d.step()
    d.evaluate(imgs[:4], labels[:4])
    assert calls == {"crop": 2, "rrc": 0} and d.input_recipe()["augment"] == "none"

    kw = dict(augment="random_resized_crop", rrc_scale=(0.25, 1.0))
    a = make(**kw)
    for _ in range(4):
        a.step()
    assert calls == {"crop": 2, "rrc": 4}
    b = make(**kw)
    for _ in range(2):
        b.step()
    path = b.save_checkpoint(str(tmp_path / "ck"))
    c = make(**kw)
    c.restore(path)
    assert c.step_idx == 2
    for _ in range(2):
        c.step()
    sa, sc = a.state_dict(), c.state_dict()
    assert set(sa) == set(sc)
    for k in sa:
        torch.testing.assert_close(sc[k], sa[k], rtol=0, atol=0, msg=k)
    # the augmentation changes what is trained on
    e, d2 = make(**kw), make()
    assert float(e.step()) != float(d2.step())
    for bad in (dict(augment="random_resized_crop", rrc_scale=(0.0, 1.0)),
                dict(augment="random_resized_crop", rrc_scale=(0.6, 0.5)),
                dict(augment="random_resized_crop", rrc_scale=(0.5, 1.1)),
                dict(augment="random_resized_crop", rrc_ratio=(1.2, 1.5)),
                dict(augment="random_resized_crop", rrc_ratio=(0.5, 0.9)),
                dict(eval_resize=31), dict(rrc_scale=(0.3, 1.0)), dict(rrc_ratio=(0.5, 2.0)), dict(augment="mixup")):
        with pytest.raises(ValueError):
            make(**bad)


def _pipe():
    spec = importlib.util.spec_from_file_location("rp", os.path.join(ROOT, "examples/image/resnet_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_pipeline_records_input_recipe(tmp_path):
    from mifx.orchestration import LocalDagRunner

    def run(name, augment):
        p = _pipe().create_pipeline(str(tmp_path / name), 48, 40, 32, 5, 2, 4, name=name, augment=augment)
        res = LocalDagRunner(device="cpu").run(p)
        assert res.succeeded
        tf = res.components["ImageTransform"].outputs["transform_output"][0]
        out = res.components["ImageTrainer"].outputs["output"][0]
        with open(os.path.join(tf.uri, "image_transform.json")) as f:
            tfj = json.load(f)
        with open(os.path.join(out.uri, "metrics.json")) as f:
            return tfj, json.load(f), out.custom_properties

    tf0, m0, p0 = run("plain", None)
    assert set(tf0) == {"mean", "std", "crop"}  # a Transform without the options writes what it wrote before
    assert m0["input"] == {"augment": "none", "rrc_scale": [0.08, 1.0], "rrc_ratio": [0.75, 4.0 / 3.0],
                           "eval_resize": None}
    assert p0["input_augment"] == "none" and "input_eval_resize" not in p0
    tf1, m1, p1 = run("rrc", {"augment": "random_resized_crop", "rrc_scale": (0.25, 1.0), "eval_resize": 36})
    assert tf1["augment"] == "random_resized_crop" and tf1["rrc_scale"] == [0.25, 1.0] and tf1["eval_resize"] == 36
    assert "rrc_ratio" not in tf1
    assert m1["input"] == {"augment": "random_resized_crop", "rrc_scale": [0.25, 1.0],
                           "rrc_ratio": [0.75, 4.0 / 3.0], "eval_resize": 36}
    assert p1["input_augment"] == "random_resized_crop" and p1["input_rrc_scale_lo"] == 0.25
    assert p1["input_rrc_ratio_hi"] == pytest.approx(4.0 / 3.0) and p1["input_eval_resize"] == 36
    drop = lambda d: {k: v for k, v in d.items() if k != "final_lr"}  # noqa: E731
    assert drop(m1["optimizer"]) == drop(m0["optimizer"]) and "augment" not in m1["optimizer"]
    assert np.isfinite(m1["final_loss"]) and m1["final_loss"] != m0["final_loss"]


# ---------------------------------------------------------------------------------------------- GPU
def _device_boxes(B, Hin, Win, seed, step, step_dev=None, **kw):
    imgs = torch.zeros(1, Hin, Win, 1, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(B, dtype=torch.int64, device="cuda")
    _, table = random_resized_crop_normalize(imgs, idx, (4, 4), True, seed, step, mean=(0,), std=(1,),
                                             dtype=torch.float32, step_dev=step_dev, return_boxes=True, **kw)
    return table


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(64, 72), (17, 23), (256, 256)])
def test_boxes_device_equals_twin(hw):
    Hin, Win = hw
    seed = (1 << 33) | 12345
    got = torch.stack([_device_boxes(64, Hin, Win, seed, s) for s in range(64)]).cpu().numpy()
    want = np.stack([np.stack(rrc_params(64, Hin, Win, seed, s), 1) for s in range(64)])
    bad = np.nonzero((got != want).any(-1))
    assert got.shape == (64, 64, 5) and bad[0].size == 0, (bad, got[bad][:4], want[bad][:4])
    dev = _device_boxes(64, Hin, Win, seed, 0, step_dev=torch.tensor([11], device="cuda"))
    assert np.array_equal(dev.cpu().numpy(), want[11])


@pytest.mark.gpu
def test_boxes_device_fallback():
    got = _device_boxes(64, 40, 48, 5, 3, scale=(1, 1), ratio=(1, 1)).cpu().numpy()
    assert (got[:, :4] == np.array([4, 0, 40, 40])).all()
    assert np.array_equal(got, np.stack(rrc_params(64, 40, 48, 5, 3, (1, 1), (1, 1)), 1))


@pytest.fixture(scope="module")
def gpu_set():
    out = {}
    g = torch.Generator().manual_seed(5)
    for C in (1, 3, 4):
        out[C] = torch.randint(0, 256, (16, 64, 72, C), dtype=torch.uint8, generator=g)
    return out, torch.randint(0, 16, (9,), generator=g)


def _hand_boxes(out_hw):
    Hout, Wout = out_hw
    return np.array([[5, 7, 1, 1, 0], [71, 63, 1, 1, 1], [0, 0, 72, 64, 0], [0, 0, 72, 64, 1],
                     [72 - 31, 64 - 17, 31, 17, 0], [72 - Wout, 64 - Hout, Wout, Hout, 1], [3, 1, 13, 50, 1],
                     [1, 2, 70, 3, 0], [70, 0, 2, 64, 1]])


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("out_hw", [(56, 56), (32, 40), (33, 35)])
def test_resample_device_vs_fp64(gpu_set, C, out_hw):
    sets, idx = gpu_set
    imgs = sets[C]
    mean, std = MEAN[:C] if C <= 3 else MEAN + (0.5,), STD[:C] if C <= 3 else STD + (0.25,)
    dimgs, didx = imgs.cuda(), idx.cuda()
    for dtype in (torch.float32, torch.bfloat16):
        x, table = random_resized_crop_normalize(dimgs, didx, out_hw, True, 3, 11, mean, std, dtype,
                                                 return_boxes=True)
        assert x.shape == (9, C, *out_hw) and x.permute(0, 2, 3, 1).is_contiguous()
        assert x.is_contiguous(memory_format=torch.channels_last) or C == 1
        table = table.cpu().numpy()
        assert np.array_equal(table, np.stack(rrc_params(9, 64, 72, 3, 11), 1))
        _assert_close(x, _ref64(imgs, idx, table, out_hw, mean, std), std, dtype, f"sampled C={C} {out_hw}")
        hand = _hand_boxes(out_hw)
        x = random_resized_crop_normalize(dimgs, didx, out_hw, boxes=torch.from_numpy(hand), mean=mean, std=std,
                                          dtype=dtype)
        _assert_close(x, _ref64(imgs, idx, hand, out_hw, mean, std), std, dtype, f"hand C={C} {out_hw}")


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 3, 4])
def test_identity_boxes_equal_crop_kernel(gpu_set, C):
    sets, idx = gpu_set
    dimgs, didx = sets[C].cuda(), idx.cuda()
    mean, std = MEAN[:C] if C <= 3 else MEAN + (0.5,), STD[:C] if C <= 3 else STD + (0.25,)
    for out_hw in ((56, 56), (33, 35)):
        oy, ox, flip = crop_params(9, 64, 72, *out_hw, True, 3, 11)
        table = torch.from_numpy(np.stack([ox, oy, np.full(9, out_hw[1]), np.full(9, out_hw[0]), flip], 1))
        for dtype in (torch.float32, torch.bfloat16):
            a = random_resized_crop_normalize(dimgs, didx, out_hw, boxes=table, mean=mean, std=std, dtype=dtype)
            b = crop_flip_normalize(dimgs, didx, out_hw, True, 3, 11, mean, std, dtype)
            assert torch.equal(a, b), (C, out_hw, dtype)
        a = random_resized_crop_normalize(dimgs, didx, out_hw, False, mean=mean, std=std)  # eval, no resize
        assert torch.equal(a, crop_flip_normalize(dimgs, didx, out_hw, False, mean=mean, std=std))


@pytest.mark.gpu
def test_device_vs_cpu_op(gpu_set):
    sets, idx = gpu_set
    imgs = sets[3]
    for dtype in (torch.float32, torch.bfloat16):
        for kw in (dict(train=True, seed=3, step=11), dict(train=False, eval_resize=60)):
            h = random_resized_crop_normalize(imgs, idx, (56, 56), dtype=torch.float32, **kw)
            d = random_resized_crop_normalize(imgs.cuda(), idx.cuda(), (56, 56), dtype=dtype, **kw)
            assert d.is_contiguous(memory_format=torch.channels_last)
            _assert_close(d, h.permute(0, 2, 3, 1).double().numpy(), STD, dtype, f"gpu vs cpu {kw}")
    box = center_box(64, 72, (56, 56), 60)
    d = random_resized_crop_normalize(imgs.cuda(), idx.cuda(), (56, 56), False, dtype=torch.float32, eval_resize=60)
    _assert_close(d, _ref64(imgs, idx, [list(box)] * 9, (56, 56)), STD, torch.float32, "eval vs fp64")


@pytest.mark.gpu
def test_trainer_gpu_graph_replay_input(monkeypatch):
    from mifx.trainer.resnet_trainer import ResNetTrainer, synthetic_imagenet

    imgs, labels = synthetic_imagenet(64, 72, 10, device="cuda")
    tr = ResNetTrainer(6, "cuda", imgs, labels, num_classes=10, crop=64, warmup_steps=2,
                       augment="random_resized_crop", eval_resize=70)
    # MIOpen's deterministic solvers, no solver search: these are the convolution shapes of
    # test_parallel_gpu.test_resnet_captured_step_matches_eager, which runs later in the same process and needs
    # bit-reproducible convolutions; a search here would leave its (not reproducible) choices cached for them
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    seen = []
    orig = tr._train_input
    tr._train_input = lambda *a, **k: (seen.append(orig(*a, **k)), seen[-1])[1]
    losses = [float(tr.step()) for _ in range(tr.graph_warmup + 2)]
    assert all(np.isfinite(losses)) and tr._gA is not None
    s = tr.step_idx - 1  # the last step was a replay: the graph's input tensor holds what it trained on
    assert len(seen) == tr.graph_warmup + 1 and int(tr._step_dev) == s
    want = random_resized_crop_normalize(tr.images, tr._idx_dev[:6], (64, 64), True, tr.seed, s, tr.mean, tr.std,
                                         torch.bfloat16)
    assert torch.equal(seen[-1], want)
    prev = random_resized_crop_normalize(tr.images, tr._idx_dev[:6], (64, 64), True, tr.seed, s - 1, tr.mean, tr.std,
                                         torch.bfloat16)
    assert not torch.equal(want, prev)
    a = tr.evaluate(imgs[:32], labels[:32])
    assert 0.0 <= a <= 1.0
