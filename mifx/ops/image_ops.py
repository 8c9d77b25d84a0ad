"""Fused crop + flip + normalize for HBM-resident uint8 image datasets (csrc/image_ops.hip).

The host reference reproduces the device Philox stream bit-exactly (mifx.ops.dp.philox4x32), so
CPU and GPU augmentations pick the same crops and flips.

`random_resized_crop_normalize` adds scale + aspect-ratio augmentation (a random box covering `scale` of the image
at an aspect ratio in `ratio`, resized bilinearly to the output) and resize-then-centre-crop evaluation. Its boxes
come from `rrc_params`, the bit-exact host twin of the device sampler. Unlike torchvision's RandomResizedCrop, which
draws the aspect ratio log-uniformly (exp of a uniform logarithm), the ratio is drawn "mirrored": a fair bit picks
landscape or portrait, and the long/short ratio q is uniform in [1, ratio_hi] or [1, 1 / ratio_lo]. That keeps the
w <-> h symmetry of the log-uniform draw but needs only + - * / sqrt, which round identically on the host and the
device; exp / log do not, and a last-bit difference can flip a rounded width."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import F32, I32, VP, check, ptr, sig, stream_handle

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("image_ops")
    return {"cfn": sig(lib, "mifx_img_crop_flip_norm", [VP, VP, I32, I32, I32, I32, I32, I32, I32, ctypes.c_ulonglong,
                                                         ctypes.c_uint, VP, VP, VP, I32, VP, VP]),
            "boxes": sig(lib, "mifx_img_rrc_boxes", [I32, I32, I32, ctypes.c_ulonglong, ctypes.c_uint, VP, F32, F32,
                                                     F32, F32, VP, VP]),
            "resample": sig(lib, "mifx_img_resample_flip_norm", [VP, VP, VP, I32, I32, I32, I32, I32, I32, I32, I32,
                                                                 VP, VP, I32, VP, VP])}


@functools.lru_cache(maxsize=64)
def _norm_consts(device: str, mean: tuple, std: tuple):
    """Device mean / 1/std (cached: no host-to-device copy per call, so the call can be captured in a hipGraph)."""
    m = torch.tensor(mean, device=device, dtype=torch.float32)
    return m, 1.0 / torch.tensor(std, device=device, dtype=torch.float32)


def crop_params(B: int, Hin: int, Win: int, Hout: int, Wout: int, train: bool, seed: int, step: int):
    if not train:
        z = np.zeros(B, np.int64)
        return z + (Hin - Hout) // 2, z + (Win - Wout) // 2, z
    from .dp import philox4x32

    x, y, zz, _ = philox4x32(np.arange(B, dtype=np.uint32), step & 0xFFFFFFFF, 0x1234, 0, seed)
    return (x % np.uint32(Hin - Hout + 1)).astype(np.int64), (y % np.uint32(Win - Wout + 1)).astype(np.int64), \
        (zz & np.uint32(1)).astype(np.int64)


def crop_flip_normalize(images: torch.Tensor, idx: torch.Tensor, out_hw=(224, 224), train: bool = True,
                        seed: int = 0, step: int = 0, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                        dtype=torch.bfloat16, step_dev: torch.Tensor | None = None) -> torch.Tensor:
    """images uint8 [N, H, W, C]; idx [B] -> [B, C, Hout, Wout] in channels_last memory format. step_dev (GPU): a
    device int64 [1] step counter the kernel reads instead of `step` (for steps captured into a hipGraph)."""
    N, Hin, Win, C = images.shape
    Hout, Wout = out_hw
    B = int(idx.numel())
    if images.is_cuda:
        out = torch.empty(B, Hout, Wout, C, device=images.device, dtype=dtype)
        m, inv = _norm_consts(str(images.device), tuple(float(v) for v in mean), tuple(float(v) for v in std))
        idx32 = idx.to(device=images.device, dtype=torch.int32).contiguous()
        if step_dev is not None and (step_dev.dtype != torch.int64 or step_dev.device != images.device):
            raise ValueError("step_dev must be an int64 tensor on the images' device")
        check(_fns()["cfn"](ptr(images), ptr(idx32), B, Hin, Win, C, Hout, Wout, int(train), seed, step,
                            ptr(step_dev), ptr(m),
                            ptr(inv), 1 if dtype == torch.bfloat16 else 0, ptr(out), stream_handle(images.device)),
              "mifx_img_crop_flip_norm")
        return out.permute(0, 3, 1, 2)  # NCHW view with channels_last strides
    if step_dev is not None:
        step = int(step_dev.reshape(-1)[0])
    oy, ox, flip = crop_params(B, Hin, Win, Hout, Wout, train, seed, step)
    outs = []
    for b in range(B):
        im = images[int(idx[b]), oy[b]:oy[b] + Hout, ox[b]:ox[b] + Wout].float() / 255.0
        if flip[b]:
            im = im.flip(1)
        outs.append(im)
    x = (torch.stack(outs) - torch.tensor(mean)) / torch.tensor(std)
    return x.to(dtype).permute(0, 3, 1, 2)


# ---- random-resized-crop / eval resize -------------------------------------------------------------------------------
RRC_SCALE = (0.08, 1.0)
RRC_RATIO = (3.0 / 4.0, 4.0 / 3.0)


def check_rrc_ranges(scale, ratio) -> None:
    """ValueError unless 0 < scale_lo <= scale_hi <= 1 and 0 < ratio_lo <= 1 <= ratio_hi (the mirrored ratio draw
    needs 1 inside the range)."""
    if len(scale) != 2 or not 0.0 < float(scale[0]) <= float(scale[1]) <= 1.0:
        raise ValueError(f"scale must satisfy 0 < lo <= hi <= 1, got {tuple(scale)}")
    if len(ratio) != 2 or not 0.0 < float(ratio[0]) <= 1.0 <= float(ratio[1]):
        raise ValueError(f"ratio must satisfy 0 < lo <= 1 <= hi, got {tuple(ratio)}")


def rrc_params(B: int, Hin: int, Win: int, seed: int = 0, step: int = 0, scale=RRC_SCALE, ratio=RRC_RATIO):
    """The boxes of the device sampler (rrc_boxes in csrc/image_ops.hip), bit for bit: int64 arrays
    (x0, y0, w, h, flip) for batch slots 0..B-1 at training step `step`. Every fp32 operation is rounded on its own,
    in the device's order."""
    from .dp import philox4x32

    check_rrc_ranges(scale, ratio)
    if Hin * Win > 1 << 24:
        raise ValueError("rrc_params: Hin * Win must not exceed 2^24")
    f32, u32 = np.float32, np.uint32
    slo, shi, rlo, rhi = f32(scale[0]), f32(scale[1]), f32(ratio[0]), f32(ratio[1])
    slot, st = np.arange(B, dtype=u32), step & 0xFFFFFFFF
    full, dscale = f32(Hin * Win), f32(shi - slo)
    qhi, qlo = f32(rhi - f32(1.0)), f32(f32(f32(1.0) / rlo) - f32(1.0))
    u01 = lambda v: (v >> u32(8)).astype(f32) * f32(1.0 / 16777216.0)  # noqa: E731
    rnd = lambda v: (v + f32(0.5)).astype(np.int64)  # noqa: E731  (floor(v + 0.5), v >= 0)
    x0, y0, w, h = (np.zeros(B, np.int64) for _ in range(4))
    todo = np.ones(B, bool)
    for k in range(10):
        if not todo.any():
            break
        b = np.nonzero(todo)[0]
        rx, ry, rz, rw = philox4x32(slot[b], st, 0x1235, k, seed)
        area = (slo + dscale * u01(rx)) * full
        portrait = (ry & u32(1)) != 0
        q = f32(1.0) + np.where(portrait, qlo, qhi).astype(f32) * u01(ry)
        a, c = rnd(np.sqrt(area * q)), rnd(np.sqrt(area / q))
        wk, hk = np.where(portrait, c, a), np.where(portrait, a, c)
        ok = (wk >= 1) & (wk <= Win) & (hk >= 1) & (hk <= Hin)
        g = b[ok]
        w[g], h[g] = wk[ok], hk[ok]
        x0[g] = (rz[ok] % (Win - wk[ok] + 1).astype(u32)).astype(np.int64)
        y0[g] = (rw[ok] % (Hin - hk[ok] + 1).astype(u32)).astype(np.int64)
        todo[g] = False
    if todo.any():  # torchvision's fallback: the central crop, the image's ratio clamped into [ratio_lo, ratio_hi]
        in_ratio = f32(Win) / f32(Hin)
        fw, fh = Win, Hin
        if in_ratio < rlo:
            fh = int(f32(f32(Win) / rlo) + f32(0.5))
        elif in_ratio > rhi:
            fw = int(f32(f32(Hin) * rhi) + f32(0.5))
        fw, fh = min(max(fw, 1), Win), min(max(fh, 1), Hin)
        w[todo], h[todo], x0[todo], y0[todo] = fw, fh, (Win - fw) // 2, (Hin - fh) // 2
    flip = (philox4x32(slot, st, 0x1234, 0, seed)[2] & u32(1)).astype(np.int64)
    return x0, y0, w, h, flip


def center_box(Hin: int, Win: int, out_hw, resize: int | None = None) -> tuple:
    """The eval box (x0, y0, w, h, flip=0): what resize-the-shorter-side-to-`resize`-then-centre-crop-`out_hw` sees
    of the stored image, i.e. the central round(min(H, W) * crop / resize) square (for a rectangular output, the
    rectangle of its aspect ratio), clamped into the image. resize=None: the central out_hw window itself."""
    Hout, Wout = out_hw
    if resize is None:
        w, h = Wout, Hout
    else:
        m, r = min(Hin, Win), int(resize)
        w, h = (2 * Wout * m + r) // (2 * r), (2 * Hout * m + r) // (2 * r)  # round half up, in integers
    w, h = min(max(w, 1), Win), min(max(h, 1), Hin)
    return (Win - w) // 2, (Hin - h) // 2, w, h, 0


@functools.lru_cache(maxsize=64)
def _eval_box_dev(device: str, box: tuple):
    """One eval box on the device (cached like _norm_consts: the eval call stays capturable)."""
    return torch.tensor([box], device=device, dtype=torch.int32)


def _taps(o: torch.Tensor, n_in: torch.Tensor, n_out: int):
    """Bilinear taps along one axis, half-pixel centres, as the kernel splits them: o [B, n_out] output positions,
    n_in [B] box pixels -> (i0, i1 int64 [B, n_out] clamped inside the box, frac fp32)."""
    num = (2 * o + 1) * n_in[:, None] - n_out
    den = 2 * n_out
    i = torch.div(num, den, rounding_mode="floor")
    frac = torch.where(i < 0, torch.zeros((), dtype=torch.float32),
                       (num - i * den).to(torch.float32) / torch.tensor(float(den), dtype=torch.float32))
    hi = (n_in - 1)[:, None]
    return torch.minimum(i.clamp(min=0), hi), torch.minimum((i + 1).clamp(min=0), hi), frac


def _resample_host(images, idx, boxes, out_hw, mean, std, dtype):
    """The resample kernel's semantics in torch fp32 on the host: boxes int64 [B, 5]."""
    Hout, Wout = out_hw
    N, Hin, Win, C = images.shape
    B = boxes.shape[0]
    x0 = boxes[:, 0].clamp(0, Win - 1)
    y0 = boxes[:, 1].clamp(0, Hin - 1)
    w = torch.minimum(boxes[:, 2].clamp(min=1), Win - x0)
    h = torch.minimum(boxes[:, 3].clamp(min=1), Hin - y0)
    flip = (boxes[:, 4] & 1).bool()
    oy = torch.arange(Hout).expand(B, Hout)
    ox = torch.arange(Wout).expand(B, Wout)
    ox = torch.where(flip[:, None], Wout - 1 - ox, ox)
    r0, r1, fy = _taps(oy, h, Hout)
    c0, c1, fx = _taps(ox, w, Wout)
    img = images[idx.long().clamp(0, N - 1)]  # [B, Hin, Win, C] uint8
    bi = torch.arange(B)[:, None, None]
    ya, yb = (y0[:, None] + r0)[:, :, None], (y0[:, None] + r1)[:, :, None]
    xa, xb = (x0[:, None] + c0)[:, None, :], (x0[:, None] + c1)[:, None, :]
    t0, t1, b0, b1 = (img[bi, yy, xx].float() for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))
    fx, fy = fx[:, None, :, None], fy[:, :, None, None]
    tv, bv = t0 + fx * (t1 - t0), b0 + fx * (b1 - b0)
    x = (tv + fy * (bv - tv)) / 255.0
    x = (x - torch.tensor(mean)) / torch.tensor(std)
    return x.to(dtype).permute(0, 3, 1, 2)


def random_resized_crop_normalize(images: torch.Tensor, idx: torch.Tensor, out_hw=(224, 224), train: bool = True,
                                  seed: int = 0, step: int = 0, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                                  dtype=torch.bfloat16, step_dev: torch.Tensor | None = None, scale=RRC_SCALE,
                                  ratio=RRC_RATIO, eval_resize: int | None = None,
                                  boxes: torch.Tensor | None = None, return_boxes: bool = False):
    """images uint8 [N, H, W, C]; idx [B] -> [B, C, Hout, Wout] in channels_last memory format: per image a box
    (x0, y0, w, h, flip) resized to out_hw bilinearly (half-pixel centres, taps clamped inside the box, no
    antialiasing), flipped and normalised as crop_flip_normalize does. A box of exactly the output size gives
    crop_flip_normalize's pixels.

    train=True: the boxes of `rrc_params(B, H, W, seed, step, scale, ratio)`, sampled on the device by the box kernel
    (step_dev as in crop_flip_normalize). train=False: `center_box(H, W, out_hw, eval_resize)` for every image.
    boxes (int [B, 5]): run the resample on this table instead. return_boxes: also return the int32 [B, 5] table."""
    N, Hin, Win, C = images.shape
    Hout, Wout = out_hw
    B = int(idx.numel())
    if boxes is not None and tuple(boxes.shape) != (B, 5):
        raise ValueError(f"boxes must be [{B}, 5], got {tuple(boxes.shape)}")
    if boxes is None and train:
        check_rrc_ranges(scale, ratio)
    if not train and eval_resize is not None and eval_resize < max(Hout, Wout):
        raise ValueError(f"eval_resize {eval_resize} is smaller than the output {tuple(out_hw)}")
    if images.is_cuda:
        dev = images.device
        if not images.is_contiguous() or images.dtype != torch.uint8:
            raise ValueError("images must be a contiguous uint8 [N, H, W, C] tensor")
        if step_dev is not None and (step_dev.dtype != torch.int64 or step_dev.device != dev):
            raise ValueError("step_dev must be an int64 tensor on the images' device")
        fns = _fns()
        stride = 5
        if boxes is not None:
            table = boxes.to(device=dev, dtype=torch.int32).contiguous()
        elif train:
            table = torch.empty(B, 5, device=dev, dtype=torch.int32)
            check(fns["boxes"](B, Hin, Win, seed, step & 0xFFFFFFFF, ptr(step_dev), float(scale[0]), float(scale[1]),
                               float(ratio[0]), float(ratio[1]), ptr(table), stream_handle(dev)),
                  "mifx_img_rrc_boxes")
        else:
            table, stride = _eval_box_dev(str(dev), center_box(Hin, Win, out_hw, eval_resize)), 0
        out = torch.empty(B, Hout, Wout, C, device=dev, dtype=dtype)
        m, inv = _norm_consts(str(dev), tuple(float(v) for v in mean), tuple(float(v) for v in std))
        idx32 = idx.to(device=dev, dtype=torch.int32).contiguous()
        check(fns["resample"](ptr(images), ptr(idx32), ptr(table), stride, N, B, Hin, Win, C, Hout, Wout, ptr(m),
                              ptr(inv), 1 if dtype == torch.bfloat16 else 0, ptr(out), stream_handle(dev)),
              "mifx_img_resample_flip_norm")
        x = out.permute(0, 3, 1, 2)  # NCHW view with channels_last strides
        return (x, table.expand(B, 5) if stride == 0 else table) if return_boxes else x
    if boxes is not None:
        table = boxes.to(torch.int64).cpu()
    elif train:
        if step_dev is not None:
            step = int(step_dev.reshape(-1)[0])
        table = torch.from_numpy(np.stack(rrc_params(B, Hin, Win, seed, step, scale, ratio), axis=1))
    else:
        table = torch.tensor([center_box(Hin, Win, out_hw, eval_resize)], dtype=torch.int64).expand(B, 5)
    x = _resample_host(images, idx.cpu(), table, out_hw, mean, std, dtype)
    return (x, table.to(torch.int32)) if return_boxes else x
