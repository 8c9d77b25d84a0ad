"""ctypes bindings for csrc/wd_general.hip (general fused Wide&Deep step on gfx950: any tower of 1..6 hidden
layers, widths 2..256; geometry and index maps: models.wide_deep.general_layout)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import F32, I32, I64, U64, VP, check, ptr, sig, stream_handle


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("wd_general")
    return {
        "constants": sig(lib, "mifx_wdg_constants", [VP, I32]),
        "fused": sig(lib, "mifx_wdg_fused", [VP, I64, I64, I64, VP, VP, VP, VP, VP, VP, F32, I32, I32, VP, VP, VP,
                                             I64, I64, U64, VP, F32, VP]),
        "reduce_opt": sig(lib, "mifx_wdg_reduce_opt", [VP, I32, I32, VP, VP, VP, VP, VP, VP, I32, VP, VP, VP, VP,
                                                       I32, F32, F32, U64]),
    }


# the kernel's DP_SHRINK, for the hosts without the library (the CPU trainer clips by the same rule)
DP_SHRINK = np.float32((1.0 - 1.0 / 4096.0) / (1.0 + 1.0 / 256.0))

_CONST_NAMES = ["T", "NTHR", "PAD", "MAXH", "MAXW", "KMAX", "NWIDE", "WIDE_BIAS", "WIDE_PAD", "SLOTS",
                "SLAB_BOUND_MB", "DESC_HDR", "DESC_LAYER", "DESC_LEN", "DP_SHRINK_BITS"]


@functools.lru_cache(maxsize=None)
def constants() -> dict[str, int]:
    """Compile-time constants of the kernel, checked against the host's copy of the layout."""
    from ..models import wide_deep as wdm

    buf = (ctypes.c_int * 32)()
    n = _fns()["constants"](buf, 32)
    if n != len(_CONST_NAMES):
        raise RuntimeError(f"general W&D kernel exports {n} constants, expected {len(_CONST_NAMES)}")
    c = {k: buf[i] for i, k in enumerate(_CONST_NAMES)}
    want = {"T": wdm.GEN_T, "PAD": wdm.GEN_PAD, "MAXH": wdm.GEN_MAX_HIDDEN, "MAXW": wdm.GEN_MAX_WIDTH,
            "NWIDE": wdm.NWIDE, "WIDE_PAD": wdm.WIDE_PAD, "DESC_HDR": wdm.GEN_DESC_HDR,
            "DESC_LAYER": wdm.GEN_DESC_LAYER, "DESC_LEN": wdm.GEN_DESC_LEN}
    for k, v in want.items():
        if c[k] != v:
            raise RuntimeError(f"general W&D kernel: {k} = {c[k]}, the host layout has {v}")
    return c


def dp_shrink() -> float:
    """The DP clip shrink s of the kernel (c_i = min(1, s C / n_i)): the fp32 value (1 - 2^-12) / (1 + 2^-8), which
    covers the bf16 rounding of the scaled dZ rows and the fp32 rounding of n_i (derivation: csrc/wd_general.hip)."""
    s = float(np.array([constants()["DP_SHRINK_BITS"]], np.int32).view(np.float32)[0])
    if s != float(DP_SHRINK):
        raise RuntimeError(f"general W&D kernel: DP_SHRINK = {s!r}, the host has {float(DP_SHRINK)!r}")
    return s


def max_grid(stride: int) -> int:
    """Workgroups whose fp32 slabs [grid, stride] stay inside the kernel's slab bound."""
    return max(1, (constants()["SLAB_BOUND_MB"] << 20) // (4 * int(stride)))


def _desc_host(desc: np.ndarray):
    d = np.ascontiguousarray(desc, dtype=np.int32)
    if d.size != constants()["DESC_LEN"]:
        raise ValueError("tower descriptor has the wrong length")
    return d


def fused(records: torch.Tensor, n_data: int, batch: int, start_fixed: int, step_ctr: torch.Tensor | None,
          wimg: torch.Tensor, wide: torch.Tensor, slab: torch.Tensor | None, slab_loss: torch.Tensor | None,
          logits_out: torch.Tensor | None, grad_scale: float, grid: int, train: bool, desc: np.ndarray,
          desc_dev: torch.Tensor, scratch: torch.Tensor | None, scratch_per_wg: int = 0,
          feed: tuple[int, int, int] | None = None, l2_norm_clip: float | None = None,
          norms_out: torch.Tensor | None = None) -> None:
    """One wdg_fused launch. wimg: 16-bit [2 * WTOT] (W^T image, then the transposed one); slab: fp32
    [>= grid, WTOT + WIDE_PAD]; scratch: 16-bit [>= grid * scratch_per_wg]; desc / desc_dev: the layout's
    descriptor on the host and (int32) on the device. feed: (stride, offset, shuffle seed), None = stored order.
    l2_norm_clip (training only): the DP mode, per-example clipping to that L2 norm; norms_out fp32 [>= batch] then
    receives the per-example gradient norms and grad_scale is left to reduce_sum / reduce_apply."""
    d = _desc_host(desc)
    wtot = int(d[2])
    c = constants()
    if records.dim() != 2 or records.shape[1] != 32 or not records.is_contiguous():
        raise ValueError("records must be contiguous uint8 [N, 32]")
    if wimg.numel() != 2 * wtot or wimg.element_size() != 2 or not wimg.is_contiguous():
        raise ValueError("weight image must be a contiguous 16-bit [2 * WTOT] tensor")
    if desc_dev.dtype != torch.int32 or desc_dev.numel() != d.size or wide.numel() < c["NWIDE"]:
        raise ValueError("device descriptor must be int32 [DESC_LEN]; wide weights [>= NWIDE]")
    if grid < 1 or grid > (batch + c["T"] - 1) // c["T"]:
        raise ValueError("grid must be in [1, tiles of the batch]")
    if train:
        stride = wtot + c["WIDE_PAD"]
        if slab is None or slab.dtype != torch.float32 or not slab.is_contiguous() or slab.shape[-1] != stride \
                or slab.shape[0] < grid or grid > max_grid(stride):
            raise ValueError("slab must be contiguous fp32 [>= grid, WTOT + WIDE_PAD] inside the slab bound")
        ksum = sum(int(d[c["DESC_HDR"] + c["DESC_LAYER"] * l]) for l in range(int(d[0])))
        if scratch is None or scratch.element_size() != 2 or scratch.numel() < grid * scratch_per_wg \
                or scratch_per_wg != ksum * c["T"]:
            raise ValueError("scratch must hold grid x (64 x sum K) 16-bit elements")
        if slab_loss is not None and slab_loss.numel() < grid:
            raise ValueError("slab_loss must hold >= grid floats")
        if step_ctr is None or step_ctr.dtype != torch.int64 or step_ctr.numel() < c["SLOTS"]:
            raise ValueError("step_ctr must be int64 [SLOTS]")
        if l2_norm_clip is not None:
            if not float(l2_norm_clip) > 0.0:
                raise ValueError("l2_norm_clip must be > 0")
            if norms_out is None or norms_out.dtype != torch.float32 or norms_out.numel() < batch \
                    or not norms_out.is_contiguous() or norms_out.device != records.device:
                raise ValueError("DP mode needs contiguous fp32 norms_out with >= batch entries on the device")
    elif l2_norm_clip is not None:
        raise ValueError("l2_norm_clip is a training mode")
    elif logits_out is None or logits_out.numel() < batch or logits_out.dtype != torch.float32:
        raise ValueError("eval launch needs fp32 logits_out with >= batch entries")
    gs, go, key = feed if feed is not None else (batch, 0, 0)
    rc = _fns()["fused"](ptr(records), n_data, batch, start_fixed, ptr(step_ctr), ptr(wimg), ptr(wide), ptr(slab),
                         ptr(slab_loss), ptr(logits_out), float(grad_scale), int(grid),
                         (2 if l2_norm_clip is not None else 1) if train else 0,
                         d.ctypes.data_as(VP), ptr(desc_dev), ptr(scratch), int(gs), int(go),
                         int(key) & (2**64 - 1), stream_handle(records.device),
                         float(l2_norm_clip) if l2_norm_clip is not None else 0.0,
                         ptr(norms_out) if l2_norm_clip is not None else None)
    check(rc, "mifx_wdg_fused")


def _dp_args(dp, stride: int, kind, step_ctr) -> tuple[int, float, float, int]:
    """dp: None or (noise stddev = noise_multiplier x l2_norm_clip or None for no noise, grad_scale, seed) ->
    (dp_mode, stddev, grad_scale, seed) of mifx_wdg_reduce_opt."""
    if dp is None:
        return 0, 0.0, 1.0, 0
    std, gscale, seed = dp
    if std is None:
        return 1, 0.0, float(gscale), 0
    if not float(std) >= 0.0:
        raise ValueError("the noise stddev must be >= 0")
    if kind is None or kind.numel() != stride or kind.dtype != torch.int32 or step_ctr is None \
            or step_ctr.dtype != torch.int64 or step_ctr.numel() < constants()["SLOTS"]:
        raise ValueError("DP noise needs kind int32 [stride] and step_ctr int64 [SLOTS]")
    return 2, float(std), float(gscale), int(seed) & (2**64 - 1)


def reduce_sum(slab: torch.Tensor, rows: int, out: torch.Tensor, dp=None, kind: torch.Tensor | None = None,
               step_ctr: torch.Tensor | None = None) -> None:
    """out [stride] = sum of the first `rows` slab rows, in row order. dp = (stddev or None, grad_scale, seed): the
    slab holds clipped per-example gradients; the sum gets stddev x N(0,1) on the columns with kind != -1 (the
    stream of the step in step_ctr, which is left alone; None: no noise), then times grad_scale."""
    stride = int(slab.shape[-1])
    if out.numel() < stride or slab.shape[0] < rows or not slab.is_contiguous() or slab.dtype != torch.float32:
        raise ValueError("reduce_sum: slab fp32 [>= rows, stride], out [>= stride]")
    mode, std, gscale, seed = _dp_args(dp, stride, kind, step_ctr)
    rc = _fns()["reduce_opt"](ptr(slab), int(rows), stride, ptr(out), ptr(kind) if mode == 2 else None, None, None,
                              None, None, 0, ptr(step_ctr) if mode == 2 else None, None, None,
                              stream_handle(slab.device), mode, std, gscale, seed)
    check(rc, "mifx_wdg_reduce_opt")


def reduce_apply(slab: torch.Tensor, rows: int, kind: torch.Tensor, param: torch.Tensor, s0: torch.Tensor,
                 s1: torch.Tensor, wimg: torch.Tensor, step_ctr: torch.Tensor, hyper_dnn: torch.Tensor,
                 hyper_wide: torch.Tensor, dp=None) -> None:
    """Slab row sum + optimizer on the slab-column-order state + both bf16 images (wdg_reduce_opt). hyper_*: host
    fp32 [8] (OptSpec.encode()). dp: as reduce_sum (the noise of the step the slots hold before the increment)."""
    stride = int(slab.shape[-1])
    wtot = stride - constants()["WIDE_PAD"]
    if slab.shape[0] < rows or not slab.is_contiguous() or slab.dtype != torch.float32:
        raise ValueError("slab must be contiguous fp32 [>= rows, stride]")
    for t in (param, s0, s1):
        if t.numel() != stride or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("param / s0 / s1 must be contiguous fp32 [stride]")
    if kind.numel() != stride or kind.dtype != torch.int32 or wimg.numel() != 2 * wtot or wimg.element_size() != 2:
        raise ValueError("kind must be int32 [stride], the image 16-bit [2 * WTOT]")
    if step_ctr.dtype != torch.int64 or step_ctr.numel() < constants()["SLOTS"]:
        raise ValueError("step_ctr must be int64 [SLOTS]")
    if hyper_dnn.device.type != "cpu" or hyper_wide.device.type != "cpu" or hyper_dnn.numel() != 8 \
            or hyper_wide.numel() != 8:
        raise ValueError("hyper-parameters are host fp32 [8] tensors")
    rc = _fns()["reduce_opt"](ptr(slab), int(rows), stride, None, ptr(kind), ptr(param), ptr(s0), ptr(s1), ptr(wimg),
                              wtot, ptr(step_ctr), ptr(hyper_dnn), ptr(hyper_wide), stream_handle(slab.device),
                              *_dp_args(dp, stride, kind, step_ctr))
    check(rc, "mifx_wdg_reduce_opt")
