"""Flat mixed-precision AdamW (csrc/adamw.hip): bf16 weights/grads in flat buffers, fp32 master +
moments, one launch per step, device-side step counter (graph-capturable). CPU reference included.

The fine-tuning recipe (clip by global norm, linear warmup / decay, per-parameter weight decay) runs on the device as
well: clip_coef_ + adamw_chunks_ex_, with adamw_recipe_reference_ as the CPU reference."""
from __future__ import annotations

import functools

import torch

from . import _lib
from ._lib import F32, I32, I64, VP, check, ptr, sig, stream_handle


@functools.lru_cache(maxsize=None)
def _fn():
    lib = _lib.load("adamw")
    return sig(lib, "mifx_adamw_flat", [VP, VP, VP, VP, VP, I64, VP, F32, F32, F32, F32, F32, F32, VP])


@functools.lru_cache(maxsize=None)
def _fns_chunks():
    lib = _lib.load("adamw")
    return {"chunk": sig(lib, "mifx_adamw_chunk_size", []),
            "run": sig(lib, "mifx_adamw_chunks", [VP, VP, VP, VP, VP, VP, I32, VP, VP, VP, VP, F32, F32, F32, F32,
                                                  F32, F32, VP]),
            "run_noadv": sig(lib, "mifx_adamw_chunks_noadv", [VP, VP, VP, VP, VP, VP, I32, VP, VP, VP, VP, F32, F32,
                                                              F32, F32, F32, F32, VP]),
            "advance": sig(lib, "mifx_adamw_advance", [VP, VP]),
            "clip_coef": sig(lib, "mifx_adamw_clip_coef", [VP, VP, VP, VP, I32, VP, F32, VP, VP]),
            "run_ex": sig(lib, "mifx_adamw_chunks_ex", [VP, VP, VP, VP, VP, VP, I32, VP, VP, VP, VP, F32, F32, F32,
                                                        F32, F32, F32, VP, VP, I32, I32, I32, VP])}


def chunk_size() -> int:
    return int(_fns_chunks()["chunk"]())


def adamw_chunks_(param: torch.Tensor, gptr: torch.Tensor, poff: torch.Tensor, bp: torch.Tensor, bo: torch.Tensor,
                  bn: torch.Tensor, master: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: torch.Tensor,
                  lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
                  grad_scale: float = 1.0, advance: bool = True) -> None:
    """AdamW over flat bf16 weights / fp32 master+moments with each parameter's gradient read from its own
    tensor: gptr [P] uint64 device addresses (0 = no grad), poff [P] int64 flat offsets (multiples of 8),
    bp/bo/bn [nblocks] int32 chunk -> (parameter, element offset, length). See FlatAdamW. advance=False leaves the
    step counter (adamw_advance_ once after all launches of a split step)."""
    assert param.dtype == torch.bfloat16 and master.dtype == m.dtype == v.dtype == torch.float32
    assert gptr.dtype == torch.int64 and poff.dtype == torch.int64 and step.dtype == torch.int32
    assert bp.dtype == bo.dtype == bn.dtype == torch.int32 and bp.numel() == bo.numel() == bn.numel()
    check(_fns_chunks()["run" if advance else "run_noadv"](ptr(param), ptr(gptr), ptr(poff), ptr(bp), ptr(bo), ptr(bn), int(bp.numel()),
                               ptr(master), ptr(m), ptr(v), ptr(step), float(lr), float(beta1), float(beta2),
                               float(eps), float(weight_decay), float(grad_scale), stream_handle(param.device)),
          "mifx_adamw_chunks")


def adamw_flat_(param: torch.Tensor, grad: torch.Tensor, master: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
                step: torch.Tensor, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                weight_decay: float = 0.0, grad_scale: float = 1.0) -> None:
    """In-place AdamW over flat 1-D buffers; `step` is an int32 device scalar advanced by one."""
    n = param.numel()
    if param.is_cuda:
        assert param.dtype == grad.dtype == torch.bfloat16 and master.dtype == m.dtype == v.dtype == torch.float32
        assert step.dtype == torch.int32 and all(t.numel() == n for t in (grad, master, m, v))
        check(_fn()(ptr(param), ptr(grad), ptr(master), ptr(m), ptr(v), n, ptr(step), float(lr), float(beta1),
                    float(beta2), float(eps), float(weight_decay), float(grad_scale), stream_handle(param.device)),
              "mifx_adamw_flat")
        return
    t = int(step.item()) + 1
    g = grad.float() * grad_scale
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    master.mul_(1 - lr * weight_decay).addcdiv_(m, v.sqrt() / bc2 ** 0.5 + eps, value=-lr / bc1)
    param.copy_(master.to(param.dtype))
    step.add_(1)


def adamw_advance_(step: torch.Tensor) -> None:
    check(_fns_chunks()["advance"](ptr(step), stream_handle(step.device)), "mifx_adamw_advance")


# ------------------------------------------------------------------ fine-tuning recipe (clip / schedule / per-param wd)
SCHED_CONSTANT, SCHED_LINEAR = 0, 1


def scheduled_lr(lr: float, schedule: tuple | None, t: int) -> float:
    """Learning rate of the update that follows `t` completed ones, in fp32 like the kernel. schedule None is
    constant; ("linear", warmup, total): t / max(1, warmup) below warmup, then max(0, (total - t) / max(1, total -
    warmup)) (LambdaLR with the usual linear-warmup lambda, stepped once per update)."""
    if schedule is None:
        return float(lr)
    _, warmup, total = schedule
    f32 = functools.partial(torch.tensor, dtype=torch.float32)
    if t < warmup:
        f = f32(t) / f32(max(1, warmup))
    else:
        f = torch.clamp_min(f32(total - t) / f32(max(1, total - warmup)), 0.0)
    return float(f32(lr) * f)


def clip_coef_(gptr: torch.Tensor, bp: torch.Tensor, bo: torch.Tensor, bn: torch.Tensor, partial: torch.Tensor,
               max_norm: float, clip: torch.Tensor) -> None:
    """clip[2] = {min(1, max_norm / (norm + 1e-6)), norm}: the global L2 norm of the bf16 gradients behind gptr over
    the chunk tables of adamw_chunks_ (partial: [nblocks] fp32 scratch). Two launches, bit-reproducible, no sync."""
    assert gptr.dtype == torch.int64 and bp.dtype == bo.dtype == bn.dtype == torch.int32
    assert partial.dtype == clip.dtype == torch.float32 and partial.numel() >= bp.numel() and clip.numel() >= 2
    check(_fns_chunks()["clip_coef"](ptr(gptr), ptr(bp), ptr(bo), ptr(bn), int(bp.numel()), ptr(partial),
                                     float(max_norm), ptr(clip), stream_handle(gptr.device)), "mifx_adamw_clip_coef")


def adamw_chunks_ex_(param: torch.Tensor, gptr: torch.Tensor, poff: torch.Tensor, bp: torch.Tensor, bo: torch.Tensor,
                     bn: torch.Tensor, master: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: torch.Tensor,
                     lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, weight_decay: float = 0.0,
                     grad_scale: float = 1.0, clip: torch.Tensor | None = None, pwd: torch.Tensor | None = None,
                     schedule: tuple | None = None) -> None:
    """adamw_chunks_ with the recipe evaluated on the device (graph-capturable): gradients scaled by clip[0] (from
    clip_coef_), weight decay per parameter from pwd [P] fp32, learning rate from `schedule` at the device step."""
    assert param.dtype == torch.bfloat16 and master.dtype == m.dtype == v.dtype == torch.float32
    assert gptr.dtype == torch.int64 and poff.dtype == torch.int64 and step.dtype == torch.int32
    assert bp.dtype == bo.dtype == bn.dtype == torch.int32 and bp.numel() == bo.numel() == bn.numel()
    assert clip is None or (clip.dtype == torch.float32 and clip.numel() >= 2)
    assert pwd is None or (pwd.dtype == torch.float32 and pwd.numel() == gptr.numel())
    kind, warmup, total = (SCHED_CONSTANT, 0, 0) if schedule is None else (SCHED_LINEAR, schedule[1], schedule[2])
    check(_fns_chunks()["run_ex"](ptr(param), ptr(gptr), ptr(poff), ptr(bp), ptr(bo), ptr(bn), int(bp.numel()),
                                  ptr(master), ptr(m), ptr(v), ptr(step), float(lr), float(beta1), float(beta2),
                                  float(eps), float(weight_decay), float(grad_scale), ptr(clip), ptr(pwd), kind,
                                  int(warmup), int(total), stream_handle(param.device)), "mifx_adamw_chunks_ex")


def adamw_recipe_reference_(params: list, grads: list, masters: list, ms: list, vs: list, step: torch.Tensor,
                            lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8,
                            weight_decays: list | float = 0.0, grad_scale: float = 1.0,
                            max_grad_norm: float | None = None, schedule: tuple | None = None) -> tuple:
    """CPU reference of clip_coef_ + adamw_chunks_ex_, one tensor per parameter (grads[i] None: the parameter is left
    untouched and does not count in the norm). The squared norm is summed over the gradient values in fp64; coef,
    lr_t and the update are fp32. Advances `step`; returns (norm or None, lr_t)."""
    t = int(step.item())
    lr_t = scheduled_lr(lr, schedule, t)
    norm, scale = None, torch.tensor(float(grad_scale), dtype=torch.float32)
    if max_grad_norm is not None:
        sq = torch.zeros((), dtype=torch.float64)
        for g in grads:
            if g is not None:
                sq += g.detach().double().pow(2).sum()
        norm_t = sq.sqrt().float()
        coef = torch.tensor(float(max_grad_norm), dtype=torch.float32) / (norm_t + 1e-6)
        scale = torch.clamp(coef, max=1.0) * scale  # (clamp keeps a NaN, like clip_grad_norm_)
        norm = float(norm_t)
    bc1, bc2 = 1 - beta1 ** (t + 1), 1 - beta2 ** (t + 1)
    for i, (p, g, w, m, v) in enumerate(zip(params, grads, masters, ms, vs)):
        if g is None:
            continue
        wd = weight_decays[i] if isinstance(weight_decays, (list, tuple)) else weight_decays
        g = g.detach().reshape(-1).float() * scale
        m.mul_(beta1).add_(g, alpha=1 - beta1)
        v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        w.mul_(1 - lr_t * wd).addcdiv_(m, v.sqrt() / bc2 ** 0.5 + eps, value=-lr_t / bc1)
        p.copy_(w.to(p.dtype))
    step.add_(1)
    return norm, lr_t
