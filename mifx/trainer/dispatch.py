"""Which Wide&Deep trainer a model trains on.

CPU: the PyTorch trainer. GPU: the chained kernel (FusedWideDeepTrainer) when it is compiled for the tower --
`check_fused_compatible` and `ops.wd_chain.check_live_tiles` accept it, which today means the live 16x16 tiles of the
taxi tower [100, 70, 48, 34] -- and the general fused kernel (GeneralWideDeepTrainer) for every other tower.
Differentially private training (dp=DPSpec) runs on the general kernel for every tower, the taxi default included:
the chained kernels have no DP mode. It is single-GPU.
"""
from __future__ import annotations

import torch

from ..models import wide_deep as wdm


def chain_kernel_accepts(cfg: wdm.WideDeepConfig) -> bool:
    """True when every build of the chained kernel (T = 64 / 128 / 256) is compiled for this tower."""
    from ..ops import wd_chain as wdc

    try:
        wdm.check_fused_compatible(cfg)
        tmap = wdm.chain_maps(cfg)[0]
        for tile in (64, 128, 256):
            wdc.check_live_tiles(cfg, tmap, tile)
    except ValueError:
        return False
    return True


def select_kernel(cfg: wdm.WideDeepConfig, kernel: str | None = None, dp: bool = False) -> str:
    """"chain" / "tile" / "general" for a GPU trainer. kernel=None: the chained kernel where it accepts the tower,
    else the general one; a forced specialised kernel on a tower it cannot run raises as before. dp: DP training,
    which only the general kernel has: every tower goes there, a forced "chain" / "tile" raises."""
    if kernel is not None and kernel not in ("chain", "tile", "general"):
        raise ValueError("kernel must be 'chain', 'tile', 'general' or None")
    if dp:
        if kernel in ("chain", "tile"):
            raise ValueError(f"DP training runs on the general fused kernel only: kernel={kernel!r} has no DP mode")
        return "general"
    if kernel is None:
        return "chain" if chain_kernel_accepts(cfg) else "general"
    return kernel


def check_world(cfg: wdm.WideDeepConfig, world: int, device_type: str = "cuda", kernel: str | None = None,
                dp: bool = False) -> None:
    """Raise before any rank starts when a data-parallel GPU job asks for a tower only the general kernel trains,
    or for DP training (any tower, any device: per-example clipping has no data-parallel path)."""
    if world > 1 and dp:
        raise ValueError(f"DP training is single-GPU: per-example clipping and the noise run inside the general "
                         f"fused step, which has no data-parallel path (num_gpus / world = {world}); use one GPU or "
                         f"train without DP")
    if world > 1 and device_type == "cuda" and select_kernel(cfg, kernel) == "general":
        wdm.check_general_compatible(cfg)
        raise ValueError(f"general towers are single-GPU: hidden_units {list(cfg.hidden_units)} train on the general "
                         f"fused kernel, which has no data-parallel path yet (num_gpus / world = {world}); use one "
                         f"GPU or the taxi tower {wdm.dnn_hidden_units()}")


def make_wide_deep_trainer(model: wdm.WideDeepModel, device, *, batch: int = 40, dnn_opt=None, wide_opt=None,
                           loss_reduction: str = "sum", process_group=None, kernel: str | None = None,
                           shuffle_seed: int = 0, feed_stride: int | None = None, feed_offset: int = 0, dp=None,
                           **kw):
    """The trainer for `model` on `device`. kernel (GPU only): None = automatic, "general" forces the general
    kernel (tests, A/B), "chain" / "tile" the specialised ones. dp: privacy.DPSpec for per-example DP-SGD (the CPU
    trainer, or the general kernel for every tower). **kw goes to the chosen trainer."""
    from .fused_wide_deep import FusedWideDeepTrainer
    from .general_wide_deep import GeneralWideDeepTrainer
    from .torch_wide_deep import TorchWideDeepTrainer

    device = torch.device(device)
    common = dict(batch=batch, device=device, dnn_opt=dnn_opt, wide_opt=wide_opt, loss_reduction=loss_reduction,
                  process_group=process_group, shuffle_seed=shuffle_seed, feed_stride=feed_stride,
                  feed_offset=feed_offset)
    if dp is not None:
        kw = dict(kw, dp=dp)  # only the trainers with a DP mode take the argument
    if device.type != "cuda":
        return TorchWideDeepTrainer(model, **common, **kw)
    k = select_kernel(model.cfg, kernel, dp=dp is not None)
    if k == "general":
        return GeneralWideDeepTrainer(model, **common, **kw)
    return FusedWideDeepTrainer(model, kernel=k, **common, **kw)
