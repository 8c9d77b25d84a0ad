"""The LambdaMART gradient pair of mifx.gbdt's XGBRanker on the device (csrc/gbdt_rank.hip; the rule is
csrc/gbdt_rank.h, the host twin mifx.gbdt.xgb.rank_grad).

`RankPlan` is built once per fit from the groups' row offsets: it checks the device path's limit (a group of more than
`max_group()` rows raises ValueError, before anything is uploaded or launched; there is no host fallback), sorts the
groups by size, descending, into the work list of the kernels' two routes, and uploads the offsets, the list and the
discount tables. `grad_hess_rank` is then one call per boosting round on the current stream: up to three launches
(workgroup route above 512 rows, workgroup route above 64, wave route), no atomics, nothing read back."""
from __future__ import annotations

import functools

import numpy as np
import torch

from ..gbdt.xgb import discount_tables
from . import _lib
from ._lib import I32, VP, check, ptr, sig, stream_handle

OBJECTIVES = {"rank:pairwise": 0, "rank:ndcg": 1}


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("gbdt_rank")
    return {
        "max_group": sig(lib, "mifx_gbdt_rank_max_group", []),
        "mid_group": sig(lib, "mifx_gbdt_rank_mid_group", []),
        "grad": sig(lib, "mifx_gbdt_rank_grad_gpu", [I32, I32, VP, VP, I32, VP, VP, I32, I32, I32, I32, I32, VP, VP, VP,
                                                     VP, I32, I32, VP]),
    }


def max_group() -> int:
    """Rows of the largest query group the device path takes (the kernel's LDS image)."""
    return int(_fns()["max_group"]())


def check_groups(gptr: np.ndarray) -> np.ndarray:
    """The groups' sizes, after the device path's limit is checked (needs no GPU)."""
    sizes = np.diff(np.asarray(gptr, np.int64))
    if len(sizes) and int(sizes.max()) > max_group():
        raise ValueError(f"device='gpu' ranks query groups of up to {max_group()} rows, got one of {int(sizes.max())} "
                         f"(there is no fallback to the host learner)")
    return sizes


class RankPlan:
    """What the gradient kernels need beside margins and labels, resident on `dev` for a whole fit."""

    def __init__(self, gptr: np.ndarray, dev: torch.device):
        gptr = np.ascontiguousarray(gptr, np.int64)
        if gptr.ndim != 1 or len(gptr) < 1 or gptr[0] != 0 or (np.diff(gptr) < 0).any():
            raise ValueError("gptr must hold the groups' ascending row offsets, starting at 0")
        sizes = check_groups(gptr)
        if len(sizes) >= 2 ** 31:
            raise ValueError("too many query groups")
        order = np.argsort(-sizes, kind="stable").astype(np.int32)  # by size, descending: the large groups start first
        mid = int(_fns()["mid_group"]())
        self.n, self.dev = int(gptr[-1]), dev
        self.n_large = int((sizes > mid).sum())
        self.n_mid = int((sizes > 64).sum()) - self.n_large
        self.n_small = len(sizes) - self.n_large - self.n_mid
        self.largest = int(sizes.max()) if self.n_large else 0
        self.largest_mid = int(sizes[order[self.n_large]]) if self.n_mid else 0
        D, P = discount_tables(int(sizes.max()) if len(sizes) else 0)
        self.gptr, self.list, self.D, self.P = (torch.from_numpy(a).to(dev) for a in (gptr, order, D, P))


def grad_hess_rank(objective: str, margin: torch.Tensor, y: torch.Tensor, plan: RankPlan, g: torch.Tensor,
                   h: torch.Tensor, topk: int = 0, _groups_per_wg: int | None = None,
                   _threads: int | None = None) -> None:
    """g, h (float32 [n]) of "rank:pairwise" or "rank:ndcg" from float64 margins and the labels y (uint8 or float64,
    integers in [0, 31]) over the groups of `plan`; topk = k >= 1 keeps the pairs with a row ranked above k, 0 all.
    The private arguments are launch geometry (groups per workgroup of the wave route, 1 to 4; threads of the
    workgroup route, 64 to 256) and change no bit of the result."""
    assert margin.dtype == torch.float64 and y.dtype in (torch.uint8, torch.float64)
    assert g.dtype == h.dtype == torch.float32
    assert len(margin) == len(y) == len(g) == len(h) == plan.n
    for t in (margin, y, g, h):
        assert t.is_contiguous() and t.device == plan.dev
    if int(topk) < 0:
        raise ValueError(f"topk must be >= 0, got {topk}")
    rc = _fns()["grad"](OBJECTIVES[objective], int(topk), ptr(margin), ptr(y), int(y.dtype == torch.float64),
                        ptr(plan.gptr), ptr(plan.list), plan.n_large, plan.largest, plan.n_mid, plan.largest_mid,
                        plan.n_small, ptr(plan.D), ptr(plan.P), ptr(g), ptr(h), int(_groups_per_wg or 4),
                        int(_threads or 256), stream_handle(plan.dev))
    if rc == -1:
        raise ValueError("launch geometry or plan outside the rank kernels' limits")
    check(rc, "mifx_gbdt_rank_grad_gpu")
