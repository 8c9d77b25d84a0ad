"""eval_metric="ndcg" / "ndcg@k" of mifx.gbdt's XGBRanker on the device (csrc/gbdt_ndcg.hip; the host twin is
mifx.gbdt.xgb.ndcg, whose bits the kernels reproduce).

`NdcgPlan` is built once per fit from the eval set's row offsets and labels: it checks them, sorts the groups into the
work lists of the kernels' two routes (groups of up to 64 rows: one wave each; larger groups, of any size: tiles of 256
rows that count ranks against the whole group), computes the per-group IDCG with the host's own expression
(mifx.gbdt.xgb.ndcg_idcg) and uploads offsets, labels (uint8), the discount table, IDCG and the lists; it owns the
scratch of the tiled route and the [G] scores. `plan.group_scores(margin)` is then one call per evaluated round on the
current stream, up to three launches, no atomics; `plan.score(margin)` reads the G doubles back -- nothing else -- and
takes their mean with mifx.gbdt.xgb.ndcg_mean, the expression of the host function."""
from __future__ import annotations

import functools

import numpy as np
import torch

from ..gbdt.xgb import discount_tables, ndcg_idcg, ndcg_mean
from . import _lib
from ._lib import I32, VP, check, ptr, sig, stream_handle


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("gbdt_ndcg")
    return {
        "max_group": sig(lib, "mifx_gbdt_ndcg_max_group", []),
        "max_groups_per_wg": sig(lib, "mifx_gbdt_ndcg_max_groups_per_wg", []),
        "tile": sig(lib, "mifx_gbdt_ndcg_tile", []),
        "chunk_ok": sig(lib, "mifx_gbdt_ndcg_chunk_ok", [I32]),
        "ndcg": sig(lib, "mifx_gbdt_ndcg_gpu", [I32, VP, VP, VP, VP, VP, VP, I32, VP, I32, VP, I32, VP, VP, I32, I32,
                                                VP]),
    }


def max_group() -> int:
    """Rows of the largest eval group XGBRanker scores on the device (measured: profiles/gbdt_ndcg.md); with a longer
    one the fit reads the margins back and calls the host function, as it always did. The kernels have no limit."""
    return int(_fns()["max_group"]())


class NdcgPlan:
    """What the NDCG kernels need beside the eval margins, resident on `dev` for a whole fit."""

    def __init__(self, gptr: np.ndarray, y: np.ndarray, k: int, dev: torch.device):
        gptr = np.ascontiguousarray(gptr, np.int64)
        y = np.asarray(y, np.float64).reshape(-1)
        if gptr.ndim != 1 or len(gptr) < 1 or gptr[0] != 0 or (np.diff(gptr) < 0).any() or gptr[-1] != len(y):
            raise ValueError("gptr must hold the groups' ascending row offsets, from 0 to the number of labels")
        if len(y) >= 2 ** 31:
            raise ValueError("ndcg on the device takes fewer than 2^31 eval rows")
        if not np.isin(y, np.arange(32)).all():
            raise ValueError("ndcg: labels must be integers in [0, 31]")
        if int(k) != k or int(k) < 0:
            raise ValueError(f"k must be >= 0 (0: no cutoff), got {k!r}")
        sizes = np.diff(gptr)
        order = np.argsort(-sizes, kind="stable").astype(np.int32)  # by size, descending: the long groups start first
        tile = int(_fns()["tile"]())
        self.k, self.n, self.G, self.dev = int(k), len(y), len(sizes), dev
        self.n_big = int((sizes > 64).sum())
        big = order[:self.n_big]
        per = -(-sizes[big] // tile)  # tiles of each large group, in the list's order
        first = (np.arange(int(per.sum())) - np.repeat(np.cumsum(per) - per, per)) * tile
        tiles = np.stack([np.repeat(big, per), first.astype(np.int32)], 1).astype(np.int32)
        self.n_tiles = len(tiles)
        D = discount_tables(int(sizes.max()) if len(sizes) else 0)[0]
        host = (gptr, y.astype(np.uint8), D, ndcg_idcg(y, gptr, self.k), order, np.ascontiguousarray(tiles))
        with torch.cuda.device(dev):
            self.gptr, self.label, self.D, self.idcg, self.list, self.tiles = (torch.from_numpy(a).to(dev)
                                                                               for a in host)
            self.terms = torch.empty(self.n if self.n_tiles else 0, dtype=torch.float64, device=dev)
            self.scores = torch.empty(self.G, dtype=torch.float64, device=dev)

    def group_scores(self, margin: torch.Tensor, _groups_per_wg: int | None = None,
                     _chunk: int | None = None) -> torch.Tensor:
        """The groups' scores, float64 [G] on the plan's device (the plan's own tensor, rewritten by every call), of
        the float64 margins [n] there. The private arguments are launch geometry (groups per workgroup of the wave
        route and of the fold, 1 to 4; keys per LDS chunk of the tiled route, 512 or 2048) and change no bit."""
        margin = margin.reshape(-1)
        assert margin.dtype == torch.float64 and len(margin) == self.n
        assert margin.is_contiguous() and margin.device == self.dev
        fns = _fns()
        gpw, chunk = int(_groups_per_wg or fns["max_groups_per_wg"]()), int(_chunk or 0)
        if not 1 <= gpw <= fns["max_groups_per_wg"]() or (chunk and not fns["chunk_ok"](chunk)):
            raise ValueError(f"launch geometry outside the ndcg kernels' limits: groups per workgroup {gpw}, chunk "
                             f"{chunk}")
        with torch.cuda.device(self.dev):
            check(fns["ndcg"](self.k, ptr(margin), ptr(self.label), ptr(self.gptr), ptr(self.D), ptr(self.idcg),
                              ptr(self.list[self.n_big:]), self.G - self.n_big, ptr(self.tiles), self.n_tiles,
                              ptr(self.list), self.n_big, ptr(self.terms if self.n_tiles else None), ptr(self.scores),
                              gpw, chunk, stream_handle(self.dev)), "mifx_gbdt_ndcg_gpu")
        return self.scores

    def score(self, margin: torch.Tensor, **geometry) -> float:
        """The metric of the eval margins ([n] or the fit's [1, n]): the mean of the G scores, taken on the host."""
        return ndcg_mean(self.group_scores(margin, **geometry).cpu().numpy())  # the round's one read-back: G doubles
