"""eval_metric="auc" of mifx.gbdt's XGBClassifier on the device (csrc/gbdt_auc.hip; the rule is csrc/gbdt_auc.h, the
host twin mifx.gbdt.xgb.auc).

`AucPlan` is built once per fit from the eval set's labels: it refuses an eval set in which a class has no positive or
no negative row (ValueError, before anything is launched), uploads the label bytes and the P_k / N_k, and owns the
scratch of every later call (the [m, 2 G] table, the sort's buffers and its [2 G, m] result, the K counters), sized for
groups of G classes that stay inside the sort's memory budget. `plan.counts(margin)` is then one call per evaluated
round on the current stream -- per group a fill launch, the batched radix sort of csrc/gbdt_sort.hip and a count
launch -- and reads back the K int64 pair counts, nothing else; `plan.score(margin)` forms the score from them with
mifx.gbdt.xgb.auc_score, the one function both learners use."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from ..gbdt.xgb import auc_score
from . import _lib
from ._lib import I32, VP, check, ptr, sig, stream_handle
from .gbdt_prep import SORT_BUDGET, _sort_fns, _sort_tile

LONG = ctypes.c_long
COUNT_TILE = 2048    # sorted positives of one workgroup of the count kernel
COUNT_THREADS = 256
COUNT_CHUNK = 4096   # negatives staged in LDS at a time (32 KB)


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("gbdt_auc")
    return {
        "max_chunk": sig(lib, "mifx_gbdt_auc_max_chunk", []),
        "max_threads": sig(lib, "mifx_gbdt_auc_max_threads", []),
        "max_group": sig(lib, "mifx_gbdt_auc_max_group", []),
        "fill": sig(lib, "mifx_gbdt_auc_fill", [VP, VP, LONG, I32, I32, I32, VP, VP, VP]),
        "count": sig(lib, "mifx_gbdt_auc_count", [VP, LONG, I32, I32, I32, VP, LONG, I32, I32, I32, VP, VP]),
    }


def class_counts(y: np.ndarray, num_class: int) -> tuple[np.ndarray, np.ndarray]:
    """(P, N) int64 [K] of labels y (class indices; K = 1: 0 / 1 with 1 the positive), after the metric's check: a class
    without a positive or without a negative row raises ValueError. Needs no GPU."""
    y = np.asarray(y).reshape(-1)
    K = int(num_class)
    if not len(y) or (y != y.astype(np.int64)).any() or y.min() < 0 or y.max() >= max(K, 2):
        raise ValueError(f"auc: labels must be class indices in [0, {max(K, 2)}), one per row of a non-empty eval set")
    per_class = np.bincount(y.astype(np.int64), minlength=max(K, 2))
    P = per_class[1:2] if K == 1 else per_class[:K]
    N = len(y) - P
    if (P == 0).any() or (N == 0).any():
        raise ValueError("auc is undefined on an eval set in which a class has no positive or no negative row")
    return P.astype(np.int64), N.astype(np.int64)


class AucPlan:
    """What the AUC kernels need beside the eval margins, resident on `dev` for a whole fit."""

    def __init__(self, y_eval: np.ndarray, num_class: int, dev: torch.device, _group: int | None = None,
                 _sort_tile_keys: int | None = None):
        self.K, self.m, self.dev = int(num_class), int(np.asarray(y_eval).size), dev
        if not 1 <= self.K <= 256:
            raise ValueError(f"auc on the device takes up to 256 classes (the labels are bytes), got {self.K}")
        if self.m >= 2 ** 31:
            raise ValueError("auc on the device takes fewer than 2^31 eval rows")
        self.P, self.N = class_counts(y_eval, self.K)
        self.sort_tile = _sort_tile(_sort_tile_keys)
        # a class is two columns of the sort (key buffers, scratch, result) and of the table: as many as the budget holds
        per_class = _sort_fns()["scratch_bytes"](self.m, 2, self.sort_tile, 1) + 32 * self.m
        self.group = int(_group or max(1, min(self.K, _fns()["max_group"](), SORT_BUDGET // per_class)))
        if not 1 <= self.group <= min(self.K, _fns()["max_group"]()):
            raise ValueError(f"the class group must be in [1, {self.K}], got {self.group}")
        cols = 2 * self.group
        with torch.cuda.device(dev):
            self.label = torch.from_numpy(np.asarray(y_eval).reshape(-1).astype(np.uint8)).to(dev)
            self.pn = torch.from_numpy(np.ascontiguousarray(np.stack([self.P, self.N], 1))).to(dev)
            self.u2 = torch.zeros(self.K, dtype=torch.int64, device=dev)
            self.table = torch.empty(self.m * cols, dtype=torch.float64, device=dev)
            self.sorted = torch.empty(cols * self.m, dtype=torch.float64, device=dev)
            self.nan_count = torch.empty(cols, dtype=torch.int64, device=dev)
            self.scratch = torch.empty(_sort_fns()["scratch_bytes"](self.m, cols, self.sort_tile, 1),
                                       dtype=torch.uint8, device=dev)

    def counts(self, margin: torch.Tensor, _tile: int | None = None, _threads: int | None = None,
               _chunk: int | None = None) -> np.ndarray:
        """U2 int64 [K] (numpy) of the class-major float64 margins [K, m] on the plan's device: per class twice the
        (negative, positive) pairs ranked right plus the tied ones, the integers of mifx.gbdt.xgb.auc. The private
        arguments are the count kernel's geometry (positives per workgroup, threads, negatives per LDS chunk) and
        change no bit. Margins must be finite (not checked here)."""
        if margin.dim() == 1:
            margin = margin[None]
        assert margin.dtype == torch.float64 and tuple(margin.shape) == (self.K, self.m)
        assert margin.is_contiguous() and margin.device == self.dev
        fns = _fns()
        tile, threads, chunk = int(_tile or COUNT_TILE), int(_threads or COUNT_THREADS), int(_chunk or COUNT_CHUNK)
        if tile < 1 or threads % 64 or not 64 <= threads <= fns["max_threads"]() or \
                not 1 <= chunk <= fns["max_chunk"]():
            raise ValueError(f"count geometry outside the kernel's limits: tile {tile}, threads {threads}, chunk {chunk}")
        with torch.cuda.device(self.dev):
            for c0 in range(0, self.K, self.group):
                G = min(self.group, self.K - c0)
                self._fill(margin, c0, G)
                self._sort(G)
                self._count(c0, G, tile, threads, chunk)
            return self.u2.cpu().numpy()  # the round's one read-back: K integers

    # the three stages of one class group [c0, c0 + G), each enqueued on the current stream
    def _fill(self, margin: torch.Tensor, c0: int, G: int) -> None:
        check(_fns()["fill"](ptr(margin), ptr(self.label), self.m, self.K, c0, G, ptr(self.table), ptr(self.u2),
                             stream_handle(self.dev)), "mifx_gbdt_auc_fill")

    def _sort(self, G: int) -> None:
        check(_sort_fns()["launch"](ptr(self.table), 1, self.m, 2 * G, 0, 2 * G, self.sort_tile, ptr(self.scratch),
                                    ptr(self.sorted), ptr(self.nan_count), stream_handle(self.dev)),
              "mifx_gbdt_sort_launch")

    def _count(self, c0: int, G: int, tile: int, threads: int, chunk: int) -> None:
        check(_fns()["count"](ptr(self.sorted), self.m, self.K, c0, G, ptr(self.pn), int(self.P[c0:c0 + G].max()),
                              tile, threads, chunk, ptr(self.u2), stream_handle(self.dev)), "mifx_gbdt_auc_count")

    def score(self, margin: torch.Tensor, **geometry) -> float:
        """The AUC (one-vs-rest, weighted by prevalence, for K >= 3) of the margins: auc_score of the device counts."""
        return auc_score(self.counts(margin, **geometry), self.P, self.N)
