"""Device learner of mifx.gbdt (csrc/gbdt_gpu.hip): gradients, one fixed-point tree per call (int64 histograms, the
split rule of csrc/gbdt_split.h), the eval set's margin update. Everything stays on the device; nothing synchronises.

`Booster` holds what is resident for a whole fit (binned matrix row-major [n, f], the workspace); `grow_numpy` is the
one-tree entry the tests use (host arrays in, host arrays out).

Stochastic boosting: `Booster.grow(subsample=, seed=, round=, level_mask=)` grows the tree on the rows that the rule of
csrc/gbdt_sample.h keeps for (seed, round), as if the table held only them, and lets level d split only on the
features of `level_mask[d]` (a [max_depth, f] uint8 tensor on the device, computed by the host:
mifx.gbdt.sample.level_mask); `grad_hess(weight=)` multiplies the float32 pair by float32 instance weights.

Multi-class (multi:softprob): `grad_hess_softmax` computes the pairs of all K classes from class-major [K, n] margins
in one launch; the round then calls `Booster.grow` (and `Booster.apply`) once per class on row k of g, h and the
margins, with the tree index round * K + k as `round`."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import I32, I64, VP, check, ptr, sig, stream_handle

F64 = ctypes.c_double
LONG = ctypes.c_long
U64 = ctypes.c_uint64
ROWS_PER_WG = 2048  # rows of one node that one workgroup accumulates in LDS before it flushes
FEAT_TILE = 8       # features per workgroup: 8 * 257 slots * 20 B = 41 KB of LDS


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("gbdt_gpu")
    return {
        "max_depth": sig(lib, "mifx_gbdt_gpu_max_depth", []),
        "max_bins": sig(lib, "mifx_gbdt_gpu_max_bins", []),
        "max_feat_tile": sig(lib, "mifx_gbdt_gpu_max_feat_tile", []),
        "ws_bytes": sig(lib, "mifx_gbdt_gpu_ws_bytes", [LONG, I32, I32, I32], I64),
        "grad": sig(lib, "mifx_gbdt_gpu_grad", [I32, VP, VP, LONG, VP, VP, VP]),
        "grow": sig(lib, "mifx_gbdt_gpu_grow", [VP, LONG, I32, VP, VP, I32, VP, VP, I32, F64, F64, F64, F64, VP, I64,
                                                 VP, VP, VP, VP, VP, VP, VP, VP, VP, I32, I32, VP]),
        "grad_w": sig(lib, "mifx_gbdt_gpu_grad_w", [I32, VP, VP, VP, LONG, VP, VP, VP]),
        "grow_ex": sig(lib, "mifx_gbdt_gpu_grow_ex", [VP, LONG, I32, VP, VP, I32, VP, VP, I32, F64, F64, F64, F64, VP,
                                                       I64, VP, VP, VP, VP, VP, VP, VP, VP, VP, I32, I32, U64, U64,
                                                       U64, VP, I32, VP]),
        "grow_stats": sig(lib, "mifx_gbdt_gpu_grow_stats", [VP, LONG, I32, VP, VP, I32, VP, VP, I32, F64, F64, F64, F64,
                                                             VP, I64, VP, VP, VP, VP, VP, VP, VP, VP, VP, I32, I32, U64,
                                                             U64, U64, VP, I32, VP, VP, VP]),
        "apply": sig(lib, "mifx_gbdt_gpu_apply", [VP, LONG, I32, VP, VP, VP, VP, VP, VP, VP, I32, VP, VP]),
        "grad_softmax": sig(lib, "mifx_gbdt_gpu_grad_softmax", [VP, VP, VP, LONG, I32, VP, VP, VP]),
    }


def check_limits(n: int, max_bins: int, max_depth: int) -> None:
    """The device path's limits, checked before anything is launched (and without a GPU)."""
    fns = _fns()
    if max_bins > fns["max_bins"]():
        raise ValueError(f"device='gpu' supports max_bins <= {fns['max_bins']()}, got {max_bins}")
    if not 0 <= max_depth <= fns["max_depth"]():
        raise ValueError(f"device='gpu' supports max_depth <= {fns['max_depth']()}, got {max_depth}")
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"device='gpu' supports 1 <= n < 2^31 rows, got {n}")


def device_for(index: int) -> torch.device:
    if not _lib.gpu_available():
        raise RuntimeError("device='gpu' was requested but no GPU is visible (there is no fallback to the host learner)")
    if index >= torch.cuda.device_count():
        raise ValueError(f"device='cuda:{index}' but only {torch.cuda.device_count()} GPU(s) are visible")
    return torch.device("cuda", index)


def upload_bins(bins: np.ndarray, dev: torch.device) -> torch.Tensor:
    """Host column-major [f, n] uint16 -> device row-major [n, f] (int16 storage, the same bits)."""
    return torch.from_numpy(np.ascontiguousarray(bins).view(np.int16)).to(dev).t().contiguous()


def grad_hess(objective: str, margin: torch.Tensor, y: torch.Tensor, g: torch.Tensor, h: torch.Tensor,
              weight: torch.Tensor | None = None) -> None:
    """g, h (float32) of "reg:squarederror" or "binary:logistic" from float64 margins and labels; with `weight`
    (float32 [n] on the device) each is the unweighted float32 value times the weight, one float32 multiply."""
    obj = {"reg:squarederror": 0, "binary:logistic": 1}[objective]
    assert margin.dtype == y.dtype == torch.float64 and g.dtype == h.dtype == torch.float32
    assert margin.is_contiguous() and y.is_contiguous() and g.is_contiguous() and h.is_contiguous()
    assert len(margin) == len(y) == len(g) == len(h)
    if weight is None:
        check(_fns()["grad"](obj, ptr(margin), ptr(y), len(y), ptr(g), ptr(h), stream_handle(margin.device)),
              "mifx_gbdt_gpu_grad")
        return
    assert weight.dtype == torch.float32 and weight.is_contiguous() and len(weight) == len(y)
    assert weight.device == margin.device
    check(_fns()["grad_w"](obj, ptr(margin), ptr(y), ptr(weight), len(y), ptr(g), ptr(h),
                           stream_handle(margin.device)), "mifx_gbdt_gpu_grad_w")


def grad_hess_softmax(margin: torch.Tensor, y: torch.Tensor, g: torch.Tensor, h: torch.Tensor,
                      weight: torch.Tensor | None = None) -> None:
    """g, h (float32 [K, n]) of "multi:softprob" from float64 margins [K, n] (class-major) and float64 class indices
    y [n], all K classes in one launch: XGBClassifier._grad_hess for K >= 3 is the specification (softmax in double,
    the sum in class order, h = max(2 p (1 - p), 1e-16)). `weight` as in grad_hess. K is margin.shape[0]: any K >= 1."""
    assert margin.dim() == 2 and margin.shape == g.shape == h.shape and y.shape == (margin.shape[1],)
    assert margin.dtype == y.dtype == torch.float64 and g.dtype == h.dtype == torch.float32
    assert margin.is_contiguous() and y.is_contiguous() and g.is_contiguous() and h.is_contiguous()
    assert y.device == g.device == h.device == margin.device
    if weight is not None:
        assert weight.dtype == torch.float32 and weight.is_contiguous() and weight.shape == y.shape
        assert weight.device == margin.device
    K, n = margin.shape
    check(_fns()["grad_softmax"](ptr(margin), ptr(y), ptr(weight), n, K, ptr(g), ptr(h),
                                 stream_handle(margin.device)), "mifx_gbdt_gpu_grad_softmax")


def row_threshold(subsample: float) -> int:
    """thr of csrc/gbdt_sample.h: (uint64)(subsample * 2^32); 2^32 keeps every row."""
    if not 0.0 < subsample <= 1.0:
        raise ValueError(f"subsample must be in (0, 1], got {subsample}")
    return int(float(subsample) * 4294967296.0)


class Booster:
    """Device-resident state of one fit: bins [n, f], per-feature bin counts, the grower's workspace."""

    def __init__(self, bins: np.ndarray, nbins: np.ndarray, max_depth: int, dev: torch.device):
        f, n = bins.shape
        self._setup(n, f, nbins, max_depth, dev, lambda: upload_bins(bins, dev))

    @classmethod
    def from_device_bins(cls, bins: torch.Tensor, nbins: np.ndarray, max_depth: int) -> "Booster":
        """A Booster on bins that are on the device already: row-major [n, f] int16 (mifx.ops.gbdt_prep.device_bins),
        kept as they are."""
        if not (bins.is_cuda and bins.dim() == 2 and bins.dtype == torch.int16 and bins.is_contiguous()):
            raise ValueError("expected a contiguous [n, f] int16 tensor on the GPU")
        self = cls.__new__(cls)
        self._setup(bins.shape[0], bins.shape[1], nbins, max_depth, bins.device, lambda: bins)
        return self

    def _setup(self, n: int, f: int, nbins: np.ndarray, max_depth: int, dev: torch.device, device_bins) -> None:
        nbins = np.asarray(nbins, np.int32)
        check_limits(n, int(nbins.max()), max_depth)
        if nbins.min() < 1 or len(nbins) != f:
            raise ValueError("nbins must hold one count >= 1 per feature")
        self.n, self.f, self.max_depth, self.dev = n, f, int(max_depth), dev
        self.cap = 2 ** (self.max_depth + 1)
        hoff = np.concatenate([[0], np.cumsum(nbins + 1)]).astype(np.int32)
        self.hsize = int(hoff[-1])
        self.bins = device_bins()
        self.nbins = torch.from_numpy(nbins).to(dev)
        self.hoff = torch.from_numpy(hoff[:-1].copy()).to(dev)
        nbytes = _fns()["ws_bytes"](n, f, self.max_depth, self.hsize)
        if nbytes < 0:
            raise ValueError("shape outside the device learner's limits")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.leaf_of_row = torch.empty(n, dtype=torch.int32, device=dev)

    def new_trees(self, count: int):
        """Tree arrays for `count` trees, [count, cap] each, and their node counts."""
        z = lambda dt: torch.empty((count, self.cap), dtype=dt, device=self.dev)  # noqa: E731
        return (z(torch.int32), z(torch.int32), z(torch.uint8), z(torch.int32), z(torch.int32), z(torch.float64),
                torch.zeros(count, dtype=torch.int32, device=self.dev))

    def new_stats(self, count: int):
        """Node statistics for `count` trees: (gain, cover), float64 [count, cap] each (Booster.grow's `stats=`)."""
        return tuple(torch.zeros((count, self.cap), dtype=torch.float64, device=self.dev) for _ in range(2))

    def grow(self, g: torch.Tensor, h: torch.Tensor, tree, min_child_weight: float, reg_lambda: float, gamma: float,
             eta: float, margin: torch.Tensor | None = None, _rows_per_wg: int | None = None,
             _feat_tile: int | None = None, subsample: float = 1.0, seed: int = 0, round: int = 0,
             level_mask: torch.Tensor | None = None, _margin_route: int = 0, stats=None) -> None:
        """One tree from float32 g, h into `tree` = (feature, split_bin, default_left, left, right, value, node_count)
        rows; leaf_of_row is set and, if given, margin += value[leaf]. The private arguments are the histogram
        kernel's launch geometry: the result does not depend on them.

        `subsample` < 1 grows the tree on the rows sampled for (seed, round) only (leaf_of_row = -1 for the others;
        every row's margin still receives the tree's output); `level_mask`: [max_depth, f] uint8 on the device, the
        features each level may split on. `_margin_route`: how the rows outside the sample get their margin (0: the
        partition updates the sampled rows and a tree walk the others, 1: one walk over all rows); the same sums.

        `stats` = (gain, cover): one tree's rows of `new_stats`; node k receives the gain of its split (0.0 at a leaf)
        and its hessian sum over the rows the tree was grown on. The tree is the same with and without them."""
        assert g.dtype == h.dtype == torch.float32 and len(g) == len(h) == self.n and g.is_contiguous()
        assert h.is_contiguous() and all(t.is_contiguous() for t in tree)
        assert margin is None or (margin.dtype == torch.float64 and len(margin) == self.n and margin.is_contiguous())
        rows, tile = int(_rows_per_wg or ROWS_PER_WG), int(_feat_tile or FEAT_TILE)
        if rows < 1 or not 1 <= tile <= _fns()["max_feat_tile"]():
            raise ValueError("launch geometry out of range")
        fe, sb, dl, le, ri, val, cnt = tree
        thr = row_threshold(subsample)
        if level_mask is not None:
            if self.max_depth == 0:
                level_mask = None
            elif not (level_mask.dtype == torch.uint8 and level_mask.is_contiguous() and level_mask.device == self.dev
                      and tuple(level_mask.shape) == (self.max_depth, self.f)):
                raise ValueError(f"level_mask must be a contiguous uint8 [{self.max_depth}, {self.f}] tensor on "
                                 f"{self.dev}")
        if stats is not None:
            gain, cover = stats
            for s in (gain, cover):
                assert s.dtype == torch.float64 and s.is_contiguous() and s.numel() == self.cap and s.device == self.dev
            check(_fns()["grow_stats"](ptr(self.bins), self.n, self.f, ptr(self.nbins), ptr(self.hoff), self.hsize,
                                       ptr(g), ptr(h), self.max_depth, float(min_child_weight), float(reg_lambda),
                                       float(gamma), float(eta), ptr(self.ws), self.ws.numel(), ptr(fe), ptr(sb),
                                       ptr(dl), ptr(le), ptr(ri), ptr(val), ptr(cnt), ptr(self.leaf_of_row),
                                       ptr(margin), rows, tile, int(seed) & (2 ** 64 - 1), int(round) & (2 ** 64 - 1),
                                       thr, ptr(level_mask), int(_margin_route), ptr(gain), ptr(cover),
                                       stream_handle(self.dev)), "mifx_gbdt_gpu_grow_stats")
            return
        if thr == 2 ** 32 and level_mask is None:
            check(_fns()["grow"](ptr(self.bins), self.n, self.f, ptr(self.nbins), ptr(self.hoff), self.hsize, ptr(g),
                                 ptr(h), self.max_depth, float(min_child_weight), float(reg_lambda), float(gamma),
                                 float(eta), ptr(self.ws), self.ws.numel(), ptr(fe), ptr(sb), ptr(dl), ptr(le),
                                 ptr(ri), ptr(val), ptr(cnt), ptr(self.leaf_of_row), ptr(margin), rows, tile,
                                 stream_handle(self.dev)), "mifx_gbdt_gpu_grow")
            return
        mask64 = 2 ** 64 - 1
        check(_fns()["grow_ex"](ptr(self.bins), self.n, self.f, ptr(self.nbins), ptr(self.hoff), self.hsize, ptr(g),
                                ptr(h), self.max_depth, float(min_child_weight), float(reg_lambda), float(gamma),
                                float(eta), ptr(self.ws), self.ws.numel(), ptr(fe), ptr(sb), ptr(dl), ptr(le),
                                ptr(ri), ptr(val), ptr(cnt), ptr(self.leaf_of_row), ptr(margin), rows, tile,
                                int(seed) & mask64, int(round) & mask64, thr, ptr(level_mask), int(_margin_route),
                                stream_handle(self.dev)), "mifx_gbdt_gpu_grow_ex")

    def apply(self, ebins: torch.Tensor, tree, emargin: torch.Tensor) -> None:
        """emargin += tree(row) for a binned row-major [m, f] matrix (upload_bins of the eval set)."""
        assert ebins.shape[1] == self.f and ebins.is_contiguous() and emargin.dtype == torch.float64
        assert len(emargin) == len(ebins) and emargin.is_contiguous()
        fe, sb, dl, le, ri, val, _ = tree
        check(_fns()["apply"](ptr(ebins), len(ebins), self.f, ptr(self.nbins), ptr(fe), ptr(sb), ptr(dl), ptr(le),
                              ptr(ri), ptr(val), self.max_depth, ptr(emargin), stream_handle(self.dev)),
              "mifx_gbdt_gpu_apply")


def grow_numpy(bins: np.ndarray, nbins: np.ndarray, g: np.ndarray, h: np.ndarray, max_depth: int,
               min_child_weight: float = 1.0, reg_lambda: float = 1.0, gamma: float = 0.0, eta: float = 0.3,
               device: int = 0, _rows_per_wg: int | None = None, _feat_tile: int | None = None, _booster=None,
               subsample: float = 1.0, seed: int = 0, round: int = 0, level_mask: np.ndarray | None = None,
               stats: bool = False):
    """One tree on the device from host arrays: (feature, split_bin, default_left, left, right, value, leaf_of_row),
    the outputs of the host's mifx_gbdt_grow_fixed (with subsample / level_mask: of mifx_gbdt_grow_fixed_ex on the
    rows sampled for (seed, round); level_mask is a host [max_depth, f] uint8 array). `stats`: the nodes' (gain, cover)
    of mifx_gbdt_grow_fixed_stats follow as an eighth and ninth array."""
    dev = device_for(device)
    with torch.cuda.device(dev):
        b = _booster or Booster(bins, nbins, max_depth, dev)
        trees = b.new_trees(1)
        tree = tuple(t[0] for t in trees)
        st = tuple(s[0] for s in b.new_stats(1)) if stats else None
        gd = torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(dev)
        hd = torch.from_numpy(np.ascontiguousarray(h, np.float32)).to(dev)
        lm = None if level_mask is None or max_depth == 0 else \
            torch.from_numpy(np.ascontiguousarray(level_mask, np.uint8).reshape(max_depth, -1)).to(dev)
        b.grow(gd, hd, tree, min_child_weight, reg_lambda, gamma, eta, None, _rows_per_wg, _feat_tile,
               subsample=subsample, seed=seed, round=round, level_mask=lm, stats=st)
        cnt = int(tree[6].item())
        out = tuple(t[:cnt].cpu().numpy() for t in tree[:6]) + (b.leaf_of_row.cpu().numpy(),)
        return out if st is None else out + tuple(s[:cnt].cpu().numpy() for s in st)
