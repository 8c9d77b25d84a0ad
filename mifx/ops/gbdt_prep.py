"""Feature preparation and prediction of mifx.gbdt on the device (csrc/gbdt_prep.hip): quantile cuts from sorted
columns, binning of the raw table into the learner's row-major [n, f] uint16 layout, and forest prediction on raw
features. Each equals its host function in csrc/gbdt.cpp exactly (mifx_gbdt_cuts, mifx_gbdt_bin, mifx_gbdt_predict).

Feature contributions (`DevicePaths`, `contribs`): path-dependent TreeSHAP from the path table that the host builds
(mifx/gbdt/shap.py), equal to the host's mifx_gbdt_contribs bit for bit.

The column sort is torch.sort on the device, one column at a time; everything else is the kernels of gbdt_prep.hip.
The private `_...` arguments are launch geometry: no result depends on them."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import I32, VP, check, ptr, sig, stream_handle

F64 = ctypes.c_double
LONG = ctypes.c_long
CUT_BLOCKS = 1024         # workgroups of the run-start count over one sorted column
ROWS_PER_WG = 1024        # rows one workgroup bins with one staging of its feature tile's cut tables
FEAT_TILE = 32            # features per workgroup: 32 * 255 cuts * 8 B = 65,280 B of LDS
NODES_PER_CHUNK = 2048    # packed nodes staged in LDS at a time: 2048 * 24 B = 48 KB

NODE_DTYPE = np.dtype([("v", np.float64), ("feature", np.int32), ("left", np.int32), ("right", np.int32),
                       ("default_left", np.int32)])


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("gbdt_prep")
    fns = {
        "max_bins": sig(lib, "mifx_gbdt_prep_max_bins", []),
        "max_feat_tile": sig(lib, "mifx_gbdt_prep_max_feat_tile", []),
        "max_chunk_nodes": sig(lib, "mifx_gbdt_prep_max_chunk_nodes", []),
        "node_bytes": sig(lib, "mifx_gbdt_prep_node_bytes", []),
        "cut_scratch_bytes": sig(lib, "mifx_gbdt_prep_cut_scratch_bytes", []),
        "cuts": sig(lib, "mifx_gbdt_prep_cuts", [VP, LONG, VP, I32, VP, VP, VP, I32, VP]),
        "bin": sig(lib, "mifx_gbdt_prep_bin", [VP, I32, LONG, I32, VP, VP, VP, VP, I32, I32, VP]),
        "predict": sig(lib, "mifx_gbdt_prep_predict", [VP, I32, LONG, I32, VP, VP, I32, F64, I32, VP, VP]),
        "reg_classes": sig(lib, "mifx_gbdt_prep_reg_classes", []),
        "predict_multi": sig(lib, "mifx_gbdt_prep_predict_multi", [VP, I32, LONG, I32, VP, VP, I32, I32, F64, I32, VP,
                                                                   I32, VP]),
        "contrib_rec_bytes": sig(lib, "mifx_gbdt_prep_contrib_rec_bytes", []),
        "contrib_min_chunk": sig(lib, "mifx_gbdt_prep_contrib_min_chunk", []),
        "contrib_max_lds": sig(lib, "mifx_gbdt_prep_contrib_max_lds", []),
        "contrib_threads": sig(lib, "mifx_gbdt_prep_contrib_threads", []),
        "contribs": sig(lib, "mifx_gbdt_prep_contribs", [VP, I32, LONG, I32, VP, VP, I32, F64, I32, I32, I32, VP, LONG,
                                                             VP]),
    }
    assert fns["node_bytes"]() == NODE_DTYPE.itemsize
    return fns


def is_tensor(x) -> bool:
    return isinstance(x, torch.Tensor)


def as_device_matrix(X, dev: torch.device) -> torch.Tensor:
    """A numpy array, CPU tensor or tensor on `dev` as a contiguous float32 / float64 tensor on `dev` (float32 stays
    float32: the kernels widen it exactly; every other dtype becomes float64, as np.asarray(X, float64) does)."""
    if not is_tensor(X):
        X = np.asarray(X)
        if X.dtype not in (np.float32, np.float64):
            X = X.astype(np.float64)
        X = torch.from_numpy(np.ascontiguousarray(X))
    X = X.detach()
    if X.is_cuda and X.device != dev:
        raise ValueError(f"the data is on {X.device} but the model's device is {dev}")
    if X.dtype not in (torch.float32, torch.float64):
        X = X.to(torch.float64)
    return X.to(dev).contiguous()


def _check_matrix(Xd: torch.Tensor) -> None:
    if not (Xd.is_cuda and Xd.dim() == 2 and Xd.is_contiguous() and Xd.dtype in (torch.float32, torch.float64)):
        raise ValueError("expected a contiguous [n, f] float32 / float64 tensor on the GPU")
    if not (1 <= Xd.shape[0] < 2 ** 31 and Xd.shape[1] >= 1):
        raise ValueError(f"the device path supports 1 <= n < 2^31 rows and f >= 1, got {tuple(Xd.shape)}")


def device_cuts(Xd: torch.Tensor, max_bins: int, _blocks: int | None = None):
    """Per-feature cut points of a device table [n, f]: (cuts, cut_flat, cut_off, ncut) as XGB*._bin_matrix sets
    them on the host -- a list of f float64 arrays, their concatenation (one zero if there is none), the int32
    offsets and counts. Each column is sorted by torch.sort (NaNs last), then one counting pass and max_bins - 1
    binary searches pick the cuts; they come back to the host in one read at the end."""
    _check_matrix(Xd)
    fns = _fns()
    max_bins, blocks = int(max_bins), int(_blocks or CUT_BLOCKS)
    if not 2 <= max_bins <= fns["max_bins"]():
        raise ValueError(f"max_bins must be in [2, {fns['max_bins']()}] on the device, got {max_bins}")
    if not 1 <= blocks <= 65535:
        raise ValueError("launch geometry out of range")
    n, f = Xd.shape
    dev = Xd.device
    with torch.cuda.device(dev):
        cuts = torch.zeros((f, max_bins - 1), dtype=torch.float64, device=dev)
        count = torch.zeros(f, dtype=torch.int32, device=dev)
        scratch = torch.empty(fns["cut_scratch_bytes"](), dtype=torch.uint8, device=dev)
        for j in range(f):
            col = Xd[:, j].contiguous().to(torch.float64)
            nan_count = torch.isnan(col).sum()
            srt = torch.sort(col).values
            check(fns["cuts"](ptr(srt), n, ptr(nan_count), max_bins, ptr(cuts[j]), ptr(count[j:]), ptr(scratch),
                              blocks, stream_handle(dev)), "mifx_gbdt_prep_cuts")
        ncut = count.cpu().numpy()
        table = cuts.cpu().numpy()
    out = [table[j, :ncut[j]].copy() for j in range(f)]
    offs = np.concatenate([[0], np.cumsum(ncut)])
    flat = np.concatenate(out) if offs[-1] else np.zeros(1)
    return out, np.ascontiguousarray(flat, np.float64), offs[:-1].astype(np.int32), ncut.astype(np.int32)


class CutTables:
    """The flat per-feature cut table on the device (checked once on the host: the kernel trusts it)."""

    def __init__(self, cut_flat: np.ndarray, cut_off: np.ndarray, ncut: np.ndarray, dev: torch.device):
        flat = np.ascontiguousarray(cut_flat, np.float64)
        off, cnt = np.ascontiguousarray(cut_off, np.int32), np.ascontiguousarray(ncut, np.int32)
        if len(off) != len(cnt) or not len(cnt):
            raise ValueError("cut_off and ncut must hold one entry per feature")
        if cnt.min() < 0 or cnt.max() > _fns()["max_bins"]() - 1 or off.min() < 0 or \
                (off.astype(np.int64) + cnt).max() > len(flat):
            raise ValueError(f"cut tables must lie inside cut_flat with at most {_fns()['max_bins']() - 1} cuts each")
        self.f, self.dev = len(cnt), dev
        self.flat, self.off, self.ncut = (torch.from_numpy(a).to(dev) for a in (flat, off, cnt))


def device_bins(Xd: torch.Tensor, tables: CutTables, _rows_per_wg: int | None = None,
                _feat_tile: int | None = None) -> torch.Tensor:
    """Row-major [n, f] bins (int16 storage of the uint16 bits, Booster.bins' layout) of a device table: the number of
    cuts <= x, NaN -> 0xFFFF."""
    _check_matrix(Xd)
    n, f = Xd.shape
    if f != tables.f or Xd.device != tables.dev:
        raise ValueError(f"expected [n, {tables.f}] features on {tables.dev}")
    rows, tile = int(_rows_per_wg or ROWS_PER_WG), int(_feat_tile or FEAT_TILE)
    if not 1 <= rows <= 2 ** 20 or not 1 <= tile <= _fns()["max_feat_tile"]() or (f + tile - 1) // tile > 65535:
        raise ValueError("launch geometry out of range")
    with torch.cuda.device(Xd.device):
        bins = torch.empty((n, f), dtype=torch.int16, device=Xd.device)
        check(_fns()["bin"](ptr(Xd), int(Xd.dtype == torch.float64), n, f, ptr(tables.flat), ptr(tables.off),
                            ptr(tables.ncut), ptr(bins), rows, tile, stream_handle(Xd.device)), "mifx_gbdt_prep_bin")
    return bins


def validate_forest(trees, nfeat: int) -> None:
    """Raise ValueError unless every tree (feature, thr, default_left, left, right, value) is walkable: arrays of one
    length >= 1, feature < nfeat, and for an inner node k (feature >= 0) k < left, right < node count. Children with
    larger indices make every walk end within the tree's node count."""
    for t, (fe, thr, dl, le, ri, val) in enumerate(trees):
        fe, le, ri = (np.asarray(a).astype(np.int64) for a in (fe, le, ri))
        c = len(fe)
        if c < 1 or not (len(thr) == len(dl) == len(le) == len(ri) == len(val) == c):
            raise ValueError(f"tree {t}: the node arrays must have one length >= 1")
        if fe.max() >= nfeat:
            raise ValueError(f"tree {t}: feature index {int(fe.max())} >= {nfeat} features")
        k = np.flatnonzero(fe >= 0)
        if ((le[k] <= k) | (le[k] >= c) | (ri[k] <= k) | (ri[k] >= c)).any():
            raise ValueError(f"tree {t}: an inner node's children must have indices in (node, {c})")


class DeviceForest:
    """A model's trees in the packed node format of gbdt_prep.hip on one device, validated on the host first."""

    def __init__(self, trees, nfeat: int, dev: torch.device):
        validate_forest(trees, nfeat)
        sizes = [len(t[0]) for t in trees]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        if off[-1] >= 2 ** 31:
            raise ValueError("the forest holds 2^31 nodes or more")
        nodes = np.zeros(max(1, int(off[-1])), NODE_DTYPE)
        for t, (fe, thr, dl, le, ri, val) in enumerate(trees):
            nd = nodes[off[t]:off[t + 1]]
            nd["feature"], nd["left"], nd["right"], nd["default_left"] = fe, le, ri, dl
            nd["v"] = np.where(np.asarray(fe) >= 0, thr, val)
        self.n_trees, self.nfeat, self.dev = len(trees), int(nfeat), dev
        self.nodes = torch.from_numpy(nodes.view(np.uint8)).to(dev)
        self.tree_off = torch.from_numpy(off.astype(np.int32)).to(dev)


def predict(forest: DeviceForest, Xd: torch.Tensor, base: float, n_trees: int | None = None,
            _nodes_per_chunk: int | None = None) -> torch.Tensor:
    """base + the sum of the first n_trees trees' outputs (all by default) per row of a device table: float64 [n] on
    the device, the bits of the host's mifx_gbdt_predict (trees in order, one double per row)."""
    _check_matrix(Xd)
    n, f = Xd.shape
    if f != forest.nfeat or Xd.device != forest.dev:
        raise ValueError(f"expected [n, {forest.nfeat}] features on {forest.dev}")
    n_trees = forest.n_trees if n_trees is None else int(n_trees)
    chunk = int(_nodes_per_chunk or NODES_PER_CHUNK)
    if not 0 <= n_trees <= forest.n_trees:
        raise ValueError(f"n_trees must be in [0, {forest.n_trees}]")
    if not 1 <= chunk <= _fns()["max_chunk_nodes"]():
        raise ValueError("launch geometry out of range")
    with torch.cuda.device(Xd.device):
        out = torch.empty(n, dtype=torch.float64, device=Xd.device)
        check(_fns()["predict"](ptr(Xd), int(Xd.dtype == torch.float64), n, f, ptr(forest.nodes),
                                ptr(forest.tree_off), n_trees, float(base), chunk, ptr(out),
                                stream_handle(Xd.device)), "mifx_gbdt_prep_predict")
    return out


def _class_major(forest: DeviceForest, num_class: int):
    """The forest's nodes regrouped by class (class k's trees k, k + num_class, ... side by side), their offsets and
    the position of every class's first tree: what k_predict needs to walk one class. Built on the device from the
    packed forest, once per forest and num_class."""
    cache = forest.__dict__.setdefault("_by_class", {})
    if num_class not in cache:
        off = forest.tree_off.cpu().numpy().astype(np.int64)
        per_class = [np.arange(k, forest.n_trees, num_class) for k in range(num_class)]
        order = np.concatenate(per_class)
        new_off = np.concatenate([[0], np.cumsum((off[1:] - off[:-1])[order])])
        idx = np.concatenate([np.arange(off[t], off[t + 1]) for t in order] + [np.zeros(0, np.int64)])
        nodes = forest.nodes.view(-1, NODE_DTYPE.itemsize)[torch.from_numpy(idx).to(forest.dev)].contiguous()
        first = np.concatenate([[0], np.cumsum([len(c) for c in per_class])])
        cache[num_class] = (nodes, torch.from_numpy(new_off.astype(np.int32)).to(forest.dev), first)
    return cache[num_class]


def predict_multi(forest: DeviceForest, Xd: torch.Tensor, base: float, num_class: int, n_trees: int | None = None,
                  _nodes_per_chunk: int | None = None, _route: str | None = None) -> torch.Tensor:
    """Multi-class margins of a device table: float64 [num_class, n] on the device, row k = base + the outputs of
    trees k, k + num_class, ... below n_trees (all by default), added in that order -- the bits of the host's
    mifx_gbdt_predict over the class's own trees. Class-major, because a wave's 64 rows are then 64 consecutive doubles
    of one class (coalesced stores) and because it is the layout of the training margins.

    `_route` (the result does not depend on it; the default is the faster one measured, profiles/gbdt_multiclass.md):
      "registers"  ONE walk of the forest, the class sums in registers: num_class <= 16, the default there
      "launches"   one launch of the single-output kernel per class over a class-major copy of the forest (made once
                   per forest): the default for more classes
      "output"     one walk, every thread accumulating in its own elements of the output: any num_class"""
    _check_matrix(Xd)
    n, f = Xd.shape
    if f != forest.nfeat or Xd.device != forest.dev:
        raise ValueError(f"expected [n, {forest.nfeat}] features on {forest.dev}")
    n_trees = forest.n_trees if n_trees is None else int(n_trees)
    num_class, chunk = int(num_class), int(_nodes_per_chunk or NODES_PER_CHUNK)
    if num_class < 1:
        raise ValueError(f"num_class must be >= 1, got {num_class}")
    if not 0 <= n_trees <= forest.n_trees:
        raise ValueError(f"n_trees must be in [0, {forest.n_trees}]")
    if not 1 <= chunk <= _fns()["max_chunk_nodes"]():
        raise ValueError("launch geometry out of range")
    fits = num_class <= _fns()["reg_classes"]()
    route = ("registers" if fits else "launches") if _route is None else _route
    if route not in ("registers", "launches", "output"):
        raise ValueError(f"unknown route {route!r}")
    if route == "registers" and not fits:
        raise ValueError(f"the register route holds at most {_fns()['reg_classes']()} classes")
    is64, stream = int(Xd.dtype == torch.float64), stream_handle(Xd.device)
    with torch.cuda.device(Xd.device):
        out = torch.empty((num_class, n), dtype=torch.float64, device=Xd.device)
        if route == "launches":
            nodes, tree_off, first = _class_major(forest, num_class)
            for k in range(num_class):  # class k's trees below n_trees are a prefix of its block
                check(_fns()["predict"](ptr(Xd), is64, n, f, ptr(nodes), VP(tree_off.data_ptr() + 4 * int(first[k])),
                                        len(range(k, n_trees, num_class)), float(base), chunk,
                                        VP(out.data_ptr() + 8 * k * n), stream), "mifx_gbdt_prep_predict")
            return out
        check(_fns()["predict_multi"](ptr(Xd), is64, n, f, ptr(forest.nodes), ptr(forest.tree_off), n_trees, num_class,
                                      float(base), chunk, ptr(out), int(route == "registers"), stream),
              "mifx_gbdt_prep_predict_multi")
    return out


RECS_PER_CHUNK = 256      # path records staged in LDS at a time: 256 * 32 B = 8 KB (profiles/gbdt_contribs.md)


class DevicePaths:
    """A host path table (mifx.gbdt.shap.PathTable: built and validated on the host) on one device."""

    def __init__(self, table, dev: torch.device):
        fns = _fns()
        assert fns["contrib_rec_bytes"]() == table.recs.dtype.itemsize
        self.table, self.nfeat, self.n_trees, self.dev = table, table.nfeat, table.n_trees, dev
        self.recs = torch.from_numpy(table.recs.view(np.uint8).reshape(-1)).to(dev)
        self.leaf_off = torch.from_numpy(table.leaf_off).to(dev)


def contrib_lds_threads(f: int, chunk: int | None = None) -> int:
    """The largest workgroup (256, 128 or 64 threads) whose f sums per thread fit in LDS beside a chunk of the table;
    0 if none does."""
    fns = _fns()
    room = fns["contrib_max_lds"]() - int(chunk or RECS_PER_CHUNK) * fns["contrib_rec_bytes"]()
    return next((t for t in (fns["contrib_threads"](), 128, 64) if f * t * 8 <= room), 0)


def contribs(paths: DevicePaths, Xd: torch.Tensor, base: float, out: torch.Tensor, n_trees: int | None = None,
             _recs_per_chunk: int | None = None, _route: str | None = None, _threads: int | None = None) -> None:
    """Feature contributions (path-dependent TreeSHAP) of the first n_trees trees of `paths` per row of a device
    table, written into `out` [n, f + 1] (float64 on the device; a view with any row stride and unit column stride,
    so a class's slice of [n, K, f + 1] works): columns 0 .. f - 1 the features, column f the bias. The bits of the
    host's mifx_gbdt_contribs.

    `_recs_per_chunk` (records of the path table staged in LDS at a time, at least 13) and `_route` ("lds": a row's
    sums live in LDS and are stored once, the default when they fit; "output": they live in the output row) and
    `_threads` (64, 128 or 256 per workgroup; by default the most that fit) are launch geometry: the result does not
    depend on them."""
    _check_matrix(Xd)
    n, f = Xd.shape
    if f != paths.nfeat or Xd.device != paths.dev:
        raise ValueError(f"expected [n, {paths.nfeat}] features on {paths.dev}")
    if not (out.dtype == torch.float64 and out.device == Xd.device and tuple(out.shape) == (n, f + 1)
            and out.stride(1) == 1 and out.stride(0) >= f + 1):
        raise ValueError(f"out must be a float64 [n, {f + 1}] tensor on {Xd.device} with unit column stride")
    fns = _fns()
    n_trees = paths.n_trees if n_trees is None else int(n_trees)
    chunk = int(_recs_per_chunk or RECS_PER_CHUNK)
    if not 0 <= n_trees <= paths.n_trees:
        raise ValueError(f"n_trees must be in [0, {paths.n_trees}]")
    if chunk < fns["contrib_min_chunk"]() or chunk * fns["contrib_rec_bytes"]() > fns["contrib_max_lds"]():
        raise ValueError("launch geometry out of range")
    fits = contrib_lds_threads(f, chunk)
    route = ("lds" if fits else "output") if _route is None else _route
    if route not in ("lds", "output"):
        raise ValueError(f"unknown route {route!r}")
    threads = int(_threads or (fits if route == "lds" else fns["contrib_threads"]()))
    if threads not in (64, 128, fns["contrib_threads"]()) or (route == "lds" and threads > fits):
        raise ValueError(f"{f} sums per row of {threads} threads do not fit in LDS beside a chunk of {chunk} records")
    with torch.cuda.device(Xd.device):
        check(fns["contribs"](ptr(Xd), int(Xd.dtype == torch.float64), n, f, ptr(paths.recs), ptr(paths.leaf_off),
                              int(paths.table.tree_leaf[n_trees]), float(base), chunk, threads, int(route == "lds"), ptr(out),
                              out.stride(0), stream_handle(Xd.device)), "mifx_gbdt_prep_contribs")
