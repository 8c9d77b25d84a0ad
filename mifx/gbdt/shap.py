"""Feature contributions of a forest on the host: the path table of csrc/gbdt_shap.h (built and validated by
mifx_gbdt_paths_build in csrc/gbdt.cpp) and path-dependent TreeSHAP from it (mifx_gbdt_contribs). The device route
(mifx/ops/gbdt_prep.py: DevicePaths, contribs) uploads the same table and returns the same bits."""
from __future__ import annotations

import ctypes
import functools

import numpy as np

REC_DTYPE = np.dtype([("a", np.float64), ("b", np.float64), ("c", np.float64), ("i", np.int32), ("j", np.int32)])
MAX_PATH = 12  # distinct features on one root-to-leaf path (MIFX_SHAP_MAX_PATH)

_ERRORS = {
    -1: "is not a tree (node arrays of one length >= 1, children with larger indices, one parent per node)",
    -2: "splits on a feature outside the table",
    -3: "has an inner node or a child of one whose cover is not finite and > 0 (a zero-weight child, as "
        "min_child_weight=0 allows): feature contributions divide by the cover ratios",
    -4: f"has a path with more than {MAX_PATH} distinct features",
    -5: "makes a path table of 2^31 records or more",
    -6: "has a NaN threshold",
}


@functools.lru_cache(maxsize=None)
def _fns():
    from .xgb import _D, _I, _U8, _lib

    lib = _lib()
    vp, lg = ctypes.c_void_p, ctypes.c_long
    lib.mifx_gbdt_paths_build.argtypes = [ctypes.c_int, _I, _I, _D, _U8, _I, _I, _D, _D, ctypes.c_int, vp, lg, _I, lg,
                                          _I, ctypes.POINTER(lg)]
    lib.mifx_gbdt_paths_build.restype = ctypes.c_int
    lib.mifx_gbdt_contribs.argtypes = [_D, lg, ctypes.c_int, vp, lg, ctypes.c_double, vp, lg, ctypes.c_int]
    lib.mifx_gbdt_contribs.restype = ctypes.c_int
    return lib.mifx_gbdt_paths_build, lib.mifx_gbdt_contribs


class PathTable:
    """Every leaf's root-to-leaf path of `trees` (6-tuples) with the nodes' `covers`, merged per feature: `recs`
    (REC_DTYPE), `leaf_off` [leaves + 1] (record offset of each leaf) and `tree_leaf` [trees + 1] (first leaf of each
    tree). Raises ValueError for a forest that contributions cannot be computed for."""

    def __init__(self, trees, covers, nfeat: int):
        from .xgb import _D, _I, _U8, _p

        if len(trees) != len(covers):
            raise ValueError("one cover array per tree is needed")
        for t, (tree, cv) in enumerate(zip(trees, covers)):
            c = len(tree[0])
            if c < 1 or any(len(a) != c for a in tree) or len(cv) != c:
                raise ValueError(f"tree {t} {_ERRORS[-1]}")
        self.n_trees, self.nfeat = len(trees), int(nfeat)
        off = np.concatenate([[0], np.cumsum([len(t[0]) for t in trees])]).astype(np.int64)
        if off[-1] >= 2 ** 31:
            raise ValueError("the forest holds 2^31 nodes or more")
        off = off.astype(np.int32)

        def cat(k, dt):
            parts = [np.asarray(t[k]) for t in trees] if k < 6 else [np.asarray(c) for c in covers]
            return np.ascontiguousarray(np.concatenate(parts + [np.zeros(1)]), dt)

        fe, le, ri = (cat(k, np.int32) for k in (0, 3, 4))
        thr, val, cov = (cat(k, np.float64) for k in (1, 5, 6))
        dl = cat(2, np.uint8)
        build, _ = _fns()
        info = (ctypes.c_long * 3)()

        def call(recs, leaf_off, tree_leaf):
            rc = build(self.n_trees, _p(off, _I), _p(fe, _I), _p(thr, _D), _p(dl, _U8), _p(le, _I), _p(ri, _I),
                       _p(val, _D), _p(cov, _D), self.nfeat, None if recs is None else recs.ctypes.data,
                       0 if recs is None else len(recs), None if recs is None else _p(leaf_off, _I),
                       0 if recs is None else len(leaf_off) - 1, None if recs is None else _p(tree_leaf, _I), info)
            if rc != 0:
                raise ValueError(f"tree {info[2]} {_ERRORS.get(rc, f'was refused ({rc})')}")

        call(None, None, None)  # the count pass (it validates everything)
        self.recs = np.zeros(max(1, info[0]), REC_DTYPE)
        self.leaf_off = np.zeros(info[1] + 1, np.int32)
        self.tree_leaf = np.zeros(self.n_trees + 1, np.int32)
        if self.n_trees:
            call(self.recs, self.leaf_off, self.tree_leaf)

    def n_recs(self, n_trees: int) -> int:
        """Records of the first n_trees trees."""
        return int(self.leaf_off[self.tree_leaf[n_trees]])


def contribs(table: PathTable, X: np.ndarray, n_trees: int, base: float, out: np.ndarray, threads: int) -> None:
    """out [n, >= f + 1] (a view with a row stride, unit column stride): the first n_trees trees' contributions per
    row of the float64 [n, f] table X, the bias (base plus the trees' mean outputs) in column f."""
    assert X.dtype == np.float64 and X.flags.c_contiguous and X.shape[1] == table.nfeat
    assert out.dtype == np.float64 and out.shape[0] == len(X) and out.shape[1] == table.nfeat + 1
    assert out.strides[1] == 8 and out.strides[0] % 8 == 0 and 0 <= n_trees <= table.n_trees
    if not len(X):
        return
    rc = _fns()[1](X.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), len(X), table.nfeat, table.recs.ctypes.data,
                   table.n_recs(n_trees), float(base), out.ctypes.data, out.strides[0] // 8, int(threads))
    if rc != 0:
        raise ValueError("the path table does not fit the feature table")
