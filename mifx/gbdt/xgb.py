"""XGBoost-style gradient-boosted trees: XGBRegressor / XGBClassifier on the native histogram learner of
csrc/gbdt.cpp (second-order split gain, learned missing-value directions, depth-wise growth).

Reference usage: `kubeflow-pipelines/fairing/fairing_xgboost.py:69-87` (XGBRegressor(n_estimators, learning_rate),
fit with `early_stopping_rounds` and `eval_set`, then `best_score`, `best_iteration`, `predict`). Semantics follow
XGBoost's scikit-learn API: the eval metric is RMSE (regression), logloss (two classes) or mlogloss (more) on the LAST
eval set; with early stopping, training stops after `early_stopping_rounds` rounds without improvement and
`predict` uses the trees up to `best_iteration` (XGBoost >= 1.4's default `iteration_range`). Defaults are
XGBoost >= 1.0's (learning_rate 0.3, max_depth 6, reg_lambda 1, min_child_weight 1, gamma 0, 256 bins); the
intercept is the training mean (regression) or its log-odds (classification), XGBoost 2's `base_score` estimate.

Classification: two classes train `binary:logistic`; K >= 3 classes train XGBoost's `multi:softprob` on all three
learners. A boosting round then grows K trees, one per class: `_trees` is round-major and class-minor (tree t belongs
to class t % K, XGBoost's layout), `n_trees_` counts trees, `n_estimators`, `best_iteration` and
`early_stopping_rounds` count rounds. Margins are float64 [K, n], class-major, every class starting from the same
intercept (`base_score` if given, else 0.5). All K gradient pairs come from the margins at the START of the round
(`XGBClassifier._softmax`, in double: p_k = exp(m_k - max) / sum in class order; g = p_k - [y = k],
h = max(2 p_k (1 - p_k), 1e-16), both float32), and the tree index t = round * K + k takes the round's place in every
draw, so each tree has its own sample. `predict_proba` is [n, K] in `classes_` order, `predict` the class of the largest
margin (ties to the lowest class); the eval metric is the unweighted mlogloss. `scale_pos_weight` is binary only.

`device="gpu"` (or "cuda", "cuda:N") trains on the device learner of csrc/gbdt_gpu.hip: gradients, fixed-point int64
histograms, split search, row partition and margin updates stay resident on the GPU for the whole fit; cuts and
binning run there too (csrc/gbdt_prep.hip, equal to the host functions bit for bit), so the table goes to the device
once -- or is there already: `fit` takes numpy arrays, CPU tensors or torch tensors on that GPU. `predict` runs where
its input is: numpy / CPU input on the host, a device tensor through the forest kernel on that tensor's device (any
model, also one trained on the host), returning a device tensor. `fixed_point=True` selects the fixed-point
semantics of csrc/gbdt_split.h (the GPU's only mode, the CPU's option): histograms are integer sums, so a model is bit-reproducible for any thread
count AND any launch geometry, and `device="cpu", fixed_point=True` is the host twin that reproduces a GPU-trained
model bit for bit. The default (`device=None`, double histograms on the host) is unchanged.

Stochastic boosting and instance weights, on all three learners (host double, host fixed point, device):
`subsample`, `colsample_bytree`, `colsample_bylevel` (each in (0, 1]), `fit(..., sample_weight=)` and the classifier's
`scale_pos_weight`. The draws are our own counter-based rule (csrc/gbdt_sample.h, numpy twin mifx/gbdt/sample.py),
not XGBoost's random stream: a pure function of `random_state`, the round and the row or feature index, so a model is
still a pure function of data, parameters and `random_state` -- independent of `n_jobs` and launch geometry, and the
GPU model equals the host twin bit for bit. A round's tree is grown on exactly the sampled rows, as if the table held
only them (quantisation exponents, the two-row leaf rule and row counts included); every row's margin then receives
the tree's output. Weights are float32 and multiply the float32 gradient pair; the intercept is the weighted mean (or
its log-odds). The eval metric stays unweighted (`sample_weight_eval_set` and `colsample_bynode` are not
implemented). With the defaults nothing is drawn and no weight is applied: the models are the unsampled ones.

What the model used: every learner records each node's `gain` (the double it maximised,
0.5 * (score_L + score_R - score_parent) - gamma, 0.0 at a leaf) and `cover` (the node's hessian sum, over the sampled
rows under `subsample`), kept beside the 6-tuples of `_trees` as `_node_stats[t] = (gain, cover)` and equal bit for bit
between the device and its host twin. XGBoost's `loss_chg` is 2 * (gain + gamma) of ours, so at gamma = 0 the normalised
importances are the same quantity. `get_score(importance_type)` and `feature_importances_` (constructor argument
`importance_type`, default "gain") are XGBoost's; `predict_contribs(X)` is its `pred_contribs`: exact path-dependent
TreeSHAP in margin space, on the host (csrc/gbdt.cpp) for host input and on the GPU (csrc/gbdt_prep.hip) for a device
tensor, the same bits. `pred_interactions` and approximate (Saabas) contributions are not implemented."""
from __future__ import annotations

import ctypes
import functools
import logging
import os
import sys

import numpy as np

_D = ctypes.POINTER(ctypes.c_double)
_F = ctypes.POINTER(ctypes.c_float)
_I = ctypes.POINTER(ctypes.c_int)
_U8 = ctypes.POINTER(ctypes.c_uint8)
_U16 = ctypes.POINTER(ctypes.c_uint16)


@functools.lru_cache(maxsize=None)
def _lib():
    from ..ops import _lib as L

    lib = L.load("gbdt")
    lib.mifx_gbdt_cuts.argtypes = [_D, ctypes.c_long, ctypes.c_long, ctypes.c_int, _D]
    lib.mifx_gbdt_bin.argtypes = [_D, ctypes.c_long, ctypes.c_int, _D, _I, _I, _U16, ctypes.c_int]
    lib.mifx_gbdt_grow.argtypes = [_U16, ctypes.c_long, ctypes.c_int, _I, _F, _F, ctypes.c_int, ctypes.c_double,
                                   ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                   _I, _I, _U8, _I, _I, _D, _I]
    lib.mifx_gbdt_predict.argtypes = [_D, ctypes.c_long, ctypes.c_int, ctypes.c_int, _I, _I, _D, _U8, _I, _I, _D,
                                      ctypes.c_double, _D, ctypes.c_int]
    lib.mifx_gbdt_grow_fixed.argtypes = lib.mifx_gbdt_grow.argtypes
    lib.mifx_gbdt_quant_exp.argtypes = [ctypes.c_double, ctypes.c_long]
    lib.mifx_gbdt_grow_ex.argtypes = lib.mifx_gbdt_grow.argtypes + [_I, ctypes.c_long, _U8]
    lib.mifx_gbdt_grow_fixed_ex.argtypes = lib.mifx_gbdt_grow_ex.argtypes
    lib.mifx_gbdt_grow_stats.argtypes = lib.mifx_gbdt_grow_ex.argtypes + [_D, _D]
    lib.mifx_gbdt_grow_fixed_stats.argtypes = lib.mifx_gbdt_grow_stats.argtypes
    u64 = ctypes.c_uint64
    lib.mifx_gbdt_sample_rows.argtypes = [u64, u64, ctypes.c_double, ctypes.c_long, _U8]
    lib.mifx_gbdt_sample_rows.restype = ctypes.c_long
    lib.mifx_gbdt_sample_features.argtypes = [u64, u64, u64, ctypes.c_double, _U8, ctypes.c_int, _U8]
    lib.mifx_gbdt_level_mask.argtypes = [u64, u64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _U8,
                                         _U8]
    for f in (lib.mifx_gbdt_cuts, lib.mifx_gbdt_bin, lib.mifx_gbdt_grow, lib.mifx_gbdt_predict,
              lib.mifx_gbdt_grow_fixed, lib.mifx_gbdt_quant_exp, lib.mifx_gbdt_grow_ex, lib.mifx_gbdt_grow_fixed_ex,
              lib.mifx_gbdt_sample_features, lib.mifx_gbdt_level_mask, lib.mifx_gbdt_grow_stats,
              lib.mifx_gbdt_grow_fixed_stats):
        f.restype = ctypes.c_int
    return lib


def _p(a: np.ndarray, t):
    return a.ctypes.data_as(t)


def _parse_device(device):
    """None / "cpu" -> None; "gpu" / "cuda" / "cuda:N" -> the GPU index."""
    if device is None or device == "cpu":
        return None
    if device in ("gpu", "cuda"):
        return 0
    if isinstance(device, str) and device.startswith("cuda:") and device[5:].isdigit():
        return int(device[5:])
    raise ValueError(f"device must be None, 'cpu', 'gpu', 'cuda' or 'cuda:N' (one GPU), got {device!r}")


def _is_tensor(x) -> bool:
    """A torch tensor, without importing torch (the default path never does)."""
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(x, getattr(torch, "Tensor", ()))


def _on_gpu(x) -> bool:
    return _is_tensor(x) and x.is_cuda


def _host(x) -> np.ndarray:
    """numpy view or copy of an array-like or of a tensor on any device."""
    return x.detach().cpu().numpy() if _is_tensor(x) else np.asarray(x)


def sample_rows(seed: int, round: int, subsample: float, n: int) -> np.ndarray:
    """Ascending int32 ids of the rows that csrc/gbdt_sample.h keeps for (seed, round)."""
    keep = np.empty(n, np.uint8)
    _lib().mifx_gbdt_sample_rows(int(seed) & _M64, int(round) & _M64, float(subsample), n, _p(keep, _U8))
    return np.flatnonzero(keep).astype(np.int32)


def level_mask(seed: int, round: int, f: int, max_depth: int, colsample_bytree: float, colsample_bylevel: float):
    """uint8 [max_depth, f] of csrc/gbdt_sample.h: the features each level of round `round`'s tree may split on."""
    mask, tree = np.empty((max_depth, f), np.uint8), np.empty(f, np.uint8)
    _lib().mifx_gbdt_level_mask(int(seed) & _M64, int(round) & _M64, f, max_depth, float(colsample_bytree),
                                float(colsample_bylevel), _p(tree, _U8), _p(mask, _U8))
    return mask


_M64 = (1 << 64) - 1


def _threads() -> int:
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))))


class _Base:
    _objective = "reg:squarederror"

    def __init__(self, n_estimators: int = 100, learning_rate: float = 0.3, max_depth: int = 6,
                 min_child_weight: float = 1.0, reg_lambda: float = 1.0, gamma: float = 0.0, max_bins: int = 256,
                 base_score: float | None = None, n_jobs: int | None = None, random_state: int = 0,
                 verbosity: int = 0, device: str | None = None, fixed_point: bool | None = None,
                 subsample: float = 1.0, colsample_bytree: float = 1.0, colsample_bylevel: float = 1.0,
                 importance_type: str = "gain"):
        self.n_estimators, self.learning_rate, self.max_depth = n_estimators, learning_rate, max_depth
        self.min_child_weight, self.reg_lambda, self.gamma, self.max_bins = min_child_weight, reg_lambda, gamma, max_bins
        self.base_score, self.n_jobs = base_score, n_jobs
        self.random_state, self.verbosity = random_state, verbosity  # random_state: the seed of every draw
        self.subsample, self.colsample_bytree, self.colsample_bylevel = subsample, colsample_bytree, colsample_bylevel
        self._check_rates()
        self.best_iteration, self.best_score, self.evals_result_ = None, None, {}
        self._trees: list[tuple] = []
        self._node_stats: list[tuple] = []  # per tree (gain, cover), parallel to _trees
        self.importance_type = importance_type
        self.device, self.fixed_point = device, fixed_point
        if _parse_device(device) is not None and fixed_point is not None and not fixed_point:
            raise ValueError("device='gpu' trains in fixed point only (fixed_point=False is the host's double learner)")

    def _rates(self):
        """(subsample, colsample_bytree, colsample_bylevel); 1.0 for a model pickled before they existed."""
        return tuple(float(getattr(self, k, 1.0)) for k in ("subsample", "colsample_bytree", "colsample_bylevel"))

    def _check_rates(self) -> None:
        for name, r in zip(("subsample", "colsample_bytree", "colsample_bylevel"), self._rates()):
            if not 0.0 < r <= 1.0:  # (a NaN fails too)
                raise ValueError(f"{name} must be in (0, 1], got {r}")

    def _seed(self) -> int:
        return int(getattr(self, "random_state", 0) or 0) & _M64

    def _weights(self, sample_weight, y: np.ndarray):
        """float32 [n] weights (None: unweighted), validated on the host before anything is launched."""
        if sample_weight is None:
            return None
        w = _host(sample_weight).reshape(-1)
        if len(w) != len(y):
            raise ValueError(f"sample_weight must hold one weight per row ({len(y)}), got {len(w)}")
        w = np.ascontiguousarray(w, np.float32)
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("sample_weight must be finite and non-negative")
        if not (w > 0).any():
            raise ValueError("sample_weight must not be all zero")
        return w

    def _round_draws(self, it: int, n: int, f: int):
        """(rows, level_mask) of boosting round `it`: None where nothing is drawn."""
        sub, bytree, bylevel = self._rates()
        rows = sample_rows(self._seed(), it, sub, n) if sub < 1.0 else None
        mask = level_mask(self._seed(), it, f, int(self.max_depth), bytree, bylevel) \
            if (bytree < 1.0 or bylevel < 1.0) and int(self.max_depth) > 0 else None
        return rows, mask

    def _gpu_index(self):
        return _parse_device(getattr(self, "device", None))

    def _fixed(self) -> bool:
        fp = getattr(self, "fixed_point", None)
        return self._gpu_index() is not None if fp is None else bool(fp)

    def _check_data_device(self, *arrays) -> None:
        """Data on a GPU must be on the model's GPU (and the model must have one)."""
        gpu = self._gpu_index()
        for a in arrays:
            if _on_gpu(a) and gpu is None:
                raise ValueError('the data is on a GPU: train it there with device="gpu" (or pass host arrays)')
            if _on_gpu(a) and a.device.index != gpu:
                raise ValueError(f"the data is on {a.device} but device={self.device!r} is GPU {gpu}")

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_dev_forest", None)  # the device copy of the trees: rebuilt on the next device predict
        state.pop("_paths", None)       # the path tables of predict_contribs and their device copies: rebuilt too
        state.pop("_dev_paths", None)
        return state

    # ---- loss (overridden by the classifier)
    def _base(self, y: np.ndarray, w: np.ndarray | None = None) -> float:
        return float(np.mean(y)) if w is None else float(np.average(y, weights=w.astype(np.float64)))

    def _intercept(self, y: np.ndarray, w: np.ndarray | None) -> float:
        """The margin every row starts from: base_score (as a margin) if given, else the objective's estimate."""
        if self.base_score is None:
            return self._base(y, w)
        if self._objective != "reg:squarederror":
            return float(np.log(self.base_score / (1 - self.base_score)))
        return float(self.base_score)

    def _num_class(self) -> int:
        """Margin rows per data row (= trees per boosting round): 1 but for the multi-class classifier."""
        return 1

    def _grad_hess(self, margin: np.ndarray, y: np.ndarray):
        return (margin - y).astype(np.float32), np.ones(len(y), np.float32)

    def _weighted_grad_hess(self, margin: np.ndarray, y: np.ndarray, w: np.ndarray | None):
        """The float32 pair times the float32 weight: one IEEE multiply each (what the device kernel does)."""
        g, h = self._grad_hess(margin, y)
        return (g, h) if w is None else (g * w, h * w)

    def _metric_name(self) -> str:
        return "rmse"

    def _metric(self, margin: np.ndarray, y: np.ndarray) -> float:
        return float(np.sqrt(np.mean((margin - y) ** 2)))

    def _check_y(self, y: np.ndarray) -> np.ndarray:
        return y.astype(np.float64)

    # ---- training
    def _bin_matrix(self, X: np.ndarray):
        lib, (n, f) = _lib(), X.shape
        cuts, offs, ncut = [], [0], []
        buf = np.empty(max(1, self.max_bins), np.float64)
        for j in range(f):
            m = lib.mifx_gbdt_cuts(_p(X[:, j:], _D), n, f, int(self.max_bins), _p(buf, _D))
            if m < 0:
                raise ValueError("max_bins must be in [2, 65535]")
            cuts.append(buf[:m].copy())
            ncut.append(m)
            offs.append(offs[-1] + m)
        self._cuts = cuts
        flat = np.concatenate(cuts) if offs[-1] else np.zeros(1)
        self._cut_flat = np.ascontiguousarray(flat, np.float64)
        self._cut_off = np.asarray(offs[:-1], np.int32)
        self._ncut = np.asarray(ncut, np.int32)
        bins = np.empty((f, n), np.uint16)
        lib.mifx_gbdt_bin(_p(X, _D), n, f, _p(self._cut_flat, _D), _p(self._cut_off, _I), _p(self._ncut, _I),
                          _p(bins, _U16), self._nthreads())
        return bins

    def _nthreads(self) -> int:
        return self.n_jobs if self.n_jobs and self.n_jobs > 0 else _threads()

    def _grow(self, bins, nbins, g, h, leaf_of_row, rows=None, level_mask=None):
        """One tree. rows (ascending int32 ids, None = all): the tree is grown on these rows only and leaf_of_row is
        -1 elsewhere; level_mask (uint8 [max_depth, f], None = all): the features each level may split on."""
        return self._grow_stats(bins, nbins, g, h, leaf_of_row, rows, level_mask)[0]

    def _grow_stats(self, bins, nbins, g, h, leaf_of_row, rows=None, level_mask=None):
        """(_grow's tree, (gain, cover)): the tree and its nodes' statistics (float64 [nodes] each)."""
        n = bins.shape[1]
        cap = 2 ** (self.max_depth + 1)
        fe, sb, left, right = (np.empty(cap, np.int32) for _ in range(4))
        dl = np.empty(cap, np.uint8)
        val = np.empty(cap, np.float64)
        gain, cover = np.empty(cap, np.float64), np.empty(cap, np.float64)
        grow = _lib().mifx_gbdt_grow_fixed_stats if self._fixed() else _lib().mifx_gbdt_grow_stats
        if rows is not None:
            rows = np.ascontiguousarray(rows, np.int32)
        if level_mask is not None:
            level_mask = np.ascontiguousarray(level_mask, np.uint8)
        cnt = grow(_p(bins, _U16), n, bins.shape[0], _p(nbins, _I), _p(g, _F), _p(h, _F),
                   int(self.max_depth), float(self.min_child_weight), float(self.reg_lambda),
                   float(self.gamma), float(self.learning_rate), self._nthreads(), cap, _p(fe, _I),
                   _p(sb, _I), _p(dl, _U8), _p(left, _I), _p(right, _I), _p(val, _D),
                   _p(leaf_of_row, _I), None if rows is None else _p(rows, _I), 0 if rows is None else len(rows),
                   None if level_mask is None else _p(level_mask, _U8), _p(gain, _D), _p(cover, _D))
        if cnt < 0:
            raise RuntimeError("tree exceeded its node capacity")
        thr = np.zeros(cnt, np.float64)
        for k in range(cnt):  # the split's cut value: bin <= b  <=>  x < cuts[b]
            if fe[k] >= 0:
                thr[k] = self._cuts[fe[k]][sb[k]]
        return ((fe[:cnt].copy(), thr, dl[:cnt].copy(), left[:cnt].copy(), right[:cnt].copy(), val[:cnt].copy()),
                (gain[:cnt].copy(), cover[:cnt].copy()))

    def fit(self, X, y, eval_set=None, early_stopping_rounds: int | None = None, verbose: bool = False, *,
            sample_weight=None):
        """Fit the boosted trees. With `device="gpu"`, X, y, the weights and the eval set may be numpy arrays, CPU
        tensors or torch tensors on that GPU (float32 means its exact widening to float64); the table is uploaded once
        if it is not there already, and its float64 form (8 n f bytes), the bins (2 n f bytes) and one column's sort
        scratch must fit on the device. Without a device, data on a GPU is refused. `sample_weight` (keyword only):
        one non-negative finite weight per row, used as float32; the eval metric stays unweighted."""
        self._dev_forest = self._paths = self._dev_paths = None
        gpu = self._gpu_index()
        self._check_rates()
        self._check_data_device(X, y, sample_weight, *(eval_set[-1] if eval_set else ()))
        y = self._check_y(_host(y).reshape(-1))
        X = X if _is_tensor(X) else np.asarray(X)
        if X.ndim != 2 or len(X) != len(y):
            raise ValueError("X must be [n, features] with one label per row")
        w = self._row_weights(self._weights(sample_weight, y), y)
        self._nfeat = X.shape[1]
        if gpu is not None:
            return self._fit_gpu(X, y, eval_set, early_stopping_rounds, verbose, w)
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        bins = self._bin_matrix(X)
        nbins = (self._ncut + 1).astype(np.int32)
        self._base_margin = self._intercept(y, w)
        # K margin rows, class-major: one for the regressor and the binary classifier, one per class for multi:softprob.
        # A round computes every row's gradients first, then grows tree `it * K + k` on row k; that tree index takes
        # the round's place in the draws (it IS the round for K = 1).
        K = self._num_class()
        margin = np.full((K, len(y)), self._base_margin)
        leaf_of_row = np.empty(len(y), np.int32)
        ev = None
        if eval_set:
            ex, ey = eval_set[-1]
            ex = np.ascontiguousarray(np.asarray(ex, dtype=np.float64))
            ey = self._check_y(np.asarray(ey).reshape(-1))
            ev_margin = np.full((K, len(ey)), self._base_margin)
            ev = (ex, ey, ev_margin)
        self._trees, self._node_stats = [], []
        best, best_it, since, hist = None, 0, 0, []
        for it in range(int(self.n_estimators)):
            g, h = self._weighted_grad_hess(margin if K > 1 else margin[0], y, w)
            g, h = g.reshape(K, -1), h.reshape(K, -1)
            for k in range(K):
                rows, mask = self._round_draws(it * K + k, len(y), self._nfeat)
                tree, stats = self._grow_stats(bins, nbins, g[k], h[k], leaf_of_row, rows, mask)
                self._trees.append(tree)
                self._node_stats.append(stats)
                if rows is None:
                    margin[k] += tree[5][leaf_of_row]
                else:  # rows outside the sample have no leaf_of_row: every row walks the tree (the same leaf values)
                    margin[k] += self._predict_trees(X, [tree], 0.0)
                if ev is not None:
                    ev[2][k] += self._predict_trees(ev[0], [tree], 0.0)
            if ev is not None:
                score = self._metric(ev[2] if K > 1 else ev[2][0], ev[1])
                hist.append(score)
                if verbose:
                    logging.info("[%d]\tvalidation_0-%s:%.5f", it, self._metric_name(), score)
                if best is None or score < best:
                    best, best_it, since = score, it, 0
                else:
                    since += 1
                    if early_stopping_rounds and since >= early_stopping_rounds:
                        break
        self.evals_result_ = {"validation_0": {self._metric_name(): hist}} if ev is not None else {}
        # XGBoost's sklearn API sets best_iteration / best_score only under early stopping; without it predict uses
        # every tree even when an eval_set was given
        self.best_score, self.best_iteration = (best, best_it) if ev is not None and early_stopping_rounds else \
            (None, None)
        return self

    def _row_weights(self, w, y):
        """The weights the learner uses (the classifier folds scale_pos_weight in)."""
        return w

    def _fit_gpu(self, X, y, eval_set, early_stopping_rounds, verbose, w=None):
        """The boosting loop on the device learner (mifx/ops/gbdt_gpu.py). The table is uploaded once (unless it is on
        the device already); cuts and binning run there (mifx/ops/gbdt_prep.py: the host's cuts and bins bit for bit,
        the cuts come back once for the trees' thresholds); then gradients, trees and margins stay on the GPU. With an
        eval set its margins come back once per round for the metric (the host's own numpy metric, so the scores are
        the host twin's bit for bit); the trees come back once at the end. Leaves the attributes of the host path.
        Sampling: the rows are drawn on the device inside the grower; the feature masks of all trees (pure functions
        of the seed, [trees, max_depth, f] bytes) are computed by the host and uploaded once before the first round.
        Multi-class: margins, g and h are [K, n] on the device; a round is one softmax gradient launch and K calls of
        the grower (and of the eval update), each on one class's row."""
        import torch

        from ..ops import gbdt_gpu as G
        from ..ops import gbdt_prep as P

        G.check_limits(len(y), int(self.max_bins), int(self.max_depth))
        if int(self.max_bins) < 2:
            raise ValueError("max_bins must be in [2, 65535]")
        dev = G.device_for(self._gpu_index())
        with torch.cuda.device(dev):
            Xd = P.as_device_matrix(X, dev)
            self._cuts, self._cut_flat, self._cut_off, self._ncut = P.device_cuts(Xd, int(self.max_bins))
            tables = P.CutTables(self._cut_flat, self._cut_off, self._ncut, dev)
            bins = P.device_bins(Xd, tables)
            del Xd
        nbins = (self._ncut + 1).astype(np.int32)
        self._base_margin = self._intercept(y, w)
        rounds, K = int(self.n_estimators), self._num_class()  # K trees per round, tree it * K + k on margin row k
        sub, bytree, bylevel = self._rates()
        masks = None
        if (bytree < 1.0 or bylevel < 1.0) and int(self.max_depth) > 0 and rounds > 0:
            masks = np.stack([level_mask(self._seed(), t, self._nfeat, int(self.max_depth), bytree, bylevel)
                              for t in range(rounds * K)])
        with torch.cuda.device(dev):
            bst = G.Booster.from_device_bins(bins, nbins, int(self.max_depth))
            yd = torch.from_numpy(y).to(dev)
            wd = None if w is None else torch.from_numpy(w).to(dev)
            masks = None if masks is None else torch.from_numpy(masks).to(dev)
            margin = torch.full((K, len(y)), self._base_margin, dtype=torch.float64, device=dev)
            g, h = (torch.empty((K, len(y)), dtype=torch.float32, device=dev) for _ in range(2))
            trees = bst.new_trees(max(1, rounds * K))
            stats = bst.new_stats(max(1, rounds * K))
            ev = None
            if eval_set:
                ex, ey = eval_set[-1]
                ex = ex if _is_tensor(ex) else np.asarray(ex)
                ey = self._check_y(_host(ey).reshape(-1))
                if ex.ndim != 2 or ex.shape[1] != self._nfeat or len(ex) != len(ey) or not len(ey):
                    raise ValueError(f"the eval set must be [m, {self._nfeat}] with one label per row")
                ev = (P.device_bins(P.as_device_matrix(ex, dev), tables), ey,
                      torch.full((K, len(ey)), self._base_margin, dtype=torch.float64, device=dev))
            best, best_it, since, hist, done = None, 0, 0, [], 0
            for it in range(rounds):
                if K > 1:  # every class's pair from the margins at the start of the round, one launch
                    G.grad_hess_softmax(margin, yd, g, h, wd)
                else:
                    G.grad_hess(self._objective, margin[0], yd, g[0], h[0], wd)
                for k in range(K):
                    tree = tuple(t[it * K + k] for t in trees)
                    bst.grow(g[k], h[k], tree, self.min_child_weight, self.reg_lambda, self.gamma, self.learning_rate,
                             margin[k], subsample=sub, seed=self._seed(), round=it * K + k,
                             level_mask=None if masks is None else masks[it * K + k],
                             stats=tuple(s[it * K + k] for s in stats))
                    if ev is not None:
                        bst.apply(ev[0], tree, ev[2][k])
                done = (it + 1) * K
                if ev is not None:
                    em = ev[2].cpu().numpy()  # the round's one read-back
                    score = self._metric(em if K > 1 else em[0], ev[1])
                    hist.append(score)
                    if verbose:
                        logging.info("[%d]\tvalidation_0-%s:%.5f", it, self._metric_name(), score)
                    if best is None or score < best:
                        best, best_it, since = score, it, 0
                    else:
                        since += 1
                        if early_stopping_rounds and since >= early_stopping_rounds:
                            break
            fe, sb, dl, le, ri, val, cnt = (t[:done].cpu().numpy() for t in trees)
            gain, cover = (s[:done].cpu().numpy() for s in stats)
        self._trees, self._node_stats = [], []
        for t in range(done):
            c = int(cnt[t])
            thr = np.zeros(c, np.float64)
            for k in range(c):  # the split's cut value: bin <= b  <=>  x < cuts[b]
                if fe[t, k] >= 0:
                    thr[k] = self._cuts[fe[t, k]][sb[t, k]]
            self._trees.append((fe[t, :c].copy(), thr, dl[t, :c].copy(), le[t, :c].copy(), ri[t, :c].copy(),
                                val[t, :c].copy()))
            self._node_stats.append((gain[t, :c].copy(), cover[t, :c].copy()))
        self.evals_result_ = {"validation_0": {self._metric_name(): hist}} if ev is not None else {}
        self.best_score, self.best_iteration = (best, best_it) if ev is not None and early_stopping_rounds else \
            (None, None)
        return self

    @property
    def n_trees_(self) -> int:
        return len(self._trees)

    # ---- prediction
    def _predict_trees(self, X: np.ndarray, trees, base: float) -> np.ndarray:
        X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
        if X.ndim != 2 or X.shape[1] != self._nfeat:
            raise ValueError(f"expected [n, {self._nfeat}] features")
        out = np.empty(len(X), np.float64)
        if not trees:
            out[:] = base
            return out
        off = np.cumsum([0] + [len(t[0]) for t in trees[:-1]]).astype(np.int32)
        fe, thr, dl, le, ri, val = (np.ascontiguousarray(np.concatenate([t[k] for t in trees])) for k in range(6))
        _lib().mifx_gbdt_predict(_p(X, _D), len(X), self._nfeat, len(trees), _p(off, _I), _p(fe, _I), _p(thr, _D),
                                 _p(dl, _U8), _p(le, _I), _p(ri, _I), _p(val, _D), float(base), _p(out, _D),
                                 self._nthreads())
        return out

    def _margin(self, X):
        """Margins where the data is: a tensor on a GPU goes through the forest kernel on that GPU and gives a tensor
        there (the host's bits); anything else takes the host path, which needs no GPU."""
        n = self._tree_limit()
        if _on_gpu(X):
            return self._margin_device(X, n)
        return self._predict_trees(_host(X) if _is_tensor(X) else X, self._trees[:n], self._base_margin)

    def _tree_limit(self) -> int:
        """Trees that predict uses: best_iteration counts rounds, a round holds _num_class() trees."""
        return len(self._trees) if self.best_iteration is None else (self.best_iteration + 1) * self._num_class()

    def _margin_device(self, X, n_trees: int, num_class: int = 1):
        """num_class > 1: the [num_class, n] margins of a multi-class forest, one walk for all classes."""
        from ..ops import gbdt_prep as P

        if X.dim() != 2 or X.shape[1] != self._nfeat:
            raise ValueError(f"expected [n, {self._nfeat}] features")
        cache = getattr(self, "_dev_forest", None)
        if cache is None:
            cache = self._dev_forest = {}
        if X.device.index not in cache:  # the packed trees, uploaded once per model and device (fit resets them)
            cache[X.device.index] = P.DeviceForest(self._trees, self._nfeat, X.device)
        Xd = P.as_device_matrix(X, X.device)
        if num_class > 1:
            return P.predict_multi(cache[X.device.index], Xd, self._base_margin, num_class, n_trees)
        return P.predict(cache[X.device.index], Xd, self._base_margin, n_trees)

    # ---- what the model used: importances and per-row contributions
    _IMPORTANCE_TYPES = ("weight", "gain", "cover", "total_gain", "total_cover")

    def _stats(self):
        """_node_stats, checked against _trees; a model without them (pickled before they were recorded, or with
        hand-assigned trees) still predicts and is refused here only."""
        stats = getattr(self, "_node_stats", None)
        if stats is None or len(stats) != len(self._trees) or \
                any(len(g) != len(t[0]) or len(c) != len(t[0]) for t, (g, c) in zip(self._trees, stats)):
            raise ValueError("this model holds no node statistics (gain and cover) for its trees: it was fitted before "
                             "they were recorded, or its trees were assigned by hand; refit it")
        return stats

    def _importance(self, importance_type: str) -> np.ndarray:
        """float64 [n_features] of one importance type over all trees (all classes' trees pooled); 0 where a feature
        never splits."""
        if importance_type not in self._IMPORTANCE_TYPES:
            raise ValueError(f"importance_type must be one of {self._IMPORTANCE_TYPES}, got {importance_type!r}")
        stats = self._stats()
        weight, gain, cover = (np.zeros(self._nfeat, np.float64) for _ in range(3))
        for (fe, *_), (g, c) in zip(self._trees, stats):
            inner = np.flatnonzero(np.asarray(fe) >= 0)
            np.add.at(weight, fe[inner], 1.0)
            np.add.at(gain, fe[inner], g[inner])
            np.add.at(cover, fe[inner], c[inner])
        if importance_type == "weight":
            return weight
        total = gain if importance_type.endswith("gain") else cover
        return total if importance_type.startswith("total_") else total / np.maximum(weight, 1.0)

    def get_score(self, importance_type: str = "weight") -> dict:
        """{"f<j>": value} for the features that split at least once, as XGBoost's Booster.get_score: "weight" the
        number of splits, "gain" / "cover" the average gain / cover of the feature's splits, "total_gain" /
        "total_cover" their sums. Our gain is the quantity the learner maximised, so XGBoost's loss_chg is
        2 * (gain + gamma) of it: with gamma = 0 the normalised importances are the same quantity."""
        score = self._importance(importance_type)
        used = self._importance("weight") > 0
        return {f"f{j}": float(score[j]) for j in np.flatnonzero(used)}

    @property
    def feature_importances_(self) -> np.ndarray:
        """float32 [n_features]: get_score(self.importance_type) normalised to sum 1 (all zero if no tree splits)."""
        score = self._importance(getattr(self, "importance_type", "gain"))
        total = score.sum()
        return (score / total if total > 0 else np.zeros_like(score)).astype(np.float32)

    def _path_tables(self, limit: int):
        """One path table (mifx/gbdt/shap.py) per margin row over the trees that predict uses, built once per model
        and tree limit. Raises ValueError for trees that contributions cannot be computed for (a zero-cover child)."""
        from . import shap

        cache = getattr(self, "_paths", None)
        if cache is None or cache[0] != limit:
            stats, K = self._stats(), self._num_class()
            cache = self._paths = (limit, [shap.PathTable(self._trees[k:limit:K], [s[1] for s in stats[k:limit:K]],
                                                           self._nfeat) for k in range(K)])
            self._dev_paths = None
        return cache[1]

    def predict_contribs(self, X, _recs_per_chunk: int | None = None, _route: str | None = None):
        """Per-row feature contributions in margin space (XGBoost's pred_contribs: path-dependent TreeSHAP):
        [n, f + 1], or [n, K, f + 1] for a K-class model; column j < f is feature j's Shapley value in the game whose
        value for a feature set S follows the row at nodes that split on S and averages both children by their cover
        elsewhere, column f the bias (the intercept plus every used tree's cover-weighted mean leaf); a row sums to
        its margin. The trees are predict's (best_iteration under early stopping; class k's are k, k + K, ...).

        numpy or CPU input gives a numpy array from the host function (threads: n_jobs, the same bits for any count);
        a tensor on a GPU gives a tensor there from the device kernel with the same bits, for any model. float32
        tables are widened exactly. The private arguments are the kernel's launch geometry. Raises ValueError for a
        model without node statistics and for a used tree with a zero-cover child (min_child_weight = 0 allows one)."""
        from . import shap

        K, limit, f = self._num_class(), self._tree_limit(), self._nfeat
        X = X if _is_tensor(X) else np.asarray(X)
        if X.ndim != 2 or X.shape[1] != f:
            raise ValueError(f"expected [n, {f}] features")
        tables = self._path_tables(limit)
        counts = [len(range(k, limit, K)) for k in range(K)]
        if _on_gpu(X):
            from ..ops import gbdt_prep as P

            torch = sys.modules["torch"]
            cache = getattr(self, "_dev_paths", None)
            if cache is None:
                cache = self._dev_paths = {}
            if X.device.index not in cache:  # the tables, uploaded once per model and device (fit resets them)
                cache[X.device.index] = [P.DevicePaths(t, X.device) for t in tables]
            Xd = P.as_device_matrix(X, X.device)
            out = torch.empty((len(Xd), K, f + 1), dtype=torch.float64, device=X.device)
            for k in range(K if len(Xd) else 0):  # one launch per class over the class's own table
                P.contribs(cache[X.device.index][k], Xd, self._base_margin, out[:, k, :], counts[k],
                           _recs_per_chunk, _route)
            return out[:, 0, :] if K == 1 else out
        X = np.ascontiguousarray(_host(X), dtype=np.float64)
        out = np.empty((len(X), K, f + 1), np.float64)
        for k in range(K):
            shap.contribs(tables[k], X, counts[k], self._base_margin, out[:, k, :], self._nthreads())
        return out[:, 0, :] if K == 1 else out


class XGBRegressor(_Base):
    """Squared-error regression (objective reg:squarederror)."""

    def predict(self, X):
        """Margins: a numpy array for host input, a tensor on the input's device for a tensor on a GPU."""
        return self._margin(X)


class XGBClassifier(_Base):
    """Classification: two classes train binary:logistic, K >= 3 classes multi:softprob (K trees per boosting round,
    tree t for class t % K). Labels are any sortable values (classes_ sorted)."""
    _objective = "binary:logistic"

    def __init__(self, *args, scale_pos_weight: float = 1.0, **kwargs):
        """The parameters of XGBRegressor, and scale_pos_weight (> 0): a factor on the weights of class-1 rows."""
        super().__init__(*args, **kwargs)
        self.scale_pos_weight = scale_pos_weight
        self._check_spw()

    def _check_spw(self) -> float:
        spw = float(getattr(self, "scale_pos_weight", 1.0))
        if not spw > 0.0 or not np.isfinite(spw):
            raise ValueError(f"scale_pos_weight must be > 0, got {spw}")
        return spw

    def _num_class(self) -> int:
        """K for K >= 3 classes (multi:softprob: K margin rows, K trees per round); 1 for binary:logistic, which is
        also what a model pickled before multi-class existed is."""
        k = len(getattr(self, "classes_", ()))
        return k if k >= 3 else 1

    def _row_weights(self, w, y):
        spw = self._check_spw()
        if spw == 1.0:
            return w
        if self._num_class() > 1:
            raise ValueError(f"scale_pos_weight is a binary parameter: with {self._num_class()} classes it must be 1, "
                             f"got {spw} (use sample_weight)")
        w = np.ones(len(y), np.float32) if w is None else w
        return np.where(y == 1.0, w * np.float32(spw), w).astype(np.float32)

    def _check_y(self, y: np.ndarray) -> np.ndarray:
        """Labels to what the loss reads: 0.0 / 1.0 (binary), the class index as a double (multi-class)."""
        if not hasattr(self, "classes_") or self._fitting:
            self.classes_ = np.unique(y)
        if len(self.classes_) >= 3:
            idx = np.minimum(np.searchsorted(self.classes_, y), len(self.classes_) - 1)
            if not (self.classes_[idx] == y).all():
                raise ValueError("the eval set holds labels that are not among the training labels (classes_)")
            return idx.astype(np.float64)
        return (np.searchsorted(self.classes_, y) == 1).astype(np.float64) if len(self.classes_) == 2 \
            else np.zeros(len(y))

    def fit(self, X, y, eval_set=None, early_stopping_rounds: int | None = None, verbose: bool = False, *,
            sample_weight=None):
        self._fitting = True
        self._check_spw()
        self._check_data_device(X, y, sample_weight, *(eval_set[-1] if eval_set else ()))
        y = _host(y).reshape(-1)
        self._check_y(y)  # classes from the training labels
        self._fitting = False
        return super().fit(X, y, eval_set, early_stopping_rounds, verbose, sample_weight=sample_weight)

    def _base(self, y: np.ndarray, w: np.ndarray | None = None) -> float:
        p = float(np.clip(super()._base(y, w), 1e-6, 1 - 1e-6))
        return float(np.log(p / (1 - p)))

    def _intercept(self, y: np.ndarray, w: np.ndarray | None) -> float:
        if self._num_class() == 1:
            return super()._intercept(y, w)
        # multi:softprob: one raw margin for every class (softmax is shift invariant: only raw margins see it)
        return float(self.base_score) if self.base_score is not None else 0.5

    @staticmethod
    def _softmax(margin: np.ndarray) -> np.ndarray:
        """p [K, n] from margins [K, n], in double: e_k = exp(m_k - max_k m_k), s = e_0 + e_1 + ... in this order,
        p_k = e_k / s. The one definition: gradients, mlogloss and predict_proba use it, and the device kernel
        k_grad_softmax (csrc/gbdt_gpu.hip) follows it operation for operation."""
        e = np.exp(margin - margin.max(0))
        s = e[0].copy()
        for k in range(1, len(e)):
            s += e[k]
        return e / s

    def _grad_hess(self, margin: np.ndarray, y: np.ndarray):
        if margin.ndim == 2:  # multi:softprob, margins [K, n], y the class index: XGBoost's softmax pair
            p = self._softmax(margin)
            onehot = (y == np.arange(len(margin), dtype=np.float64)[:, None]).astype(np.float64)
            return (p - onehot).astype(np.float32), np.maximum(2.0 * p * (1.0 - p), 1e-16).astype(np.float32)
        p = 1.0 / (1.0 + np.exp(-margin))
        return (p - y).astype(np.float32), np.maximum(p * (1 - p), 1e-16).astype(np.float32)

    def _metric_name(self) -> str:
        return "mlogloss" if self._num_class() > 1 else "logloss"

    def _metric(self, margin: np.ndarray, y: np.ndarray) -> float:
        if margin.ndim == 2:  # mlogloss from [K, m] margins
            p = self._softmax(margin)[y.astype(np.int64), np.arange(len(y))]
            return float(-np.mean(np.log(np.clip(p, 1e-15, 1 - 1e-15))))
        p = np.clip(1.0 / (1.0 + np.exp(-margin)), 1e-15, 1 - 1e-15)
        return float(-np.mean(y * np.log(p) + (1 - y) * np.log(1 - p)))

    def _margins(self, X):
        """Multi-class margins [K, n], class k from trees k, k + K, ... below the tree limit: numpy for host input
        (the per-class host walk), a device tensor for a tensor on a GPU (one walk of the forest kernel)."""
        K, limit = self._num_class(), self._tree_limit()
        if _on_gpu(X):
            return self._margin_device(X, limit, K)
        X = _host(X) if _is_tensor(X) else X
        return np.stack([self._predict_trees(X, self._trees[k:limit:K], self._base_margin) for k in range(K)])

    def predict_proba(self, X):
        """[n, K] probabilities, columns in classes_ order (K = 2 for binary:logistic): numpy for host input, a tensor
        on the input's device for a tensor on a GPU."""
        if self._num_class() > 1:
            m = self._margins(X)
            if not _is_tensor(m):
                return np.ascontiguousarray(self._softmax(m).T)
            torch = sys.modules["torch"]
            e = torch.exp(m - m.max(0).values)
            s = e[0].clone()
            for k in range(1, len(e)):
                s += e[k]
            return (e / s).t().contiguous()
        m = self._margin(X)
        if _is_tensor(m):
            torch = sys.modules["torch"]
            p1 = 1.0 / (1.0 + torch.exp(-m))
            return torch.stack([1 - p1, p1], 1)
        p1 = 1.0 / (1.0 + np.exp(-m))
        return np.stack([1 - p1, p1], 1)

    def predict(self, X) -> np.ndarray:
        """Labels, always a numpy array (classes_ may hold strings): for a device tensor, one read-back of the class
        index. Multi-class: the class of the largest margin (softmax is monotone, so it is the most probable class),
        ties to the lowest class."""
        if self._num_class() > 1:
            m = self._margins(X)
            if not _is_tensor(m):
                return self.classes_[np.argmax(m, 0)]
            torch = sys.modules["torch"]
            k = torch.arange(len(m), device=m.device)[:, None]  # the lowest class among the largest margins
            return self.classes_[_host(torch.where(m == m.max(0).values, k, len(m)).min(0).values)]
        return self.classes_[_host(self.predict_proba(X)[:, 1] > 0.5).astype(int)]
