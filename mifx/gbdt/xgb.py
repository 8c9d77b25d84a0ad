"""XGBoost-style gradient-boosted trees: XGBRegressor / XGBClassifier on the native histogram learner of
csrc/gbdt.cpp (second-order split gain, learned missing-value directions, depth-wise or leaf-wise growth).

Reference usage: `kubeflow-pipelines/fairing/fairing_xgboost.py:69-87` (XGBRegressor(n_estimators, learning_rate),
fit with `early_stopping_rounds` and `eval_set`, then `best_score`, `best_iteration`, `predict`). Semantics follow
XGBoost's scikit-learn API: the eval metric is RMSE (regression), logloss (two classes) or mlogloss (more), or the
classifier's `eval_metric="auc"` (below), on the LAST eval set; with early stopping, training stops after `early_stopping_rounds` rounds without improvement and
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
its log-odds). The eval metric stays unweighted (`sample_weight_eval_set` is not implemented).
`interaction_constraints` (groups of feature indices) and `colsample_bynode` give every node its own feature set, the
rule of csrc/gbdt_nodeset.h: a node below the root may split on its path's features and on the groups that hold all of
them, intersected with a per-node draw from its level set keyed by (random_state, tree index, node index); on the GPU
the sets are made on the device (k_nodeset) and the model equals the fixed-point host twin bit for bit. With the defaults nothing is drawn and no weight is applied: the models are the unsampled ones.

What the model used: every learner records each node's `gain` (the double it maximised,
0.5 * (score_L + score_R - score_parent) - gamma, 0.0 at a leaf) and `cover` (the node's hessian sum, over the sampled
rows under `subsample`), kept beside the 6-tuples of `_trees` as `_node_stats[t] = (gain, cover)` and equal bit for bit
between the device and its host twin. XGBoost's `loss_chg` is 2 * (gain + gamma) of ours, so at gamma = 0 the normalised
importances are the same quantity. `get_score(importance_type)` and `feature_importances_` (constructor argument
`importance_type`, default "gain") are XGBoost's; `predict_contribs(X)` is its `pred_contribs`: exact path-dependent
TreeSHAP in margin space, on the host (csrc/gbdt.cpp) for host input and on the GPU (csrc/gbdt_prep.hip) for a device
tensor, the same bits. `predict_interactions(X)` is its `pred_interactions`: the (f + 1) x (f + 1) SHAP interaction
values per row from the same path tables, one conditioned pass per feature over the leaves that hold it, on the host
(mifx_gbdt_interactions) or on the GPU (csrc/gbdt_interactions.hip), the same bits. Approximate (Saabas)
contributions are not implemented.

Growth policy, on all three learners: `grow_policy="depthwise"` (the default: level by level to `max_depth`) or
XGBoost's `grow_policy="lossguide"` with a leaf budget `max_leaves` >= 2 (LightGBM's default rule): the open leaf with
the largest gain is split next, ties to the lowest node id, until `max_leaves` leaves exist or no leaf has a split
left; children take the next two node ids, left then right, so tree arrays hold at most 2 * max_leaves - 1 nodes.
`max_depth=0` then means no depth limit, `max_depth > 0` also closes a node at that depth. A node's candidate split
is the depth-wise learners' (same histograms, same scan, same leaf test), so the tree is the best-first prefix of the
depth-wise tree with the same depth limit, and with a budget that does not bind (`max_leaves = 2 ** max_depth`) every
row gets the same leaf value. On the GPU (csrc/gbdt_lossguide.hip) a tree is max_leaves - 1 expansions of four
launches, each histogramming only the smaller child and subtracting it from the parent's histogram in place (exact in
int64, so the host twin `device="cpu", fixed_point=True` still equals the GPU model bit for bit); limits there:
`max_leaves <= 4096`, `max_depth` 0 or <= 12. `max_leaves` under depth-wise growth and `colsample_bylevel < 1` under
lossguide raise ValueError. Prediction, contributions and interactions walk child indices and do not change;
TreeSHAP's limit of 12 distinct features on a path applies to deep chains too.

Monotone predictions, on all three learners, both growth policies and all three estimators:
`monotone_constraints` is a sequence of one direction per feature in {-1, 0, +1}, or a dict {feature index: direction}
(0 elsewhere); None or all zeros is unconstrained and takes the code paths and gives the bits it always did. The rule has
one copy (csrc/gbdt_split.h): every node carries an interval [lo, hi] of weights, the root's unbounded; a weight is
-G / (H + lambda) clamped into it and a leaf holds learning_rate times that; gains use the score
-(2 G w + (H + lambda) w w) with clamped weights for parent and children; a candidate on a +1 feature with wl > wr (-1:
wl < wr) is dropped; the children of a split on a constrained feature divide the interval at (wl + wr) / 2. So the
margin never falls (+1) or rises (-1) when the feature rises, exactly, for every setting of the other features, NaN
included. Candidate order and tie rules are the unconstrained ones. On the GPU: k_split_mono / k_decide_mono
(csrc/gbdt_gpu.hip) and k_split_mono (csrc/gbdt_lossguide.hip), equal to the host twin bit for bit. With
reg:absoluteerror / reg:quantileerror the refreshed leaves would need clamping to their intervals: not implemented,
ValueError. A wrong length, a value outside {-1, 0, 1} or a non-integer raises ValueError before the first round.

Robust loss and prediction intervals, on all three learners: `XGBRegressor(objective="reg:absoluteerror")` and
`objective="reg:quantileerror", quantile_alpha=a` (one scalar a in (0, 1); absolute error is a = 0.5), XGBoost's
objectives with its "adaptive tree". With d = margin - y in double the pair is g = +1 / 0 / -1 for d > 0 / = 0 / < 0
(absolute error) or g = float32(1 - a) for d >= 0 and float32(-a) below (quantile error), h = 1.0f, each times the
float32 weight as above; the unchanged growers grow the tree from these pairs. The hessian is constant, so the Newton
leaf value means nothing: once the tree is complete, and before any margin moves, every leaf is REFRESHED to
learning_rate times the weighted lower a-quantile of the residuals r_i = y_i - margin_i (double) of the rows in it.
The rule (csrc/gbdt_quantile.h, the one copy for host and device) is exact: row i weighs the integer q_i, its hessian
quantised by the fixed-point rule with the exponent of the tree's rows (the integers the fixed-point histograms
summed; the double learner quantises for the refresh only); a leaf's Q is the sum of its q_i over the sampled rows,
T = ceil(a * (double)Q) clamped to [1, Q], and the quantile is the smallest residual r of the leaf whose rows with
r_i <= r weigh at least T (numeric order, -0.0 before +0.0). A leaf with Q = 0 keeps the grower's value. Then every
row's margin, sampled or not, and the eval set's receive the refreshed tree's output. XGBoost interpolates between two
neighbouring residuals in the unweighted case; ours is the lower of them, so a leaf value differs from XGBoost's by
less than learning_rate times one gap between adjacent residuals of the leaf. Sums and comparisons are on integers,
so the GPU (csrc/gbdt_quantile.hip: a segmented weighted radix select over the leaves, nothing read back) equals the
host twin bit for bit, for any launch geometry. With `base_score=None` the intercept is the same lower weighted
a-quantile of y (float32 weights accumulated in double over the sorted labels). The eval metric is "mae" or "quantile"
(the mean pinball loss at a), unweighted. `gain` and `cover` stay the grower's. Several quantiles in one model,
XGBoost's interpolation and reg:pseudohubererror are not implemented.

Learning to rank, on all three learners: `XGBRanker(objective="rank:ndcg" | "rank:pairwise")`, LambdaMART over query
groups given to `fit` as `qid` (non-decreasing, one per row) or `group` (sizes). The gradient pair is not a row's own:
inside a group the rows are ranked by margin, descending (on the integer key of csrc/gbdt_sort_key.h, ties to the
lower row), and every pair (i, j) with label_i > label_j adds, with s = m_i - m_j and rho = 1 / (1 + exp(s)),
lambda = rho * delta to g_j and -lambda to g_i, and eta = 2 max(rho (1 - rho), 1e-16) delta to both hessians; delta is
1 (rank:pairwise) or |(2^l_i - 2^l_j) (D[r_i] - D[r_j])| / IDCG with D[r] = 1 / log2(r + 2) (rank:ndcg). Labels are
integers in [0, 31]. `lambdarank_pair_method="all"` (our default) counts every such pair, "topk" with
`lambdarank_num_pair_per_sample=k` those with a row ranked above k. The rule has one copy, csrc/gbdt_rank.h: a row's
sums run in double over its partners in rank order, so they depend on no thread count or launch geometry; the host
function is `rank_grad` (mifx_gbdt_rank_grad), the device path csrc/gbdt_rank.hip (one wave per group of up to 64 rows,
one workgroup with a bitonic sort in LDS per group of up to 4096; a longer group raises ValueError on the device, there
is no host fallback). Host and device differ only in exp (a few double ulps per term): the first tree, grown from
equal margins, is equal bit for bit, later ones are not promised to be. Everything downstream is unchanged: sampling,
both growth policies, `predict` (margins), contributions, interactions and importances. The intercept is `base_score`
or 0.0. The eval metric is "ndcg" or "ndcg@k" (the mean over groups, a group without a relevant row scores 1.0) and is
MAXIMISED by early stopping. The host function is `ndcg`; with device="gpu" the eval margins are NOT read back:
mifx/ops/gbdt_ndcg.py scores the groups in csrc/gbdt_ndcg.hip -- one wave per group of up to 64 rows; a longer group, of
any size, in tiles of 256 rows that COUNT each row's rank against the group's keys streamed through LDS, so the
gradient path's 4096-row limit does not apply to eval groups -- with the discount table and the per-group IDCG
(`ndcg_idcg`, computed once per fit) uploaded by the host, and one double per group comes back per round, their mean
taken by `ndcg_mean`, the host function's own expression. Every term is one IEEE multiply and every sum one IEEE add
per term in rank order, so the history is the host's bit for bit, for any launch geometry. Limits of the device
metric: fewer than 2^31 eval rows; counting is O(m^2) per group, so with an eval group of more than
mifx.ops.gbdt_ndcg.max_group() = 2^20 rows (the largest size measured, profiles/gbdt_ndcg.md) the fit keeps the host
path, the same scores. Not implemented: group and row weights (`sample_weight` raises), rank:map,
`lambdarank_normalization` and XGBoost's score-difference normalisation, "mean" pair sampling (XGBoost's default pair
method is "topk": pass it explicitly to follow it), unbiased LambdaMART.

Validation AUC, on all three learners: `XGBClassifier(eval_metric="auc")`; `eval_metric=None` (the default) keeps
logloss / mlogloss, which may also be named; anything else, or a name that does not fit the number of classes, raises
ValueError. `evals_result_["validation_0"]["auc"]` holds the history and early stopping MAXIMISES it. The rule has one
copy, csrc/gbdt_auc.h: unweighted, margins compared numerically as doubles (-0.0 ties +0.0), and per class the int64
U2 = sum over positives i of (2 #{negatives below m_i} + #{negatives equal to m_i}) <= 2 P N. The score is formed from
the integers by `auc_score`, the one function both learners call, in exact rational arithmetic rounded once:
U2 / (2 P N) for two classes, XGBoost's one-vs-rest average weighted by prevalence, sum_k P_k auc_k / sum_k P_k with
class k's margin row scored against y == k, for K >= 3. The host function is `auc` (mifx_gbdt_auc: a sort per class
and side, one merge walk); with device="gpu" the eval margins are NOT read back: mifx/ops/gbdt_auc.py fills a
[m, 2 K] table (a class's negatives and positives as two NaN-padded columns), sorts all columns at once with the
batched radix sort of the cuts (csrc/gbdt_sort.hip) and counts the pairs in csrc/gbdt_auc.hip (one workgroup per tile
of sorted positives, its span of the sorted negatives staged through LDS, integer adds only), and K integers come
back per round. Equal integers give equal bits, so the device score equals the host twin's for any launch geometry.
An eval set in which some class has no positive or no negative row raises ValueError in `fit`, before the first
round; the host function refuses margins that are not finite (the device path does not check: a fit's margins are
finite by construction); the device path takes up to 256 classes. Not implemented: weighted AUC, aucpr, error, map,
AUC for XGBRanker; beside AUC and the ranker's ndcg / ndcg@k (above) the metrics keep their host path: rmse, mae,
quantile, logloss and mlogloss have their margins read back once per round."""
from __future__ import annotations

import ctypes
import functools
import logging
import os
import sys

import numpy as np

from .sample import group_bitsets

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
    a = lib.mifx_gbdt_grow_stats.argtypes  # the leaf-wise growers: max_leaves follows max_depth, the mask is [f]
    lib.mifx_gbdt_grow_lossguide_stats.argtypes = a[:7] + [ctypes.c_int] + a[7:]
    lib.mifx_gbdt_grow_fixed_lossguide_stats.argtypes = lib.mifx_gbdt_grow_lossguide_stats.argtypes
    for name in ("", "_fixed", "_lossguide", "_fixed_lossguide"):  # the *_stats arguments, then the directions [f]
        fn = getattr(lib, f"mifx_gbdt_grow{name}_mono")
        fn.argtypes = getattr(lib, f"mifx_gbdt_grow{name}_stats").argtypes + [_I]
        fn.restype = ctypes.c_int
    u64 = ctypes.c_uint64
    for name in ("", "_lossguide"):  # fixed, the *_mono arguments (mono nullable), then groups, n_groups, rate, seed, round
        fn = getattr(lib, f"mifx_gbdt_grow{name}_nodeset")
        fn.argtypes = [ctypes.c_int] + getattr(lib, f"mifx_gbdt_grow{name}_mono").argtypes + \
            [ctypes.POINTER(u64), ctypes.c_int, ctypes.c_double, u64, u64]
        fn.restype = ctypes.c_int
    lib.mifx_gbdt_sample_rows.argtypes = [u64, u64, ctypes.c_double, ctypes.c_long, _U8]
    lib.mifx_gbdt_sample_rows.restype = ctypes.c_long
    lib.mifx_gbdt_sample_features.argtypes = [u64, u64, u64, ctypes.c_double, _U8, ctypes.c_int, _U8]
    lib.mifx_gbdt_level_mask.argtypes = [u64, u64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, _U8,
                                         _U8]
    lib.mifx_gbdt_leaf_refresh.argtypes = [_D, _F, _I, ctypes.c_long, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                           _D, ctypes.c_int]
    lib.mifx_gbdt_rank_grad.argtypes = [ctypes.c_int, _D, _D, ctypes.POINTER(ctypes.c_long), ctypes.c_long, _D, _D,
                                        ctypes.c_int, _F, _F, ctypes.c_int]
    lib.mifx_gbdt_auc.argtypes = [_D, _D, ctypes.c_long, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    for f in (lib.mifx_gbdt_cuts, lib.mifx_gbdt_bin, lib.mifx_gbdt_grow, lib.mifx_gbdt_predict,
              lib.mifx_gbdt_grow_fixed, lib.mifx_gbdt_quant_exp, lib.mifx_gbdt_grow_ex, lib.mifx_gbdt_grow_fixed_ex,
              lib.mifx_gbdt_sample_features, lib.mifx_gbdt_level_mask, lib.mifx_gbdt_grow_stats,
              lib.mifx_gbdt_grow_fixed_stats, lib.mifx_gbdt_grow_lossguide_stats,
              lib.mifx_gbdt_grow_fixed_lossguide_stats, lib.mifx_gbdt_leaf_refresh, lib.mifx_gbdt_rank_grad,
              lib.mifx_gbdt_auc):
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


def leaf_refresh(resid: np.ndarray, h: np.ndarray, leaf_of_row: np.ndarray, value: np.ndarray, alpha: float,
                 eta: float, threads: int = 1) -> None:
    """mifx_gbdt_leaf_refresh (csrc/gbdt.cpp), in place on `value` (float64, contiguous): value[l] becomes eta times the
    weighted lower alpha-quantile of resid (float64) over the rows with leaf_of_row == l (int32; -1 takes no part),
    the rows weighing their float32 hessians h as the integers of csrc/gbdt_quantile.h."""
    n = len(resid)
    assert resid.dtype == value.dtype == np.float64 and h.dtype == np.float32 and leaf_of_row.dtype == np.int32
    assert len(h) == len(leaf_of_row) == n and all(a.flags.c_contiguous for a in (resid, h, leaf_of_row, value))
    if _lib().mifx_gbdt_leaf_refresh(_p(resid, _D), _p(h, _F), _p(leaf_of_row, _I), n, len(value), float(alpha),
                                     float(eta), _p(value, _D), int(threads)) != 0:
        raise ValueError("leaf_of_row holds a leaf outside the tree")


_RANK_OBJECTIVES = {"rank:pairwise": 0, "rank:ndcg": 1}


def discount_tables(max_size: int):
    """(D, P) of csrc/gbdt_rank.h, float64 [max_size + 1] each: D[r] = 1 / log2(r + 2) and its exclusive prefix sums,
    summed sequentially. The one place they are computed: the host function and the device kernels read these bits."""
    D = 1.0 / np.log2(np.arange(max_size + 1, dtype=np.float64) + 2.0)
    P = np.zeros(max_size + 1, np.float64)
    np.cumsum(D[:-1], out=P[1:])
    return D, P


def rank_grad(objective: str, margin: np.ndarray, y: np.ndarray, gptr: np.ndarray, topk: int = 0, threads: int = 1):
    """mifx_gbdt_rank_grad (csrc/gbdt.cpp): the float32 LambdaMART pair (g, h) of "rank:pairwise" or "rank:ndcg" from
    float64 margins and labels (integers in [0, 31]) over the contiguous query groups with row offsets gptr [G + 1];
    topk = k >= 1 keeps the pairs with a row ranked above k, 0 all of them. The rule is csrc/gbdt_rank.h."""
    margin, y = np.ascontiguousarray(margin, np.float64), np.ascontiguousarray(y, np.float64)
    gptr = np.ascontiguousarray(gptr, np.int64)
    if len(gptr) < 1 or gptr[-1] != len(y) or len(margin) != len(y):
        raise ValueError("gptr must cover every row: one margin and one label per row")
    D, P = discount_tables(int(np.diff(gptr).max()) if len(gptr) > 1 else 0)
    g, h = np.empty(len(y), np.float32), np.empty(len(y), np.float32)
    if _lib().mifx_gbdt_rank_grad(_RANK_OBJECTIVES[objective], _p(margin, _D), _p(y, _D),
                                  _p(gptr, ctypes.POINTER(ctypes.c_long)), len(gptr) - 1, _p(D, _D), _p(P, _D),
                                  int(topk), _p(g, _F), _p(h, _F), int(threads)) != 0:
        raise ValueError("gptr must ascend from 0, labels must be integers in [0, 31] and topk >= 0")
    return g, h


def _rank_order(margin: np.ndarray, gid: np.ndarray) -> np.ndarray:
    """Row ids group by group, each group in the rank order of csrc/gbdt_rank.h: margin descending on the integer
    key of csrc/gbdt_sort_key.h (+0.0 above -0.0), ties to the lower row."""
    b = np.ascontiguousarray(margin, np.float64).view(np.uint64)
    key = np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    return np.lexsort((~key, gid))  # (stable: equal keys keep their row order)


def _ndcg_terms(y: np.ndarray, gptr: np.ndarray, k: int):
    """(gid, gain, disc) of ndcg, one entry per row: the row's group, its gain 2^label - 1 and the discount of its
    POSITION inside the group, 0.0 at and below the cutoff k >= 1."""
    sizes = np.diff(gptr)
    gid = np.repeat(np.arange(len(gptr) - 1), sizes)
    pos = np.arange(len(y)) - np.repeat(gptr[:-1], sizes)
    disc = 1.0 / np.log2(pos + 2.0)
    if k > 0:
        disc = np.where(pos < k, disc, 0.0)
    return gid, np.exp2(y) - 1.0, disc


def ndcg_idcg(y: np.ndarray, gptr: np.ndarray, k: int = 0, _terms=None) -> np.ndarray:
    """IDCG float64 [G] of ndcg: per group the gains sorted descending times the discounts, summed in that order and
    truncated at k. Labels and groups only, so the device metric (mifx.ops.gbdt_ndcg) computes it once per fit."""
    gid, gain, disc = _terms or _ndcg_terms(y, gptr, k)
    return np.bincount(gid, gain[np.lexsort((-y, gid))] * disc, minlength=len(gptr) - 1)


def ndcg_mean(scores: np.ndarray) -> float:
    """The metric from the groups' scores: the one expression the host function and the device path share."""
    return float(np.mean(scores)) if len(scores) else 1.0


def ndcg(margin: np.ndarray, y: np.ndarray, gptr: np.ndarray, k: int = 0) -> float:
    """Mean NDCG over the groups (XGBoost's "ndcg", "ndcg@k" for k >= 1): gains 2^label - 1, discounts
    1 / log2(rank + 2), @k truncating both DCG and IDCG; a group without a relevant row scores 1.0."""
    G = len(gptr) - 1
    gid, gain, disc = terms = _ndcg_terms(y, gptr, k)
    dcg = np.bincount(gid, gain[_rank_order(margin, gid)] * disc, minlength=G)
    idcg = ndcg_idcg(y, gptr, k, terms)
    return ndcg_mean(np.where(idcg > 0, dcg / np.where(idcg > 0, idcg, 1.0), 1.0))


def _threads() -> int:
    return max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1))))


def auc_counts(margin: np.ndarray, y: np.ndarray, threads: int | None = None):
    """mifx_gbdt_auc (csrc/gbdt.cpp; the rule is csrc/gbdt_auc.h): (U2, P, N), int64 [K] each, of margins [n] (K = 1:
    y is 0 / 1, 1 the positive) or class-major [K, n] (y the class index, row k scored against y == k). U2_k counts 2
    for every (negative, positive) pair of class k with the positive's margin above and 1 for every tied pair, margins
    compared as doubles. Refuses margins that are not finite."""
    margin = np.ascontiguousarray(margin, np.float64)
    margin = margin[None] if margin.ndim == 1 else margin
    y = np.ascontiguousarray(np.asarray(y).reshape(-1), np.float64)
    K, m = margin.shape[0], margin.shape[-1]
    if margin.ndim != 2 or len(y) != m or m >= 2 ** 31:
        raise ValueError("auc: margins must be [n] or [K, n] with one label per row (n < 2^31)")
    if ((y != np.floor(y)) | (y < 0) | (y >= max(K, 2))).any():
        raise ValueError(f"auc: labels must be class indices in [0, {max(K, 2)})")
    out = np.zeros((K, 3), np.int64)
    rc = _lib().mifx_gbdt_auc(_p(margin, _D), _p(y, _D), m, K, _p(out, ctypes.POINTER(ctypes.c_longlong)),
                              int(threads or _threads()))
    if rc != 0:
        raise ValueError("auc: the margins must be finite" if rc == -2 else "auc: bad arguments")
    return out[:, 0].copy(), out[:, 1].copy(), out[:, 2].copy()


def auc_score(U2, P, N) -> float:
    """The AUC from the integers of `auc_counts` or of the device kernels (mifx.ops.gbdt_auc), the one place it is
    formed: U2 / (2 P N) for one class, XGBoost's one-vs-rest average weighted by prevalence, sum_k P_k auc_k / sum_k
    P_k, for several -- exact rational arithmetic, rounded once. A class without a positive or a negative row raises."""
    from fractions import Fraction

    U2, P, N = ([int(v) for v in np.ravel(a)] for a in (U2, P, N))
    if not P or any(p <= 0 for p in P) or any(n <= 0 for n in N):
        raise ValueError("auc is undefined on an eval set in which a class has no positive or no negative row")
    return float(sum(Fraction(u, 2 * n) for u, n in zip(U2, N)) / sum(P))


def auc(margin: np.ndarray, y: np.ndarray, threads: int | None = None, return_counts: bool = False):
    """Unweighted AUC of margins [n] against 0 / 1 labels, or of class-major margins [K, n] against class indices
    (one-vs-rest, weighted by prevalence): `auc_score` of `auc_counts`. With return_counts, (score, (U2, P, N))."""
    counts = auc_counts(margin, y, threads)
    score = auc_score(*counts)
    return (score, counts) if return_counts else score


class _Base:
    _objective = "reg:squarederror"

    def __init__(self, n_estimators: int = 100, learning_rate: float = 0.3, max_depth: int = 6,
                 min_child_weight: float = 1.0, reg_lambda: float = 1.0, gamma: float = 0.0, max_bins: int = 256,
                 base_score: float | None = None, n_jobs: int | None = None, random_state: int = 0,
                 verbosity: int = 0, device: str | None = None, fixed_point: bool | None = None,
                 subsample: float = 1.0, colsample_bytree: float = 1.0, colsample_bylevel: float = 1.0,
                 importance_type: str = "gain", grow_policy: str = "depthwise", max_leaves: int = 0,
                 monotone_constraints=None, interaction_constraints=None, colsample_bynode: float = 1.0):
        self.n_estimators, self.learning_rate, self.max_depth = n_estimators, learning_rate, max_depth
        self.min_child_weight, self.reg_lambda, self.gamma, self.max_bins = min_child_weight, reg_lambda, gamma, max_bins
        self.base_score, self.n_jobs = base_score, n_jobs
        self.random_state, self.verbosity = random_state, verbosity  # random_state: the seed of every draw
        self.subsample, self.colsample_bytree, self.colsample_bylevel = subsample, colsample_bytree, colsample_bylevel
        self.grow_policy, self.max_leaves = grow_policy, max_leaves
        self.monotone_constraints = monotone_constraints
        self.interaction_constraints, self.colsample_bynode = interaction_constraints, colsample_bynode
        self._check_rates()
        self._check_policy()
        self._monotone(None)
        self._nodeset(None)
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

    def _policy(self):
        """(grow_policy, max_leaves); depth-wise for a model pickled before they existed."""
        return str(getattr(self, "grow_policy", "depthwise")), int(getattr(self, "max_leaves", 0))

    def _lossguide(self) -> bool:
        return self._policy()[0] == "lossguide"

    def _check_policy(self) -> None:
        policy, leaves = self._policy()
        if policy not in ("depthwise", "lossguide"):
            raise ValueError(f"grow_policy must be 'depthwise' or 'lossguide', got {policy!r}")
        if policy == "depthwise":
            if leaves != 0:
                raise ValueError(f"max_leaves={leaves} needs grow_policy='lossguide' (depth-wise growth has no leaf "
                                 f"budget)")
            return
        if leaves < 2:
            raise ValueError(f"grow_policy='lossguide' needs max_leaves >= 2, got {leaves}")
        if int(self.max_depth) < 0:
            raise ValueError(f"max_depth must be >= 0 (0: no depth limit), got {self.max_depth}")
        if self._rates()[2] < 1.0:
            raise ValueError("colsample_bylevel < 1 is not defined for grow_policy='lossguide' (use colsample_bytree)")

    def _monotone(self, f: int | None):
        """monotone_constraints as int32 [f] directions, or None when nothing is constrained (None, empty, all zeros;
        a model pickled before the argument existed): the growers then take their unconstrained paths. A sequence of f
        integers in {-1, 0, +1} or a dict {feature index: direction}; f = None checks the values only."""
        mc = getattr(self, "monotone_constraints", None)
        if mc is None:
            return None
        if isinstance(mc, dict):
            keys = list(mc)
            if any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0 for k in keys):
                raise ValueError(f"monotone_constraints: the keys of a dict are feature indices, got {keys!r}")
            if f is not None and any(k >= f for k in keys):
                raise ValueError(f"monotone_constraints names feature {max(keys)} but the table has {f} features")
            vals, size = list(mc.values()), (max(keys, default=-1) + 1 if f is None else f)
        else:
            if isinstance(mc, (str, bytes)) or np.ndim(mc) != 1:
                raise ValueError("monotone_constraints must be a sequence of integers or a dict {feature: direction}")
            vals, keys, size = list(mc), None, len(mc)
            if f is not None and size != f:
                raise ValueError(f"monotone_constraints holds {size} directions but the table has {f} features")
        for v in vals:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v not in (-1, 0, 1):
                raise ValueError(f"monotone_constraints: every direction must be the integer -1, 0 or +1, got {v!r}")
        out = np.zeros(size, np.int32)
        out[keys if keys is not None else slice(None)] = vals
        if not out.any():
            return None
        if self._refresh_alpha() is not None:
            raise ValueError("monotone_constraints with reg:absoluteerror / reg:quantileerror is not implemented: the "
                             "refreshed leaf values would have to be clamped to the leaves' intervals")
        return out

    def _nodeset(self, f: int | None):
        """(groups, colsample_bynode) for the growers' node-set entries (csrc/gbdt_nodeset.h), or None when both options
        are off (None or no groups, a rate of 1.0; a model pickled before the arguments existed): the growers then take
        the paths they always took. groups: None or a list of lists of feature indices. f = None checks the values
        only; with f an index >= f raises."""
        ic, rate = getattr(self, "interaction_constraints", None), float(getattr(self, "colsample_bynode", 1.0))
        if not 0.0 < rate <= 1.0:  # (a NaN fails too)
            raise ValueError(f"colsample_bynode must be in (0, 1], got {rate}")
        groups = None
        if ic is not None:
            if isinstance(ic, (str, bytes)) or not hasattr(ic, "__iter__"):
                raise ValueError("interaction_constraints must be a sequence of sequences of feature indices")
            groups = []
            for grp in ic:
                if isinstance(grp, (str, bytes)) or not hasattr(grp, "__iter__"):
                    raise ValueError(f"interaction_constraints: every group is a sequence of feature indices, got {grp!r}")
                grp = list(grp)
                for j in grp:
                    if isinstance(j, bool) or not isinstance(j, (int, np.integer)) or j < 0:
                        raise ValueError(f"interaction_constraints: a feature index is a non-negative integer, got {j!r}")
                    if f is not None and j >= f:
                        raise ValueError(f"interaction_constraints names feature {j} but the table has {f} features")
                groups.append([int(j) for j in grp])
        return (groups or None, rate) if groups or rate < 1.0 else None

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
        if self._lossguide():  # the tree's own feature set [f]: the one level of a depth-1 mask
            return rows, level_mask(self._seed(), it, f, 1, bytree, 1.0)[0] if bytree < 1.0 else None
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

    def _refresh_alpha(self):
        """The quantile every finished tree's leaves are refreshed to (absolute / quantile error); None: no refresh."""
        return None

    def _metric_name(self) -> str:
        return "rmse"

    def _metric(self, margin: np.ndarray, y: np.ndarray) -> float:
        return float(np.sqrt(np.mean((margin - y) ** 2)))

    def _better(self, score: float, best: float) -> bool:
        """Whether an eval score improves on the best so far: every metric but NDCG and AUC is minimised."""
        return score < best

    def _check_y(self, y: np.ndarray) -> np.ndarray:
        return y.astype(np.float64)

    def _check_eval(self, ey: np.ndarray) -> None:
        """Refuses, before the first round, an eval set the metric is not defined on (the classifier's AUC)."""

    def _device_metric(self, ey: np.ndarray, dev):
        """A callable scoring the eval margins on the device ([K, m] tensor -> float), built once per fit, or None:
        the margins are then read back and scored by _metric on the host."""
        return None

    def _device_grad(self, G, margin, yd, g, h, wd, alpha) -> None:
        """The single-margin gradient launch of the device loop (the ranker has its own kernel)."""
        G.grad_hess(self._objective, margin, yd, g, h, wd, alpha=0.5 if alpha is None else alpha)

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

    def _grow_stats(self, bins, nbins, g, h, leaf_of_row, rows=None, level_mask=None, round: int = 0):
        """(_grow's tree, (gain, cover)): the tree and its nodes' statistics (float64 [nodes] each). Under
        grow_policy="lossguide" the tree is grown leaf-wise and level_mask is the tree's [f] feature mask. `round`: the
        tree's index, the key of its colsample_bynode draws."""
        n = bins.shape[1]
        lossguide, leaves = self._lossguide(), self._policy()[1]
        cap = 2 * leaves - 1 if lossguide else 2 ** (self.max_depth + 1)
        fe, sb, left, right = (np.empty(cap, np.int32) for _ in range(4))
        dl = np.empty(cap, np.uint8)
        val = np.empty(cap, np.float64)
        gain, cover = np.empty(cap, np.float64), np.empty(cap, np.float64)
        grow = _lib().mifx_gbdt_grow_fixed_stats if self._fixed() else _lib().mifx_gbdt_grow_stats
        mono = getattr(self, "_mono", None)  # fit's validated directions: the constrained entries take them last
        ns = getattr(self, "_ns", None)  # fit's validated node-set spec: one entry per policy, after a nullable mono
        if mono is not None:
            grow = _lib().mifx_gbdt_grow_fixed_mono if self._fixed() else _lib().mifx_gbdt_grow_mono
        if ns is not None:
            nsfn, fixed = _lib().mifx_gbdt_grow_nodeset, int(self._fixed())
            grow = lambda *a: nsfn(fixed, *a)  # noqa: E731
        if lossguide:
            fn = _lib().mifx_gbdt_grow_fixed_lossguide_stats if self._fixed() else _lib().mifx_gbdt_grow_lossguide_stats
            if mono is not None:
                fn = _lib().mifx_gbdt_grow_fixed_lossguide_mono if self._fixed() else _lib().mifx_gbdt_grow_lossguide_mono
            grow = lambda *a: fn(*a[:7], leaves, *a[7:])  # noqa: E731
            if ns is not None:
                nsfn = _lib().mifx_gbdt_grow_lossguide_nodeset
                grow = lambda *a: nsfn(fixed, *a[:7], leaves, *a[7:])  # noqa: E731
        tail = () if mono is None else (_p(mono, _I),)
        if ns is not None:  # groups as bitsets, the rate, and the draw's key: the seed and the tree index
            table, rate = ns
            tail = (None if mono is None else _p(mono, _I),
                    None if table is None else _p(table, ctypes.POINTER(ctypes.c_uint64)),
                    0 if table is None else len(table), rate, self._seed(), int(round) & _M64)
        if rows is not None:
            rows = np.ascontiguousarray(rows, np.int32)
        if level_mask is not None:
            level_mask = np.ascontiguousarray(level_mask, np.uint8)
        cnt = grow(_p(bins, _U16), n, bins.shape[0], _p(nbins, _I), _p(g, _F), _p(h, _F),
                   int(self.max_depth), float(self.min_child_weight), float(self.reg_lambda),
                   float(self.gamma), float(self.learning_rate), self._nthreads(), cap, _p(fe, _I),
                   _p(sb, _I), _p(dl, _U8), _p(left, _I), _p(right, _I), _p(val, _D),
                   _p(leaf_of_row, _I), None if rows is None else _p(rows, _I), 0 if rows is None else len(rows),
                   None if level_mask is None else _p(level_mask, _U8), _p(gain, _D), _p(cover, _D),
                   *tail)
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
        self._check_policy()
        self._check_data_device(X, y, sample_weight, *(eval_set[-1] if eval_set else ()))
        y = self._check_y(_host(y).reshape(-1))
        X = X if _is_tensor(X) else np.asarray(X)
        if X.ndim != 2 or len(X) != len(y):
            raise ValueError("X must be [n, features] with one label per row")
        w = self._row_weights(self._weights(sample_weight, y), y)
        self._nfeat = X.shape[1]
        self._mono = self._monotone(self._nfeat)
        ns = self._nodeset(self._nfeat)  # the host learners take the groups as the bitset table of csrc/gbdt_nodeset.h
        self._ns = None if ns is None else (None if ns[0] is None else group_bitsets(ns[0], self._nfeat), ns[1])
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
            self._check_eval(ey)
            ev_margin = np.full((K, len(ey)), self._base_margin)
            ev = (ex, ey, ev_margin)
        self._trees, self._node_stats = [], []
        best, best_it, since, hist = None, 0, 0, []
        alpha = self._refresh_alpha()
        for it in range(int(self.n_estimators)):
            g, h = self._weighted_grad_hess(margin if K > 1 else margin[0], y, w)
            g, h = g.reshape(K, -1), h.reshape(K, -1)
            for k in range(K):
                rows, mask = self._round_draws(it * K + k, len(y), self._nfeat)
                tree, stats = self._grow_stats(bins, nbins, g[k], h[k], leaf_of_row, rows, mask, it * K + k)
                if alpha is not None:  # the leaves' exact quantiles of the residuals, before any margin moves
                    leaf_refresh(y - margin[k], np.ascontiguousarray(h[k]), leaf_of_row, tree[5], alpha,
                                 float(self.learning_rate), self._nthreads())
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
                if best is None or self._better(score, best):
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
        the grower (and of the eval update), each on one class's row. Absolute / quantile error: the grower leaves
        the margins alone, the leaf refresh (csrc/gbdt_quantile.hip) rewrites the tree's leaf values from them, and
        the refreshed tree is then applied to every training row as it is to the eval set."""
        import torch

        from ..ops import gbdt_gpu as G
        from ..ops import gbdt_prep as P

        lossguide, leaves = self._lossguide(), self._policy()[1]
        if lossguide:
            G.check_limits_lossguide(len(y), int(self.max_bins), int(self.max_depth), leaves)
        else:
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
        masks, mask_kw = None, "feature_mask" if lossguide else "level_mask"
        if lossguide and bytree < 1.0 and rounds > 0:  # one [f] set per tree
            masks = np.stack([level_mask(self._seed(), t, self._nfeat, 1, bytree, 1.0)[0] for t in range(rounds * K)])
        elif not lossguide and (bytree < 1.0 or bylevel < 1.0) and int(self.max_depth) > 0 and rounds > 0:
            masks = np.stack([level_mask(self._seed(), t, self._nfeat, int(self.max_depth), bytree, bylevel)
                              for t in range(rounds * K)])
        with torch.cuda.device(dev):
            ns = self._nodeset(self._nfeat)  # the groups go up once, as a bitset table
            bst = G.LossguideBooster.from_device_bins(bins, nbins, int(self.max_depth), leaves, self._mono, ns) \
                if lossguide else G.Booster.from_device_bins(bins, nbins, int(self.max_depth), self._mono, ns)
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
                self._check_eval(ey)
                ev = (P.device_bins(P.as_device_matrix(ex, dev), tables), ey,
                      torch.full((K, len(ey)), self._base_margin, dtype=torch.float64, device=dev))
            best, best_it, since, hist, done = None, 0, 0, [], 0
            alpha = self._refresh_alpha()
            refresh = None if alpha is None else G.LeafRefresh(len(y), bst.cap, dev)
            dev_metric = None if ev is None else self._device_metric(ev[1], dev)
            for it in range(rounds):
                if K > 1:  # every class's pair from the margins at the start of the round, one launch
                    G.grad_hess_softmax(margin, yd, g, h, wd)
                else:
                    self._device_grad(G, margin[0], yd, g[0], h[0], wd, alpha)
                for k in range(K):
                    tree = tuple(t[it * K + k] for t in trees)
                    bst.grow(g[k], h[k], tree, self.min_child_weight, self.reg_lambda, self.gamma, self.learning_rate,
                             margin[k] if refresh is None else None, subsample=sub, seed=self._seed(),
                             round=it * K + k, stats=tuple(s[it * K + k] for s in stats),
                             **{mask_kw: None if masks is None else masks[it * K + k]})
                    if refresh is not None:  # the margins are still the ones the residuals are taken from
                        refresh(bst.leaf_of_row, tree[5], margin[k], yd, h[k], alpha, float(self.learning_rate))
                        bst.apply(bst.bins, tree, margin[k])
                    if ev is not None:
                        bst.apply(ev[0], tree, ev[2][k])
                done = (it + 1) * K
                if ev is not None:
                    if dev_metric is not None:  # scored where the margins are: only the metric's integers come back
                        score = dev_metric(ev[2])
                    else:
                        em = ev[2].cpu().numpy()  # the round's one read-back
                        score = self._metric(em if K > 1 else em[0], ev[1])
                    hist.append(score)
                    if verbose:
                        logging.info("[%d]\tvalidation_0-%s:%.5f", it, self._metric_name(), score)
                    if best is None or self._better(score, best):
                        best, best_it, since = score, it, 0
                    else:
                        since += 1
                        if early_stopping_rounds and since >= early_stopping_rounds:
                            break
            fe, sb, dl, le, ri, val, cnt = (t[:done].cpu().numpy() for t in trees)
            gain, cover = (s[:done].cpu().numpy() for s in stats)
        self._trees, self._node_stats = [], []
        for t in range(done):
            c = int(np.ravel(cnt[t])[0])  # (the leaf-wise grower's count comes with the tree's depth)
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

    def _device_paths(self, dev, tables):
        """The path tables on `dev`, uploaded once per model and device (fit and a new tree limit reset them)."""
        from ..ops import gbdt_prep as P

        cache = getattr(self, "_dev_paths", None)
        if cache is None:
            cache = self._dev_paths = {}
        if dev.index not in cache:
            cache[dev.index] = [P.DevicePaths(t, dev) for t in tables]
        return cache[dev.index]

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
            Xd = P.as_device_matrix(X, X.device)
            out = torch.empty((len(Xd), K, f + 1), dtype=torch.float64, device=X.device)
            for k in range(K if len(Xd) else 0):  # one launch per class over the class's own table
                P.contribs(self._device_paths(X.device, tables)[k], Xd, self._base_margin, out[:, k, :], counts[k],
                           _recs_per_chunk, _route)
            return out[:, 0, :] if K == 1 else out
        X = np.ascontiguousarray(_host(X), dtype=np.float64)
        out = np.empty((len(X), K, f + 1), np.float64)
        for k in range(K):
            shap.contribs(tables[k], X, counts[k], self._base_margin, out[:, k, :], self._nthreads())
        return out[:, 0, :] if K == 1 else out

    def predict_interactions(self, X, _recs_per_chunk: int | None = None, _route: str | None = None,
                             _threads: int | None = None):
        """Per-row SHAP interaction values in margin space (XGBoost's pred_interactions, path-dependent):
        [n, f + 1, f + 1], or [n, K, f + 1, f + 1] for a K-class model, float64. Cell (i, j), i != j < f, is the
        Shapley interaction index of features i and j in the game of predict_contribs; both (i, j) and (j, i) are
        computed, each from its own conditioned pass, and agree to rounding. The diagonal (i, i) is feature i's
        contribution minus the rest of row i, so row i sums to predict_contribs' column i and the matrix to the
        margin; cell (f, f) is the bias and the rest of row and column f is zero.

        Inputs, trees, devices and errors are predict_contribs': numpy or CPU input gives a numpy array from the
        host function (threads: n_jobs, the same bits for any count), a tensor on a GPU a tensor there from the
        device kernel with the same bits. The result takes 8 (f + 1)^2 bytes per row and class and is made in one
        piece. The private arguments are the kernels' launch geometry."""
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
            Xd = P.as_device_matrix(X, X.device)
            out = torch.empty((len(Xd), K, f + 1, f + 1), dtype=torch.float64, device=X.device)
            for k in range(K if len(Xd) else 0):  # one launch per class over the class's own table
                P.interactions(self._device_paths(X.device, tables)[k], Xd, self._base_margin, out[:, k], counts[k],
                               _recs_per_chunk, _route, _threads)
            return out[:, 0] if K == 1 else out
        X = np.ascontiguousarray(_host(X), dtype=np.float64)
        out = np.empty((len(X), K, f + 1, f + 1), np.float64)
        for k in range(K):
            shap.interactions(tables[k], X, counts[k], self._base_margin, out[:, k], self._nthreads())
        return out[:, 0] if K == 1 else out


class XGBRegressor(_Base):
    """Regression: squared error (objective "reg:squarederror", the default), absolute error ("reg:absoluteerror")
    or the pinball loss of one quantile ("reg:quantileerror" at `quantile_alpha`); the latter two refresh every
    finished tree's leaves to exact weighted quantiles of the residuals (the module docstring has the rule)."""
    _OBJECTIVES = ("reg:squarederror", "reg:absoluteerror", "reg:quantileerror")

    def __init__(self, *args, objective: str = "reg:squarederror", quantile_alpha: float = 0.5, **kwargs):
        """The parameters of _Base, the objective and, for reg:quantileerror, the quantile in (0, 1)."""
        super().__init__(*args, **kwargs)
        self.objective, self.quantile_alpha = objective, quantile_alpha
        self._refresh_alpha()

    @property
    def _objective(self) -> str:
        """squared error for a model pickled before the argument existed"""
        return getattr(self, "objective", "reg:squarederror")

    def _refresh_alpha(self):
        obj, alpha = self._objective, getattr(self, "quantile_alpha", 0.5)
        if obj not in self._OBJECTIVES:
            raise ValueError(f"objective must be one of {self._OBJECTIVES}, got {obj!r}")
        if np.ndim(alpha) != 0:
            raise ValueError("quantile_alpha must be one scalar: multi-quantile models are not implemented")
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise ValueError(f"quantile_alpha must be in (0, 1), got {alpha}")
        if obj == "reg:absoluteerror" and alpha != 0.5:
            raise ValueError(f"reg:absoluteerror is the quantile 0.5: quantile_alpha={alpha} needs reg:quantileerror")
        return None if obj == "reg:squarederror" else alpha

    def fit(self, X, y, eval_set=None, early_stopping_rounds: int | None = None, verbose: bool = False, *,
            sample_weight=None):
        self._refresh_alpha()
        return super().fit(X, y, eval_set, early_stopping_rounds, verbose, sample_weight=sample_weight)

    def _base(self, y: np.ndarray, w: np.ndarray | None = None) -> float:
        """The training mean, or the lower weighted alpha-quantile of y: the smallest label at which the weights of
        the labels up to it, accumulated in double over the sorted labels, reach alpha times their total."""
        alpha = self._refresh_alpha()
        if alpha is None:
            return super()._base(y, w)
        order = np.argsort(y, kind="stable")
        cum = np.cumsum(np.ones(len(y)) if w is None else w[order].astype(np.float64))
        return float(y[order[min(int(np.searchsorted(cum, alpha * cum[-1], side="left")), len(y) - 1)]])

    def _intercept(self, y: np.ndarray, w: np.ndarray | None) -> float:
        return self._base(y, w) if self.base_score is None else float(self.base_score)

    def _grad_hess(self, margin: np.ndarray, y: np.ndarray):
        alpha = self._refresh_alpha()
        if alpha is None:
            return super()._grad_hess(margin, y)
        d = margin - y
        if self._objective == "reg:absoluteerror":
            g = (d > 0).astype(np.float32) - (d < 0).astype(np.float32)
        else:
            g = np.where(d >= 0, np.float32(1.0 - alpha), np.float32(-alpha)).astype(np.float32)
        return g, np.ones(len(y), np.float32)

    def _metric_name(self) -> str:
        return {"reg:squarederror": "rmse", "reg:absoluteerror": "mae", "reg:quantileerror": "quantile"}[self._objective]

    def _metric(self, margin: np.ndarray, y: np.ndarray) -> float:
        alpha = self._refresh_alpha()
        if alpha is None:
            return super()._metric(margin, y)
        if self._objective == "reg:absoluteerror":
            return float(np.mean(np.abs(margin - y)))
        r = y - margin
        return float(np.mean(np.maximum(alpha * r, (alpha - 1.0) * r)))

    def predict(self, X):
        """Margins: a numpy array for host input, a tensor on the input's device for a tensor on a GPU."""
        return self._margin(X)


class XGBClassifier(_Base):
    """Classification: two classes train binary:logistic, K >= 3 classes multi:softprob (K trees per boosting round,
    tree t for class t % K). Labels are any sortable values (classes_ sorted)."""
    _objective = "binary:logistic"

    _EVAL_METRICS = (None, "logloss", "mlogloss", "auc")

    def __init__(self, *args, scale_pos_weight: float = 1.0, eval_metric: str | None = None, **kwargs):
        """The parameters of _Base, scale_pos_weight (> 0): a factor on the weights of class-1 rows, and eval_metric:
        None (the default: logloss for two classes, mlogloss for more), that default by name, or "auc"."""
        super().__init__(*args, **kwargs)
        self.scale_pos_weight, self.eval_metric = scale_pos_weight, eval_metric
        self._check_spw()
        self._auc()

    def _auc(self) -> bool:
        """Whether the eval metric is AUC, after the argument is checked (None for a model pickled before it existed)."""
        name = getattr(self, "eval_metric", None)
        if name not in self._EVAL_METRICS:
            raise ValueError(f"eval_metric must be one of {self._EVAL_METRICS}, got {name!r}")
        return name == "auc"

    def _check_eval(self, ey: np.ndarray) -> None:
        if self._auc():  # (raises for a class without a positive or a negative row)
            P = np.bincount(ey.astype(np.int64), minlength=max(2, self._num_class()))[-self._num_class():]
            auc_score(np.zeros_like(P), P, len(ey) - P)

    def _device_metric(self, ey: np.ndarray, dev):
        if not self._auc():
            return None
        from ..ops import gbdt_auc as A

        return A.AucPlan(ey, self._num_class(), dev).score

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
        name, default = getattr(self, "eval_metric", None), "mlogloss" if self._num_class() > 1 else "logloss"
        if not self._auc() and name not in (None, default):
            raise ValueError(f"eval_metric={name!r} does not fit {len(self.classes_)} classes: their metric is "
                             f"{default!r} (or 'auc')")
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
        if self._auc():
            return "auc"
        return "mlogloss" if self._num_class() > 1 else "logloss"

    def _better(self, score: float, best: float) -> bool:
        return score > best if self._auc() else score < best

    def _metric(self, margin: np.ndarray, y: np.ndarray) -> float:
        if self._auc():
            return auc(margin, y, self._nthreads())
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


class XGBRanker(_Base):
    """Learning to rank: LambdaMART on "rank:ndcg" (the default) or "rank:pairwise" over query groups given by `qid`
    or `group`; `predict` returns margins (the module docstring has the rule)."""
    _OBJECTIVES = tuple(_RANK_OBJECTIVES)

    def __init__(self, *args, objective: str = "rank:ndcg", lambdarank_pair_method: str = "all",
                 lambdarank_num_pair_per_sample: int | None = None, eval_metric: str = "ndcg", **kwargs):
        """The parameters of _Base, the objective, the pair method ("all": every pair of a group with different
        labels, our default; "topk" with lambdarank_num_pair_per_sample = k >= 1: the pairs with a row ranked above k)
        and the eval metric ("ndcg" or "ndcg@k")."""
        super().__init__(*args, **kwargs)
        self.objective, self.eval_metric = objective, eval_metric
        self.lambdarank_pair_method = lambdarank_pair_method
        self.lambdarank_num_pair_per_sample = lambdarank_num_pair_per_sample
        self._topk()
        self._metric_k()

    @property
    def _objective(self) -> str:
        return self.objective

    def _topk(self) -> int:
        """The k of the pair rule (0: every pair), after the constructor arguments are checked."""
        if self.objective not in self._OBJECTIVES:
            raise ValueError(f"objective must be one of {self._OBJECTIVES}, got {self.objective!r}")
        method, k = self.lambdarank_pair_method, self.lambdarank_num_pair_per_sample
        if method == "all":
            if k is not None:
                raise ValueError("lambdarank_num_pair_per_sample needs lambdarank_pair_method='topk'")
            return 0
        if method != "topk":
            raise ValueError(f"lambdarank_pair_method must be 'all' or 'topk' ('mean' is not implemented), got "
                             f"{method!r}")
        if k is None or int(k) != k or int(k) < 1:
            raise ValueError(f"lambdarank_pair_method='topk' needs lambdarank_num_pair_per_sample >= 1, got {k!r}")
        return int(k)

    def _metric_k(self) -> int:
        name = str(self.eval_metric)
        if name == "ndcg":
            return 0
        if name.startswith("ndcg@") and name[5:].isdigit() and int(name[5:]) >= 1:
            return int(name[5:])
        raise ValueError(f"eval_metric must be 'ndcg' or 'ndcg@k' with k >= 1, got {name!r}")

    @staticmethod
    def _group_ptr(n: int, qid, group, what: str) -> np.ndarray:
        """int64 [G + 1] row offsets from exactly one of qid (non-decreasing, one per row) and group (sizes)."""
        if (qid is None) == (group is None):
            raise ValueError(f"{what}: exactly one of qid and group must be given")
        if group is not None:
            sizes = np.asarray(_host(group)).reshape(-1)
            if (sizes < 0).any() or (sizes != sizes.astype(np.int64)).any() or int(sizes.sum()) != n:
                raise ValueError(f"{what}: group must hold non-negative sizes that sum to the number of rows ({n})")
            return np.concatenate([[0], np.cumsum(sizes.astype(np.int64))]).astype(np.int64)
        qid = np.asarray(_host(qid)).reshape(-1)
        if len(qid) != n:
            raise ValueError(f"{what}: qid must hold one id per row ({n}), got {len(qid)}")
        if n and (qid[1:] < qid[:-1]).any():
            raise ValueError(f"{what}: qid must be non-decreasing (sort the rows by query)")
        return np.concatenate([[0], np.flatnonzero(qid[1:] != qid[:-1]) + 1, [n]]).astype(np.int64)

    def fit(self, X, y, *, qid=None, group=None, eval_set=None, eval_qid=None, eval_group=None,
            early_stopping_rounds: int | None = None, verbose: bool = False, sample_weight=None):
        """Fit the ranker. Exactly one of `qid` (one non-decreasing query id per row) and `group` (the groups' sizes,
        in row order) names the query groups; the LAST eval set takes its groups from the last entry of `eval_qid` or
        `eval_group`. Labels are integers in [0, 31]. Data may be where _Base.fit takes it. `sample_weight` (group or
        row weights) is not implemented and raises ValueError. With device="gpu" a group of more than
        mifx.ops.gbdt_rank.max_group() rows raises ValueError before anything is launched."""
        self._topk()
        self._metric_k()
        if sample_weight is not None:
            raise ValueError("XGBRanker: sample_weight (group and row weights) is not implemented")
        self._check_data_device(X, y)
        n = len(_host(y).reshape(-1))
        ctx = {"gptr": self._group_ptr(n, qid, group, "fit")}
        if eval_set:
            eq, eg = (None if v is None else v[-1] for v in (eval_qid, eval_group))
            if eq is None and eg is None:
                raise ValueError("an eval set needs its query groups: eval_qid or eval_group, one entry per eval set")
            ctx["eval_gptr"] = self._group_ptr(len(_host(eval_set[-1][1]).reshape(-1)), eq, eg, "eval set")
        if self._gpu_index() is not None:
            from ..ops import gbdt_rank as R

            R.check_groups(ctx["gptr"])
        self._fit_ctx = ctx
        try:
            return super().fit(X, y, eval_set, early_stopping_rounds, verbose)
        finally:
            del self._fit_ctx  # the groups and the device plan belong to the fit, not to the model

    def _check_y(self, y: np.ndarray) -> np.ndarray:
        y = np.asarray(y)
        if y.dtype.kind not in "biuf" or not np.isin(y, np.arange(32)).all():
            raise ValueError("XGBRanker: labels must be integers in [0, 31] (relevance grades)")
        return y.astype(np.float64)

    def _intercept(self, y: np.ndarray, w: np.ndarray | None) -> float:
        return 0.0 if self.base_score is None else float(self.base_score)

    def _grad_hess(self, margin: np.ndarray, y: np.ndarray):
        return rank_grad(self.objective, margin, y, self._fit_ctx["gptr"], self._topk(), self._nthreads())

    def _device_grad(self, G, margin, yd, g, h, wd, alpha) -> None:
        from ..ops import gbdt_rank as R

        if "plan" not in self._fit_ctx:  # once per fit: the groups do not change between rounds
            self._fit_ctx["plan"] = R.RankPlan(self._fit_ctx["gptr"], margin.device)
        R.grad_hess_rank(self.objective, margin, yd, self._fit_ctx["plan"], g, h, self._topk())

    def _metric_name(self) -> str:
        return str(self.eval_metric)

    def _metric(self, margin: np.ndarray, y: np.ndarray) -> float:
        return ndcg(margin, y, self._fit_ctx["eval_gptr"], self._metric_k())

    def _device_metric(self, ey: np.ndarray, dev):
        from ..ops import gbdt_ndcg as N

        gptr = self._fit_ctx["eval_gptr"]
        if len(gptr) > 1 and int(np.diff(gptr).max()) > N.max_group():
            return None  # counting is O(m^2): above the measured limit the read-back and the host function are faster
        return N.NdcgPlan(gptr, ey, self._metric_k(), dev).score

    def _better(self, score: float, best: float) -> bool:
        return score > best  # NDCG is maximised

    def predict(self, X):
        """Margins (the ranking scores): a numpy array for host input, a tensor on the input's device for a tensor on
        a GPU."""
        return self._margin(X)
