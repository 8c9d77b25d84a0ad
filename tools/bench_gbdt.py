"""Time per boosting round of mifx.gbdt: the device learner (device="gpu", csrc/gbdt_gpu.hip) against the host
learner (csrc/gbdt.cpp, double histograms, 16 threads) and the host's fixed-point twin.

Synthetic data: standard-normal features (32), 256 bins, depth 6, squared error. One round = gradients + one tree +
the training margins' update, exactly what `fit` does per round; device rounds are timed with a host clock around a
window that ends in a device synchronise, after warm-up rounds. Cuts + binning (host, once per fit) and the upload
(once per fit) are reported separately. The first device tree is compared with the host twin's (they must be equal).
`--subsample` / `--colsample-bytree` time stochastic rounds (round t draws with seed 0 and round t, as `fit` does; a
sampled round also walks the tree for the margins of the rows outside the sample); 1.0, the default, draws nothing.
`--num-class K` times a classifier's round on K quantile classes of the same target: K = 2 is binary:logistic (one tree
per round), K >= 3 multi:softprob (one softmax gradient launch + K trees per round; the yardstick is K binary rounds).
The softmax gradient kernel is also timed alone, against the 16 K n bytes it must move at least (the float64 margins
in, float32 g and h out). The default, 0, is the squared-error round.
`--stats 0` grows the trees without recording the nodes' gain and cover (1, the default, is what `fit` does).

  python tools/bench_gbdt.py --sizes 10000 100000 1000000 --out profiles/gbdt_gpu.jsonl
  python tools/bench_gbdt.py --sizes 1000000 --subsample 0.5 --host-rounds 1 --out profiles/gbdt_sample.jsonl
  python tools/bench_gbdt.py --sizes 1000000 --num-class 3 --host-rounds 1 --out profiles/gbdt_multiclass.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_rounds(model, bins, nbins, y, rounds, base, X=None):
    K = model._num_class()  # trees per round: fit's own loop
    margin = np.full((K, len(y)), base)
    leaf = np.empty(len(y), np.int32)
    times, first = [], None
    for it in range(rounds):
        t0 = time.perf_counter()
        g, h = model._grad_hess(margin if K > 1 else margin[0], y)
        g, h = g.reshape(K, -1), h.reshape(K, -1)
        for k in range(K):
            rows, mask = model._round_draws(it * K + k, len(y), bins.shape[0])
            tree = model._grow(bins, nbins, g[k], h[k], leaf, rows, mask)
            margin[k] += tree[5][leaf] if rows is None else model._predict_trees(X, [tree], 0.0)
            first = first or tree
        times.append(time.perf_counter() - t0)
    return times, first


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-bins", type=int, default=256)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=20, help="timed device rounds")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--subsample", type=float, default=1.0, help="rows sampled per round, in (0, 1]")
    ap.add_argument("--colsample-bytree", type=float, default=1.0, help="features sampled per tree, in (0, 1]")
    ap.add_argument("--margin-route", type=int, default=0, choices=[0, 1],
                    help="sampled rounds: 0 = partition updates the sampled rows + a walk for the others, 1 = one walk")
    ap.add_argument("--num-class", type=int, default=0,
                    help="0: squared error (default); 2: binary:logistic; K >= 3: multi:softprob, K trees per round")
    ap.add_argument("--stats", type=int, default=1, choices=[0, 1],
                    help="1 (default): the grower records every node's gain and cover, as fit does; 0: it does not")
    ap.add_argument("--out", default=None, help="append one JSON line per size")
    a = ap.parse_args(argv)

    import torch

    from mifx.gbdt import XGBClassifier, XGBRegressor
    from mifx.ops import gbdt_gpu as G

    dev = G.device_for(0)  # no GPU: an error, never a CPU number in a GPU column
    for n in a.sizes:
        r = np.random.default_rng(n)
        X = r.standard_normal((n, a.features))
        y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + 0.5 * X[:, 3] + r.normal(0, 0.1, n)
        kw = dict(max_bins=a.max_bins, max_depth=a.max_depth, n_jobs=a.threads, subsample=a.subsample,
                  colsample_bytree=a.colsample_bytree, random_state=0)
        if a.num_class == 1 or a.num_class < 0:
            raise SystemExit("--num-class must be 0 or >= 2")
        if a.num_class:  # K quantile classes of the target, as class indices
            y = np.searchsorted(np.quantile(y, np.arange(1, a.num_class) / a.num_class), y).astype(np.float64)
            host, twin = XGBClassifier(**kw), XGBClassifier(fixed_point=True, **kw)
            host.classes_ = twin.classes_ = np.arange(a.num_class)
            base = 0.5 if a.num_class > 2 else 0.0
        else:
            host, twin = XGBRegressor(**kw), XGBRegressor(fixed_point=True, **kw)
            base = float(np.mean(y))
        K = host._num_class()
        t0 = time.perf_counter()
        bins = host._bin_matrix(X)
        t_bin = time.perf_counter() - t0
        twin._cuts = host._cuts
        nbins = (host._ncut + 1).astype(np.int32)
        host._nfeat = twin._nfeat = a.features
        if a.subsample >= 1.0:
            X = None  # only a sampled host round walks the raw table (the margins of the rows outside the sample)
        th, _ = host_rounds(host, bins, nbins, y, a.host_rounds, base, X)
        tt, first_twin = host_rounds(twin, bins, nbins, y, a.host_rounds, base, X)
        del X
        total = a.warmup + a.rounds
        masks = None
        if a.colsample_bytree < 1.0 and a.max_depth > 0:
            from mifx.gbdt import xgb

            masks = np.stack([xgb.level_mask(0, t, a.features, a.max_depth, a.colsample_bytree, 1.0)
                              for t in range(total * K)])

        with torch.cuda.device(dev):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bst = G.Booster(bins, nbins, a.max_depth, dev)
            yd = torch.from_numpy(y).to(dev)
            torch.cuda.synchronize()
            t_up = time.perf_counter() - t0
            margin = torch.full((K, n), base, dtype=torch.float64, device=dev)
            g, h = (torch.empty((K, n), dtype=torch.float32, device=dev) for _ in range(2))
            trees = bst.new_trees(total * K)
            stats = bst.new_stats(total * K) if a.stats else None
            md = None if masks is None else torch.from_numpy(masks).to(dev)
            objective = "binary:logistic" if a.num_class else "reg:squarederror"

            def grad():
                if K > 1:
                    G.grad_hess_softmax(margin, yd, g, h)
                else:
                    G.grad_hess(objective, margin[0], yd, g[0], h[0])

            def run(lo, hi):
                for it in range(lo, hi):
                    grad()
                    for k in range(K):
                        t = it * K + k
                        bst.grow(g[k], h[k], tuple(x[t] for x in trees), 1.0, 1.0, 0.0, 0.3, margin[k],
                                 subsample=a.subsample, seed=0, round=t, level_mask=None if md is None else md[t],
                                 _margin_route=a.margin_route,
                                 stats=None if stats is None else tuple(x[t] for x in stats))
                torch.cuda.synchronize()

            run(0, a.warmup)
            t0 = time.perf_counter()
            run(a.warmup, a.warmup + a.rounds)
            t_gpu = (time.perf_counter() - t0) / a.rounds
            # the gradient launch alone, on the margins the rounds left: host clock around `reps` launches that end in
            # one synchronise, sized to move ~10 GB
            reps = max(20, int(1e10 / (16.0 * K * n)))
            grad()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                grad()
            torch.cuda.synchronize()
            t_grad = (time.perf_counter() - t0) / reps
            cnt = int(trees[6][0].item())
            same = all(np.array_equal(trees[k][0, :cnt].cpu().numpy(), w) for k, w in
                       ((0, first_twin[0]), (2, first_twin[2]), (3, first_twin[3]), (4, first_twin[4]),
                        (5, first_twin[5])))
            del bst, yd, margin, g, h, trees, stats
            torch.cuda.empty_cache()
        rec = {"n": n, "features": a.features, "max_bins": a.max_bins, "max_depth": a.max_depth,
               "subsample": a.subsample, "colsample_bytree": a.colsample_bytree, "margin_route": a.margin_route,
               "host_threads": a.threads, "bin_s": round(t_bin, 4), "upload_s": round(t_up, 4),
               "host_round_s": [round(t, 5) for t in th], "host_fixed_round_s": [round(t, 5) for t in tt],
               "num_class": a.num_class, "trees_per_round": K, "node_stats": a.stats,
               "gpu_round_s": round(t_gpu, 6), "gpu_rounds": a.rounds, "gpu_grad_s": round(t_grad, 8),
               "gpu_grad_reps": reps, "grad_min_bytes": 16 * K * n, "grad_GBps": round(16e-9 * K * n / t_grad, 1),
               "host_over_gpu": round(min(th) / t_gpu, 2), "first_tree_equals_host_twin": bool(same)}
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        if not same:
            return 1
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
