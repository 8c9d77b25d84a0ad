"""Time per boosting round of mifx.gbdt: the device learner (device="gpu", csrc/gbdt_gpu.hip) against the host
learner (csrc/gbdt.cpp, double histograms, 16 threads) and the host's fixed-point twin.

Synthetic data: standard-normal features (32), 256 bins, depth 6, squared error. One round = gradients + one tree +
the training margins' update, exactly what `fit` does per round; device rounds are timed with a host clock around a
window that ends in a device synchronise, after warm-up rounds. Cuts + binning (host, once per fit) and the upload
(once per fit) are reported separately. The first device tree is compared with the host twin's (they must be equal).
`--subsample` / `--colsample-bytree` time stochastic rounds (round t draws with seed 0 and round t, as `fit` does; a
sampled round also walks the tree for the margins of the rows outside the sample); 1.0, the default, draws nothing.

  python tools/bench_gbdt.py --sizes 10000 100000 1000000 --out profiles/gbdt_gpu.jsonl
  python tools/bench_gbdt.py --sizes 1000000 --subsample 0.5 --host-rounds 1 --out profiles/gbdt_sample.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_rounds(model, bins, nbins, y, rounds, X=None):
    margin = np.full(len(y), float(np.mean(y)))
    leaf = np.empty(len(y), np.int32)
    times, first = [], None
    for it in range(rounds):
        t0 = time.perf_counter()
        g, h = model._grad_hess(margin, y)
        rows, mask = model._round_draws(it, len(y), bins.shape[0])
        tree = model._grow(bins, nbins, g, h, leaf, rows, mask)
        margin += tree[5][leaf] if rows is None else model._predict_trees(X, [tree], 0.0)
        times.append(time.perf_counter() - t0)
        first = first or tree
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
    ap.add_argument("--out", default=None, help="append one JSON line per size")
    a = ap.parse_args(argv)

    import torch

    from mifx.gbdt import XGBRegressor
    from mifx.ops import gbdt_gpu as G

    dev = G.device_for(0)  # no GPU: an error, never a CPU number in a GPU column
    for n in a.sizes:
        r = np.random.default_rng(n)
        X = r.standard_normal((n, a.features))
        y = X[:, 0] * X[:, 1] + np.abs(X[:, 2]) + 0.5 * X[:, 3] + r.normal(0, 0.1, n)
        kw = dict(max_bins=a.max_bins, max_depth=a.max_depth, n_jobs=a.threads, subsample=a.subsample,
                  colsample_bytree=a.colsample_bytree, random_state=0)
        host, twin = XGBRegressor(**kw), XGBRegressor(fixed_point=True, **kw)
        t0 = time.perf_counter()
        bins = host._bin_matrix(X)
        t_bin = time.perf_counter() - t0
        twin._cuts = host._cuts
        nbins = (host._ncut + 1).astype(np.int32)
        host._nfeat = twin._nfeat = a.features
        if a.subsample >= 1.0:
            X = None  # only a sampled host round walks the raw table (the margins of the rows outside the sample)
        th, _ = host_rounds(host, bins, nbins, y, a.host_rounds, X)
        tt, first_twin = host_rounds(twin, bins, nbins, y, a.host_rounds, X)
        del X
        total = a.warmup + a.rounds
        masks = None
        if a.colsample_bytree < 1.0 and a.max_depth > 0:
            from mifx.gbdt import xgb

            masks = np.stack([xgb.level_mask(0, it, a.features, a.max_depth, a.colsample_bytree, 1.0)
                              for it in range(total)])

        with torch.cuda.device(dev):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bst = G.Booster(bins, nbins, a.max_depth, dev)
            yd = torch.from_numpy(y).to(dev)
            torch.cuda.synchronize()
            t_up = time.perf_counter() - t0
            margin = torch.full((n,), float(np.mean(y)), dtype=torch.float64, device=dev)
            g, h = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
            trees = bst.new_trees(total)
            md = None if masks is None else torch.from_numpy(masks).to(dev)

            def run(lo, hi):
                for it in range(lo, hi):
                    G.grad_hess("reg:squarederror", margin, yd, g, h)
                    bst.grow(g, h, tuple(t[it] for t in trees), 1.0, 1.0, 0.0, 0.3, margin, subsample=a.subsample,
                             seed=0, round=it, level_mask=None if md is None else md[it],
                             _margin_route=a.margin_route)
                torch.cuda.synchronize()

            run(0, a.warmup)
            t0 = time.perf_counter()
            run(a.warmup, a.warmup + a.rounds)
            t_gpu = (time.perf_counter() - t0) / a.rounds
            cnt = int(trees[6][0].item())
            same = all(np.array_equal(trees[k][0, :cnt].cpu().numpy(), w) for k, w in
                       ((0, first_twin[0]), (2, first_twin[2]), (3, first_twin[3]), (4, first_twin[4]),
                        (5, first_twin[5])))
            del bst, yd, margin, g, h, trees
            torch.cuda.empty_cache()
        rec = {"n": n, "features": a.features, "max_bins": a.max_bins, "max_depth": a.max_depth,
               "subsample": a.subsample, "colsample_bytree": a.colsample_bytree, "margin_route": a.margin_route,
               "host_threads": a.threads, "bin_s": round(t_bin, 4), "upload_s": round(t_up, 4),
               "host_round_s": [round(t, 5) for t in th], "host_fixed_round_s": [round(t, 5) for t in tt],
               "gpu_round_s": round(t_gpu, 6), "gpu_rounds": a.rounds,
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
