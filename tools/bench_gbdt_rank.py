"""Time of XGBRanker's gradient launch on the device (csrc/gbdt_rank.hip), next to the host function at 16 threads on
the same data and to the rest of a depth-6 boosting round on the same bins (a squared-error round: gradients + grow).

Synthetic data: uniform random bins (32 features x 256 bins), labels 0 ... 4 from the bin of feature 0, margins
standard normal (a fit's later rounds; the first round's equal margins cost the same number of exp calls). A shape is
`rows:group` -- groups of `group` rows, or of sizes uniform in [group / 2, 3 group / 2] with a trailing `~`. Every figure
is a host clock around a window of calls that ends in a device synchronise, after warm-up calls; a window is repeated
`--repeats` times and the least, median and largest time per call are recorded.

  python tools/bench_gbdt_rank.py --shapes 1000000:120~ 1000000:2048 100000:40 --out profiles/gbdt_rank.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def windows(fn, calls, repeats, sync):
    """[least, median, largest] milliseconds per call of fn over `repeats` windows of `calls` calls"""
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / calls)
    out.sort()
    return [round(out[0], 4), round(out[len(out) // 2], 4), round(out[-1], 4)]


def group_ptr(rows: int, shape: str, rng) -> np.ndarray:
    size = int(shape.rstrip("~"))
    count = max(1, rows // size)
    sizes = rng.integers(size // 2, size + size // 2 + 1, count) if shape.endswith("~") else np.full(count, size)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["100000:40"])
    ap.add_argument("--objective", default="rank:ndcg")
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="append one JSON line per shape")
    a = ap.parse_args(argv)

    import torch

    from mifx.gbdt import xgb
    from mifx.ops import gbdt_gpu as G
    from mifx.ops import gbdt_rank as R

    dev = G.device_for(0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    for shape in a.shapes:
        rows, group = shape.split(":")
        rng = np.random.default_rng(int(rows))
        gptr = group_ptr(int(rows), group, rng)
        n = int(gptr[-1])
        gen = torch.Generator(device=dev).manual_seed(n)
        bins = torch.randint(0, 256, (n, a.features), generator=gen, device=dev, dtype=torch.int16)
        y = torch.div(bins[:, 0], 52, rounding_mode="floor").double()
        margin = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
        plan = R.RankPlan(gptr, dev)
        g, h = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        sizes = np.diff(gptr)
        rec = {"shape": shape, "rows": n, "groups": len(sizes), "largest_group": int(sizes.max()),
               "objective": a.objective, "launches": {"workgroup_large": plan.n_large, "workgroup_mid": plan.n_mid,
                                                      "wave_groups": plan.n_small, "threads": 256, "groups_per_wg": 4},
               "exp_per_row_mean": round(float((sizes.astype(np.float64) ** 2).sum() / n * 0.8), 1),
               "ms_are": "least, median, largest per call"}

        def grad():
            R.grad_hess_rank(a.objective, margin, y, plan, g, h)

        for _ in range(a.warmup):
            grad()
        rec["rank_grad_gpu_ms"] = windows(grad, a.calls, a.repeats, sync)

        bst = G.Booster.from_device_bins(bins, np.full(a.features, 256, np.int32), a.max_depth)
        tree = tuple(t[0] for t in bst.new_trees(1))
        stats = tuple(s[0] for s in bst.new_stats(1))
        sq_margin = torch.zeros(n, dtype=torch.float64, device=dev)

        def squared():
            G.grad_hess("reg:squarederror", sq_margin, y, g, h)
            bst.grow(g, h, tree, 1.0, 1.0, 0.0, 0.3, sq_margin, stats=stats)

        for _ in range(a.warmup):
            squared()
        rec["squared_error_round_ms"] = windows(squared, a.calls, a.repeats, sync)

        mh, yh = margin.cpu().numpy(), y.cpu().numpy()
        host = lambda: xgb.rank_grad(a.objective, mh, yh, gptr, 0, a.host_threads)  # noqa: E731
        host()
        rec["rank_grad_host_ms"] = windows(host, 1, 3, lambda: None)
        rec["host_threads"] = a.host_threads
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        del bst, bins, plan
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
