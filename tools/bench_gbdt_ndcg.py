"""Time of XGBRanker's eval metric step on the device (mifx/ops/gbdt_ndcg.py: `NdcgPlan.score`, up to three launches of
csrc/gbdt_ndcg.hip and the read-back of one double per group), for "ndcg" and "ndcg@k", next to the route it replaces
(read-back of the eval margins plus the numpy function mifx.gbdt.xgb.ndcg) and to a depth-6 rank:ndcg boosting round
(gradient launch + one tree) on as many training rows in the same groups.

Synthetic data as in tools/bench_gbdt_rank.py: labels 0 ... 4 uniform, margins standard normal (a fit's later rounds,
nearly all distinct). A shape is `rows:group` -- groups of `group` rows, or of sizes uniform in [group / 2, 3 group / 2]
with a trailing `~`; `N:N` is one group of N rows, the sweep that fixes mifx_gbdt_ndcg_max_group(). Every figure is a
host clock around a window of calls that ends in a device synchronise (the metric call ends in its own read-back),
after warm-up calls; a window is repeated `--repeats` times and the least, median and largest time per call are
recorded. Before a shape is timed the device score is compared with the host function's: they must be equal.

  python tools/bench_gbdt_ndcg.py --shapes 100000:40 1000000:120~ 1000000:2048 --out profiles/gbdt_ndcg.jsonl
  python tools/bench_gbdt_ndcg.py --skip-round --shapes 4096:4096 8192:8192 ... 1048576:1048576
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

from bench_gbdt_rank import group_ptr, windows  # noqa: E402  (the same shapes, the same protocol)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["100000:40"])
    ap.add_argument("--cutoffs", nargs="+", type=int, default=[0, 10], help="0 is ndcg, k is ndcg@k")
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-round", action="store_true", help="do not time the boosting round")
    ap.add_argument("--out", default=None, help="append one JSON line per shape")
    a = ap.parse_args(argv)

    import torch

    from mifx.gbdt import xgb
    from mifx.ops import gbdt_gpu as G
    from mifx.ops import gbdt_ndcg as N
    from mifx.ops import gbdt_rank as R

    dev = G.device_for(0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    for shape in a.shapes:
        rows, group = shape.split(":")
        gptr = group_ptr(int(rows), group, np.random.default_rng(int(rows)))
        n, sizes = int(gptr[-1]), np.diff(gptr)
        gen = torch.Generator(device=dev).manual_seed(n)
        yd = torch.randint(0, 5, (n,), generator=gen, device=dev).double()
        margin = torch.randn((1, n), generator=gen, device=dev, dtype=torch.float64)
        y = yd.cpu().numpy()
        rec = {"shape": shape, "rows": n, "groups": len(sizes), "largest_group": int(sizes.max()),
               "host_threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)),
               "ms_are": "least, median, largest per call"}
        if not a.skip_round and int(sizes.max()) <= R.max_group():
            bins = torch.randint(0, 256, (n, a.features), generator=gen, device=dev, dtype=torch.int16)
            bst = G.Booster.from_device_bins(bins, np.full(a.features, 256, np.int32), a.max_depth)
            tree = tuple(t[0] for t in bst.new_trees(1))
            stats = tuple(s[0] for s in bst.new_stats(1))
            rank_plan = R.RankPlan(gptr, dev)
            train_margin = torch.zeros(n, dtype=torch.float64, device=dev)
            g, h = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))

            def rank_round():
                R.grad_hess_rank("rank:ndcg", train_margin, yd, rank_plan, g, h)
                bst.grow(g, h, tree, 1.0, 1.0, 0.0, 0.3, train_margin, stats=stats)

            for _ in range(a.warmup):
                rank_round()
            rec["rank_ndcg_round_ms"] = windows(rank_round, a.calls, a.repeats, sync)
            del bst, bins, rank_plan
        rec["readback_alone_ms"] = windows(lambda: margin.cpu(), 1, 3, lambda: None)
        for k in a.cutoffs:
            name = "ndcg" if k == 0 else f"ndcg@{k}"
            plan = N.NdcgPlan(gptr, y, k, dev)
            host = lambda: xgb.ndcg(margin.cpu().numpy()[0], y, gptr, k)  # noqa: E731  (the parent's path)
            step = lambda: plan.score(margin)  # noqa: E731
            score = host()
            assert step() == score  # what is timed is equal
            for _ in range(a.warmup):
                step()
            rec[name] = {"score": score, "tiles": plan.n_tiles, "wave_groups": plan.G - plan.n_big,
                         "device_step_ms": windows(step, a.calls, a.repeats, sync),
                         "readback_plus_host_ndcg_ms": windows(host, 1, 3, lambda: None)}
            del plan
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
