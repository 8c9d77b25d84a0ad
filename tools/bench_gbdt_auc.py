"""Time of XGBClassifier's eval_metric="auc" step on the device (mifx/ops/gbdt_auc.py: fill, batched radix sort, pair
count, read-back of K integers), next to the route it replaces (read-back of the eval margins plus the host function
mifx.gbdt.xgb.auc at 16 threads), to the default metric's evaluated-round overhead (read-back plus the numpy logloss /
mlogloss) and to a depth-6 binary:logistic boosting round on as many training rows.

Synthetic data: labels uniform over the classes; margins standard normal plus 1 on the row's own class ("normal": a
fit's later rounds, nearly all distinct) or those rounded to 64 levels ("levels": a fit's first rounds, when a few
shallow trees give few distinct margins -- long ties, the count kernel's closed-form tiles). A shape is `rows:classes`
(classes 2 is the binary case, one margin row). Every figure is a host clock around a window of calls that ends in a
device synchronise (the AUC call ends in its own read-back), after warm-up calls; a window is repeated `--repeats`
times and the least, median and largest time per call are recorded. The fill / sort / count split is the same kind of
window around each stage's launches alone.

  python tools/bench_gbdt_auc.py --shapes 100000:2 1000000:2 10000000:2 1000000:10 --out profiles/gbdt_auc.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]

from bench_gbdt_rank import windows  # noqa: E402  (the same protocol)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["100000:2"])
    ap.add_argument("--margins", nargs="+", default=["normal", "levels"], choices=["normal", "levels"])
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--skip-round", action="store_true", help="do not time the boosting round")
    ap.add_argument("--out", default=None, help="append one JSON line per shape and margin set")
    a = ap.parse_args(argv)

    import torch

    from mifx.gbdt import XGBClassifier, xgb
    from mifx.ops import gbdt_auc as A
    from mifx.ops import gbdt_gpu as G

    dev = G.device_for(0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    for shape in a.shapes:
        m, classes = (int(v) for v in shape.split(":"))
        K = 1 if classes == 2 else classes
        gen = torch.Generator(device=dev).manual_seed(m + classes)
        yd = torch.randint(0, classes, (m,), generator=gen, device=dev)
        y = yd.cpu().numpy().astype(np.float64)
        own = (yd[None, :] == (torch.arange(K, device=dev)[:, None] if K > 1 else 1)).double()
        base = torch.randn((K, m), generator=gen, device=dev, dtype=torch.float64) + own
        plan = A.AucPlan(y, K, dev)
        clf = XGBClassifier()  # the default metric's host function
        clf.classes_ = np.arange(classes)
        round_ms = None
        if not a.skip_round:
            bins = torch.randint(0, 256, (m, a.features), generator=gen, device=dev, dtype=torch.int16)
            bst = G.Booster.from_device_bins(bins, np.full(a.features, 256, np.int32), a.max_depth)
            tree = tuple(t[0] for t in bst.new_trees(1))
            stats = tuple(s[0] for s in bst.new_stats(1))
            train_margin = torch.zeros(m, dtype=torch.float64, device=dev)
            y01 = (yd == 1).double()
            g, h = (torch.empty(m, dtype=torch.float32, device=dev) for _ in range(2))

            def logistic_round():
                G.grad_hess("binary:logistic", train_margin, y01, g, h, None, alpha=0.5)
                bst.grow(g, h, tree, 1.0, 1.0, 0.0, 0.3, train_margin, stats=stats)

            for _ in range(a.warmup):
                logistic_round()
            round_ms = windows(logistic_round, a.calls, a.repeats, sync)
            del bst, bins
        for kind in a.margins:
            margin = base if kind == "normal" else (torch.round(base * 8.0).clamp(-32, 31) / 8.0).contiguous()
            rec = {"shape": shape, "rows": m, "classes": classes, "margin_rows": K, "margins": kind,
                   "class_group": plan.group, "geometry": {"tile": A.COUNT_TILE, "threads": A.COUNT_THREADS,
                                                           "chunk": A.COUNT_CHUNK, "sort_tile": plan.sort_tile},
                   "ms_are": "least, median, largest per call", "logistic_round_ms": round_ms}
            step = lambda: plan.counts(margin)  # noqa: E731
            for _ in range(a.warmup):
                step()
            rec["auc_gpu_ms"] = windows(step, a.calls, a.repeats, sync)
            if plan.group >= K:  # one class group: the three stages can be timed alone, in their order
                rec["fill_ms"] = windows(lambda: plan._fill(margin, 0, K), a.calls, a.repeats, sync)
                rec["sort_ms"] = windows(lambda: plan._sort(K), a.calls, a.repeats, sync)
                rec["count_ms"] = windows(lambda: plan._count(0, K, A.COUNT_TILE, A.COUNT_THREADS, A.COUNT_CHUNK),
                                          a.calls, a.repeats, sync)
            u2 = plan.counts(margin)
            mh = margin.cpu().numpy()
            host = lambda: xgb.auc(margin.cpu().numpy(), y, a.host_threads, return_counts=True)  # noqa: E731
            score, (U2, P, N) = host()
            assert np.array_equal(U2, u2) and score == xgb.auc_score(u2, plan.P, plan.N)  # what is timed is equal
            rec["auc"] = score
            rec["readback_plus_host_auc_ms"] = windows(host, 1, 3, lambda: None)
            rec["host_auc_alone_ms"] = windows(lambda: xgb.auc(mh, y, a.host_threads), 1, 3, lambda: None)
            rec["host_threads"] = a.host_threads
            logloss = lambda: clf._metric(margin.cpu().numpy() if K > 1 else margin.cpu().numpy()[0], y)  # noqa: E731
            logloss()
            rec["readback_plus_numpy_logloss_ms"] = windows(logloss, 1, 3, lambda: None)
            rec["readback_alone_ms"] = windows(lambda: margin.cpu(), 1, 3, lambda: None)
            print(json.dumps(rec), flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(rec) + "\n")
        del plan, base
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
