"""Time of a reg:quantileerror boosting round of mifx.gbdt on the device, and of the leaf refresh inside it
(csrc/gbdt_quantile.hip), next to a squared-error round on the same bins.

Synthetic data: uniform random bins (32 features x 256 bins), y = bin of feature 0 / 64 + standard-normal noise,
depth 6. A squared-error round is gradients + grow (the grower updates the margins); a quantile round is gradients +
grow without margins + leaf refresh + apply of the refreshed tree to the training rows, exactly `fit`'s round. Every
figure is a host clock around a window of rounds that ends in a device synchronise, after warm-up rounds; a window is
repeated `--repeats` times and the least, median and largest time per round are recorded. The refresh alone is timed on
the state the last round left (same leaf_of_row, margins and hessians). `--sort-route` also times the obvious non-HIP
route at that size: torch.sort of the residuals, a stable torch.sort of their leaves, and a gather at each leaf's
rank (unweighted; it computes the same leaf values for unit hessians, which is checked). The select passes per leaf
are counted by the kernels, for float64 labels and for float32-widened labels at a zero intercept.

  python tools/bench_gbdt_quantile.py --sizes 100000 1000000 10000000 --sort-route 1000000 --out profiles/gbdt_quantile.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def windows(fn, rounds, repeats, sync):
    """[least, median, largest] milliseconds per call of fn over `repeats` windows of `rounds` calls"""
    out = []
    for _ in range(repeats):
        sync()
        t0 = time.perf_counter()
        for _ in range(rounds):
            fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3 / rounds)
    out.sort()
    return [round(out[0], 4), round(out[len(out) // 2], 4), round(out[-1], 4)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--alpha", type=float, default=0.9)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sort-route", type=int, default=0, help="the size at which the torch.sort route is timed too")
    ap.add_argument("--out", default=None, help="append one JSON line per size")
    a = ap.parse_args(argv)

    import torch

    from mifx.ops import gbdt_gpu as G

    dev = G.device_for(0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    eta, lam = 0.3, 1.0
    for n in a.sizes:
        gen = torch.Generator(device=dev).manual_seed(n)
        bins = torch.randint(0, 256, (n, a.features), generator=gen, device=dev, dtype=torch.int16)
        noise = torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
        y = bins[:, 0].double() / 64.0 + noise
        nbins = np.full(a.features, 256, np.int32)
        bst = G.Booster.from_device_bins(bins, nbins, a.max_depth)
        refresh = G.LeafRefresh(n, bst.cap, dev)
        tree = tuple(t[0] for t in bst.new_trees(1))
        stats = tuple(s[0] for s in bst.new_stats(1))
        g, h = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        rec = {"rows": n, "features": a.features, "max_depth": a.max_depth, "alpha": a.alpha, "rounds": a.rounds,
               "repeats": a.repeats, "ms_are": "least, median, largest per round"}

        def squared(margin):
            G.grad_hess("reg:squarederror", margin, y, g, h)
            bst.grow(g, h, tree, 1.0, lam, 0.0, eta, margin, stats=stats)

        def quantile(margin, yy=y):
            G.grad_hess("reg:quantileerror", margin, yy, g, h, alpha=a.alpha)
            bst.grow(g, h, tree, 1.0, lam, 0.0, eta, None, stats=stats)
            refresh(bst.leaf_of_row, tree[5], margin, yy, h, a.alpha, eta)
            bst.apply(bst.bins, tree, margin)

        for name, fn in (("squared_error_round_ms", squared), ("quantile_round_ms", quantile)):
            margin = torch.full((n,), float(y.mean()), dtype=torch.float64, device=dev)
            for _ in range(a.warmup):
                fn(margin)
            rec[name] = windows(lambda: fn(margin), a.rounds, a.repeats, sync)
        value = tree[5].clone()
        only = lambda: refresh(bst.leaf_of_row, value, margin, y, h, a.alpha, eta)  # noqa: E731
        only()
        rec["refresh_ms"] = windows(only, a.rounds, a.repeats, sync)
        rec["apply_ms"] = windows(lambda: bst.apply(bst.bins, tree, margin), a.rounds, a.repeats, sync)
        passes, leaves = refresh.stats()
        rec["float64_passes_per_leaf"] = round(passes / max(leaves, 1), 3)
        rec["leaves"] = leaves
        y32 = y.float().double()  # float32-widened labels at a zero intercept: the first round's residuals are y32
        quantile(torch.zeros(n, dtype=torch.float64, device=dev), y32)
        passes, leaves = refresh.stats()
        rec["float32_passes_per_leaf"] = round(passes / max(leaves, 1), 3)

        if n == a.sort_route:
            leaf = bst.leaf_of_row.long()
            cap = bst.cap

            def sort_route():
                r, order = torch.sort(y - margin)
                ls, o2 = torch.sort(leaf[order], stable=True)
                cnt = torch.bincount(ls, minlength=cap)
                off = torch.cumsum(cnt, 0) - cnt
                rank = torch.clamp(torch.ceil(a.alpha * cnt.double()).long(), min=1) - 1
                has = cnt > 0
                out = value.clone()
                out[has] = eta * r[o2[(off + rank)[has]]]
                return out

            ones = torch.ones_like(h)
            want = tree[5].clone()
            refresh(bst.leaf_of_row, want, margin, y, ones, a.alpha, eta)
            value.copy_(tree[5])
            rec["sort_route_equal"] = bool(torch.equal(sort_route(), want))
            rec["sort_route_ms"] = windows(sort_route, a.rounds, a.repeats, sync)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        del bst, refresh, bins, y, noise
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
