"""Time of one boosting round (squared-error gradients + one tree) on the device with monotone_constraints against the
same round without them, depth-wise (k_split_mono / k_decide_mono of csrc/gbdt_gpu.hip) and leaf-wise (k_split_mono of
csrc/gbdt_lossguide.hip).

Synthetic data: uniform random bins (32 features x 256 bins); y follows feature 0 up and down (a sine over its bins),
falls with feature 1 and carries noise, so under the constraints (+1, -1, 0, ...) candidates are rejected and weights
clamped. The constrained and the unconstrained round alternate window by window on the same bins; every figure is a
host clock around a window of calls that ends in a device synchronise, after warm-up calls; a window is repeated
`--repeats` times and the least, median and largest time per call are recorded.

  python tools/bench_gbdt_monotone.py --rows 100000 1000000 10000000 --out profiles/gbdt_monotone.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window(fn, calls, sync):
    sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / calls


def spread(ms):
    ms = sorted(ms)
    return [round(ms[0], 4), round(ms[len(ms) // 2], 4), round(ms[-1], 4)]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", nargs="+", type=int, default=[100000])
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--max-leaves", type=int, default=64)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="append one JSON line per shape")
    a = ap.parse_args(argv)

    import torch

    from mifx.ops import gbdt_gpu as G

    dev = G.device_for(0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    mono = np.zeros(a.features, np.int32)
    mono[:2] = (1, -1)
    nbins = np.full(a.features, 256, np.int32)
    for n in a.rows:
        gen = torch.Generator(device=dev).manual_seed(n)
        bins = torch.randint(0, 256, (n, a.features), generator=gen, device=dev, dtype=torch.int16)
        y = torch.sin(bins[:, 0].double() / 20.0) - bins[:, 1].double() / 256.0 + \
            0.3 * torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
        g, h = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        rec = {"rows": n, "features": a.features, "max_depth": a.max_depth, "max_leaves": a.max_leaves,
               "calls": a.calls, "repeats": a.repeats, "ms_are": "least, median, largest per call"}
        for policy in ("depthwise", "lossguide"):
            rounds = {}
            for name, m in (("free", None), ("mono", mono)):
                bst = G.Booster.from_device_bins(bins, nbins, a.max_depth, m) if policy == "depthwise" else \
                    G.LossguideBooster.from_device_bins(bins, nbins, 0, a.max_leaves, m)
                tree = tuple(t[0] for t in bst.new_trees(1))
                stats = tuple(s[0] for s in bst.new_stats(1))
                margin = torch.zeros(n, dtype=torch.float64, device=dev)

                def one_round(bst=bst, tree=tree, stats=stats, margin=margin):
                    margin.zero_()  # every call grows the first round's tree
                    G.grad_hess("reg:squarederror", margin, y, g, h)
                    bst.grow(g, h, tree, 1.0, 1.0, 0.0, 0.3, margin, stats=stats)

                for _ in range(a.warmup):
                    one_round()
                sync()
                rounds[name] = (one_round, int(tree[6].reshape(-1)[0].item()))
            ms = {"free": [], "mono": []}
            for _ in range(a.repeats):  # alternate, so drift hits both alike
                for name in ("free", "mono"):
                    ms[name].append(window(rounds[name][0], a.calls, sync))
            rec[policy] = {"free_ms": spread(ms["free"]), "mono_ms": spread(ms["mono"]),
                           "free_nodes": rounds["free"][1], "mono_nodes": rounds["mono"][1],
                           "ratio_of_medians": round(spread(ms["mono"])[1] / spread(ms["free"])[1], 4)}
            del rounds, bst
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        del bins, y
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
