"""Time of one boosting round (squared-error gradients + one tree) on the device with per-node feature sets
(csrc/gbdt_nodeset.h: k_nodeset and the per-node masks of the split and histogram kernels) against the default round:

  default   no node sets: the entry points and kernels of a plain round
  groups    interaction_constraints = --groups disjoint groups of equal size over the features
  bynode    colsample_bynode = 0.5

Synthetic data: uniform random bins (32 features x 256 bins); y is a sum of products of neighbouring features and noise,
so every feature carries signal and the trees fill their depth. The variants alternate window by window on the same
bins; every figure is a host clock around a window of calls that ends in a device synchronise, after warm-up calls; a
window is repeated `--repeats` times and the least, median and largest time per call are recorded.
`--variants default` runs on a tree without node sets too (an A/B of two builds of the library is two runs of it).

  python tools/bench_gbdt_nodeset.py --rows 1000000 10000000 --out profiles/gbdt_nodeset.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_gbdt_monotone import spread, window  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", nargs="+", type=int, default=[100000])
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--max-leaves", type=int, default=0, help="> 0: leaf-wise growth with this budget, no depth limit")
    ap.add_argument("--variants", nargs="+", default=["default", "groups", "bynode"])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--label", default="", help="copied into the record (which build ran)")
    ap.add_argument("--out", default=None, help="append one JSON line per shape")
    a = ap.parse_args(argv)

    import numpy as np
    import torch

    from mifx.ops import gbdt_gpu as G

    dev = G.device_for(0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    f, per = a.features, a.features // a.groups
    specs = {"default": None, "groups": ([list(range(i * per, (i + 1) * per)) for i in range(a.groups)], 1.0),
             "bynode": (None, 0.5)}
    nbins = np.full(f, 256, np.int32)
    for n in a.rows:
        gen = torch.Generator(device=dev).manual_seed(n)
        bins = torch.randint(0, 256, (n, f), generator=gen, device=dev, dtype=torch.int16)
        x = bins.double() / 128.0 - 1.0
        y = (x * x.roll(1, dims=1)).sum(dim=1) + 0.3 * torch.randn(n, generator=gen, device=dev, dtype=torch.float64)
        del x
        g, h = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        rec = {"label": a.label, "rows": n, "features": f, "max_depth": a.max_depth, "max_leaves": a.max_leaves,
               "calls": a.calls, "repeats": a.repeats, "ms_are": "least, median, largest per call"}
        rounds = {}
        for name in a.variants:
            kw = {} if specs[name] is None else {"nodeset": specs[name]}  # (a build without node sets has no keyword)
            bst = G.LossguideBooster.from_device_bins(bins, nbins, 0, a.max_leaves, **kw) if a.max_leaves else \
                G.Booster.from_device_bins(bins, nbins, a.max_depth, **kw)
            tree = tuple(t[0] for t in bst.new_trees(1))
            margin = torch.zeros(n, dtype=torch.float64, device=dev)

            def one_round(bst=bst, tree=tree, margin=margin):
                margin.zero_()  # every call grows the first round's tree
                G.grad_hess("reg:squarederror", margin, y, g, h)
                bst.grow(g, h, tree, 1.0, 1.0, 0.0, 0.3, margin)

            for _ in range(a.warmup):
                one_round()
            sync()
            rounds[name] = one_round
            rec[name + "_nodes"] = int(tree[6].reshape(-1)[0].item())
        ms = {name: [] for name in a.variants}
        for _ in range(a.repeats):  # alternate, so drift hits all alike
            for name in a.variants:
                ms[name].append(window(rounds[name], a.calls, sync))
        for name in a.variants:
            rec[name + "_ms"] = spread(ms[name])
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
        del bins, y, rounds, bst
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
