"""Multi-class forest prediction on the device (csrc/gbdt_prep.hip): the one-launch kernel k_predict_multi against the
code it replaces, K launches of k_predict over class-strided forests (trees k, k + K, ... of class k) on the same
device table.

A K-class model (32 standard-normal features, depth 6, --rounds rounds, so rounds x K trees) is trained on the device on
--train-rows rows; --rows fresh rows are then predicted, float64 and float32 tables. Three routes, timed alternately
(host clock around one call that ends in a device synchronise, one warm-up each, --repeats repeats, min / median / max):
  one_launch_registers   one walk of the forest with the class sums in registers (K <= 16)
  one_launch_in_output   one walk, every thread accumulating in its own elements of the output (any K)
  k_launches             the single-output kernel once per class over a class-major copy of the forest
All three must give the same bits as each other: a mismatch is exit status 1.

  python tools/bench_gbdt_multiclass_predict.py --out profiles/gbdt_multiclass.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ts):
    return {"min": round(min(ts), 6), "median": round(statistics.median(ts), 6), "max": round(max(ts), 6)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--num-class", type=int, nargs="+", default=[3])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="append one JSON line per measurement")
    a = ap.parse_args(argv)

    import torch

    from mifx.gbdt import XGBClassifier
    from mifx.ops import gbdt_gpu as G
    from mifx.ops import gbdt_prep as P

    dev = G.device_for(0)  # no GPU: an error, never a CPU number in a GPU column
    ok = True
    with torch.cuda.device(dev):
        for K in a.num_class:
            r = np.random.default_rng(K)
            Xt = r.standard_normal((a.train_rows, a.features))
            s = Xt[:, 0] * Xt[:, 1] + np.abs(Xt[:, 2]) + 0.5 * Xt[:, 3] + r.normal(0, 0.1, a.train_rows)
            y = np.searchsorted(np.quantile(s, np.arange(1, K) / K), s)
            model = XGBClassifier(n_estimators=a.rounds, max_depth=6, device="gpu").fit(Xt, y)
            trees, base = model._trees, model._base_margin
            forest = P.DeviceForest(trees, a.features, dev)
            X = r.standard_normal((a.rows, a.features))
            for dtype in (np.float64, np.float32):
                Xd = torch.from_numpy(X.astype(dtype)).to(dev)
                routes = {"k_launches": lambda: P.predict_multi(forest, Xd, base, K, _route="launches"),
                          "one_launch_in_output": lambda: P.predict_multi(forest, Xd, base, K, _route="output")}
                if K <= P._fns()["reg_classes"]():
                    routes["one_launch_registers"] = lambda: P.predict_multi(forest, Xd, base, K, _route="registers")
                outs, times = {}, {name: [] for name in routes}
                for rep in range(a.repeats + 1):  # the first pass warms up; the routes alternate
                    for name, fn in routes.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        outs[name] = fn()
                        torch.cuda.synchronize()
                        if rep:
                            times[name].append(time.perf_counter() - t0)
                same = all(torch.equal(o.view(torch.int64), outs["k_launches"].view(torch.int64))
                           for o in outs.values())
                ok &= same
                rec = {"what": "predict_multi", "n": a.rows, "features": a.features, "num_class": K,
                       "trees": len(trees), "nodes": int(sum(len(t[0]) for t in trees)),
                       "dtype": np.dtype(dtype).name, "repeats": a.repeats,
                       **{name + "_s": spread(ts) for name, ts in times.items()}, "routes_equal": bool(same)}
                print(json.dumps(rec), flush=True)
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "a") as fh:
                        fh.write(json.dumps(rec) + "\n")
                del Xd, outs
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
