"""Feature contributions (path-dependent TreeSHAP) on the device (csrc/gbdt_prep.hip, k_contribs) against the host
function (csrc/gbdt.cpp, mifx_gbdt_contribs, --threads threads).

A regressor (--features standard-normal features, --trees trees of depth --max-depth) is trained on the device on
--train-rows rows; fresh rows are then explained. Per size: the device kernel on a resident float64 table (host clock
around one call that ends in a device synchronise, one warm-up, --repeats repeats, min / median / max), the same with
the table's upload and the result's read-back inside the window, and the host function on at most --host-rows of the
rows (its time scales with the rows; the ratio is taken per row). The device result must equal the host's bit for bit
on the rows both computed: a mismatch is exit status 1. "model_gflops" counts, per (row, leaf) with m path elements,
2 m (m + 1) operations for EXTEND, 4 m^2 for UNWIND and 3 m for the products (the branch taken where o = 1).
--routes also times both accumulation routes ("lds" with the largest workgroup that fits, "output" with 256 threads)
and the workgroup sizes; --num-class K times a K-class model (one launch per class over class-major tables).

  python tools/bench_gbdt_contribs.py --sizes 10000 100000 1000000 --out profiles/gbdt_contribs.jsonl
  python tools/bench_gbdt_contribs.py --sizes 100000 --max-depth 12 --trees 10 --out profiles/gbdt_contribs.jsonl
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


def timed(fn, repeats):
    import torch

    ts, out = [], None
    for rep in range(repeats + 1):  # the first pass warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep:
            ts.append(time.perf_counter() - t0)
    return ts, out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--num-class", type=int, default=0, help="0: a regressor; K >= 3: a K-class classifier")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-rows", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--routes", action="store_true", help="also time every accumulation route and workgroup size")
    ap.add_argument("--out", default=None, help="append one JSON line per measurement")
    a = ap.parse_args(argv)

    import torch

    from mifx.gbdt import XGBClassifier, XGBRegressor
    from mifx.ops import gbdt_gpu as G
    from mifx.ops import gbdt_prep as P

    dev = G.device_for(0)  # no GPU: an error, never a CPU number in a GPU column
    r = np.random.default_rng(a.features)
    Xt = r.standard_normal((a.train_rows, a.features))
    y = Xt[:, 0] * Xt[:, 1] + np.abs(Xt[:, 2]) + 0.5 * Xt[:, 3] + r.normal(0, 0.1, a.train_rows)
    kw = dict(n_estimators=a.trees, max_depth=a.max_depth, device="gpu", n_jobs=a.threads)
    if a.num_class:
        y = np.searchsorted(np.quantile(y, np.arange(1, a.num_class) / a.num_class), y)
        model = XGBClassifier(**kw).fit(Xt, y)
    else:
        model = XGBRegressor(**kw).fit(Xt, y)
    K = model._num_class()
    tables = model._path_tables(model._tree_limit())
    m = np.concatenate([t.recs["i"][t.leaf_off[:-1]] for t in tables]).astype(np.float64)
    flops_per_row = float((2 * m * (m + 1) + 4 * m * m + 3 * m).sum())
    ok = True
    with torch.cuda.device(dev):
        for n in a.sizes:
            X = r.standard_normal((n, a.features))
            X[r.random(X.shape) < 0.05] = np.nan
            Xd = torch.from_numpy(X).to(dev)
            t_dev, out = timed(lambda: model.predict_contribs(Xd), a.repeats)
            t_up, _ = timed(lambda: model.predict_contribs(torch.from_numpy(X).to(dev)).cpu(), a.repeats)
            hn = min(n, a.host_rows)
            t0 = time.perf_counter()
            want = model.predict_contribs(X[:hn])
            t_host = time.perf_counter() - t0
            same = bool(np.array_equal(out[:hn].cpu().numpy().view(np.uint64), want.view(np.uint64)))
            ok &= same
            rec = {"what": "contribs", "n": n, "features": a.features, "trees": model.n_trees_, "num_class": K,
                   "max_depth": a.max_depth, "leaves": int(len(m)), "records": int(sum(t.n_recs(t.n_trees) for t in tables)),
                   "mean_path_elements": round(float(m.mean()), 3), "route": "lds" if P.contrib_lds_threads(a.features)
                   else "output", "workgroup": P.contrib_lds_threads(a.features) or 256,
                   "recs_per_chunk": P.RECS_PER_CHUNK,
                   "device_s": spread(t_dev), "device_with_transfers_s": spread(t_up), "host_rows": hn,
                   "host_threads": a.threads, "host_s": round(t_host, 4),
                   "host_over_device_per_row": round((t_host / hn) / (min(t_dev) / n), 1),
                   "model_gflops": round(flops_per_row * n / min(t_dev) / 1e9, 1), "equal_bits": same}
            if a.routes and K == 1:
                dp = P.DevicePaths(tables[0], dev)
                buf = torch.empty((n, a.features + 1), dtype=torch.float64, device=dev)
                fits = P.contrib_lds_threads(a.features)
                for route, threads in [("lds", t) for t in (256, 128, 64) if t <= fits] + \
                                      [("output", t) for t in (256, 128, 64)]:
                    ts, _ = timed(lambda: P.contribs(dp, Xd, model._base_margin, buf, None, None, route, threads),
                                  a.repeats)
                    rec[f"{route}_{threads}_s"] = spread(ts)
                    ok &= bool(torch.equal(buf.view(torch.int64), out.view(torch.int64)))
                for chunk in (64, 128, 256, 512, 1024):  # records staged at a time, on the default route
                    ts, _ = timed(lambda: P.contribs(dp, Xd, model._base_margin, buf, None, chunk), a.repeats)
                    rec[f"chunk_{chunk}_s"] = spread(ts)
                    rec[f"chunk_{chunk}_workgroup"] = P.contrib_lds_threads(a.features, chunk) or 256
                    ok &= bool(torch.equal(buf.view(torch.int64), out.view(torch.int64)))
            print(json.dumps(rec), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(rec) + "\n")
            del Xd, out
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
