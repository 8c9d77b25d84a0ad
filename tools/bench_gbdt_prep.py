"""Feature preparation and prediction of mifx.gbdt on the device (csrc/gbdt_prep.hip) against the host functions of
csrc/gbdt.cpp, measured in one session.

Preparation, per size (standard-normal features, 32 of them, 256 bins):
  host    `_bin_matrix` (cuts + binning) and the `Booster(...)` upload of the host bins, as `fit` ran them before
  device  upload of the float64 table; per-column torch.sort (with the column copy and the NaN count); the cut kernels;
          the bin kernel -- each timed on its own (host clock around a window that ends in a device synchronise, after
          one warm-up pass), several repeats, min / median / max reported -- and the whole `device_cuts` + `device_bins`
          as `fit` runs them now.
Prediction (default 10^6 rows, 100 trees of depth 6): the host's mifx_gbdt_predict at --threads threads against the
forest kernel, with and without the upload of X.

Every run compares the device cuts and bins with the host's and the device predictions with the host's: a mismatch is
exit status 1.

  python tools/bench_gbdt_prep.py --sizes 10000 100000 1000000 10000000 --out profiles/gbdt_prep.jsonl
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--max-bins", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5, help="timed repeats of every device step")
    ap.add_argument("--host-repeats", type=int, default=2, help="timed repeats of the host preparation")
    ap.add_argument("--predict-rows", type=int, default=1_000_000, help="0: skip the prediction part")
    ap.add_argument("--predict-trees", type=int, default=100)
    ap.add_argument("--out", default=None, help="append one JSON line per measurement")
    a = ap.parse_args(argv)

    import torch

    from mifx.gbdt import XGBRegressor
    from mifx.ops import gbdt_gpu as G
    from mifx.ops import gbdt_prep as P

    dev = G.device_for(0)  # no GPU: an error, never a CPU number in a GPU column
    sync = torch.cuda.synchronize
    ok = True

    def timed(fn, repeats):
        out, ts = None, []
        for _ in range(repeats):
            sync()
            t0 = time.perf_counter()
            out = fn()
            sync()
            ts.append(time.perf_counter() - t0)
        return out, ts

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")

    with torch.cuda.device(dev):
        torch.zeros(1, device=dev)  # the context, outside every window
        for n in a.sizes:
            X = np.random.default_rng(n).standard_normal((n, a.features))
            host = XGBRegressor(max_bins=a.max_bins, n_jobs=a.threads)
            t_host, t_boost = [], []
            for _ in range(a.host_repeats):
                t0 = time.perf_counter()
                bins = host._bin_matrix(X)
                t_host.append(time.perf_counter() - t0)
                nbins = (host._ncut + 1).astype(np.int32)
                bst, ts = timed(lambda: G.Booster(bins, nbins, 6, dev), 1)
                t_boost += ts
                del bst
            # device, step by step (what device_cuts / device_bins do, with a synchronise after each step)
            fns = P._fns()
            scratch = torch.empty(fns["cut_scratch_bytes"](), dtype=torch.uint8, device=dev)
            cuts = torch.zeros((a.features, a.max_bins - 1), dtype=torch.float64, device=dev)
            count = torch.zeros(a.features, dtype=torch.int32, device=dev)
            tables = P.CutTables(host._cut_flat, host._cut_off, host._ncut, dev)

            def sort_all(Xd):
                return [(torch.sort(c).values, torch.isnan(c).sum())
                        for c in (Xd[:, j].contiguous().to(torch.float64) for j in range(a.features))]

            def cut_all(cols):
                for j, (srt, nan_count) in enumerate(cols):
                    P.check(fns["cuts"](P.ptr(srt), n, P.ptr(nan_count), a.max_bins, P.ptr(cuts[j]), P.ptr(count[j:]),
                                        P.ptr(scratch), P.CUT_BLOCKS, P.stream_handle(dev)), "mifx_gbdt_prep_cuts")

            def prepare(Xd):  # what fit runs
                c = P.device_cuts(Xd, a.max_bins)
                return c, P.device_bins(Xd, P.CutTables(c[1], c[2], c[3], dev))

            t_up, t_sort, t_cut, t_bin, t_all = [], [], [], [], []
            for rep in range(a.repeats + 1):  # the first pass is the warm-up
                Xd, ts_up = timed(lambda: torch.from_numpy(X).to(dev), 1)
                cols, ts_sort = timed(lambda: sort_all(Xd), 1)  # every sorted column is kept: one more table
                _, ts_cut = timed(lambda: cut_all(cols), 1)
                del cols
                dbins, ts_bin = timed(lambda: P.device_bins(Xd, tables), 1)
                del dbins
                res, ts_all = timed(lambda: prepare(Xd), 1)
                if rep:
                    for acc, ts in ((t_up, ts_up), (t_sort, ts_sort), (t_cut, ts_cut), (t_bin, ts_bin), (t_all, ts_all)):
                        acc += ts
                else:
                    (dc, dflat, doff, dncut), db = res
                    same_cuts = all(np.array_equal(u, v) for u, v in zip(dc, host._cuts)) and \
                        np.array_equal(dflat, host._cut_flat) and np.array_equal(doff, host._cut_off) and \
                        np.array_equal(dncut, host._ncut)
                    same_bins = np.array_equal(db.cpu().numpy().view(np.uint16), bins.T)
                del res, Xd
            torch.cuda.empty_cache()
            steps = statistics.median(t_sort) + statistics.median(t_cut) + statistics.median(t_bin)
            rec = {"what": "prep", "n": n, "features": a.features, "max_bins": a.max_bins, "host_threads": a.threads,
                   "host_bin_matrix_s": spread(t_host), "host_booster_upload_s": spread(t_boost),
                   "dev_upload_f64_s": spread(t_up), "dev_sort_s": spread(t_sort), "dev_cut_kernels_s": spread(t_cut),
                   "dev_bin_kernel_s": spread(t_bin), "dev_cuts_plus_bins_s": spread(t_all),
                   "sort_share_of_dev_steps": round(statistics.median(t_sort) / steps, 3),
                   "sort_share_of_dev_total": round(statistics.median(t_sort) / (steps + statistics.median(t_up)), 3),
                   "host_over_dev_incl_upload": round((min(t_host) + min(t_boost)) /
                                                      (statistics.median(t_up) + statistics.median(t_all)), 2),
                   "cuts_equal_host": bool(same_cuts), "bins_equal_host": bool(same_bins)}
            emit(rec)
            ok = ok and same_cuts and same_bins
            del X, bins

        if a.predict_rows:
            n = a.predict_rows
            r = np.random.default_rng(1)
            Xt = r.standard_normal((20_000, a.features))
            yt = Xt[:, 0] * Xt[:, 1] + np.abs(Xt[:, 2]) + 0.5 * Xt[:, 3] + r.normal(0, 0.1, len(Xt))
            model = XGBRegressor(n_estimators=a.predict_trees, max_depth=6, n_jobs=a.threads).fit(Xt, yt)
            X = r.standard_normal((n, a.features))
            X[r.random(X.shape) < 0.02] = np.nan
            want, t_host = None, []
            for _ in range(a.host_repeats + 1):
                t0 = time.perf_counter()
                want = model.predict(X)
                t_host.append(time.perf_counter() - t0)
            Xd = torch.from_numpy(X).to(dev)
            model.predict(Xd)  # warm-up: the packed forest goes up once per model
            got, t_dev = timed(lambda: model.predict(Xd), a.repeats)
            _, t_with = timed(lambda: model.predict(torch.from_numpy(X).to(dev)), a.repeats)
            same = np.array_equal(got.cpu().numpy().view(np.int64), want.view(np.int64))
            emit({"what": "predict", "n": n, "features": a.features, "trees": model.n_trees_,
                  "nodes": sum(len(t[0]) for t in model._trees), "max_depth": 6, "host_threads": a.threads,
                  "host_predict_s": spread(t_host[1:]), "dev_predict_s": spread(t_dev),
                  "dev_predict_with_upload_s": spread(t_with),
                  "host_over_dev": round(min(t_host) / statistics.median(t_dev), 1),
                  "host_over_dev_with_upload": round(min(t_host) / statistics.median(t_with), 1),
                  "predictions_equal_host": bool(same)})
            ok = ok and same
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
