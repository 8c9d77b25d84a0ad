"""SHAP interaction values on the device (csrc/gbdt_interactions.hip, k_interactions, after one k_contribs launch)
against the host function (csrc/gbdt.cpp, mifx_gbdt_interactions, --threads threads).

A regressor (--features standard-normal features, --trees trees of depth --max-depth) is trained on the device on
--train-rows rows; fresh rows are then explained. Per size: predict_interactions of a resident float64 table (host
clock around one call that ends in a device synchronise, one warm-up, --repeats repeats, min / median / max), the
same with the table's upload and the result's read-back inside the window, predict_contribs of the same table the
same way, and the host function on at most --host-rows of the rows (its time scales with the rows; the ratio is taken
per row). The device result must equal the host's bit for bit on the rows both computed: a mismatch is exit status 1.
--routes also times both accumulation routes and the workgroup sizes that fit.

  python tools/bench_gbdt_interactions.py --sizes 10000 100000 --routes --out profiles/gbdt_interactions.jsonl
  python tools/bench_gbdt_interactions.py --sizes 100000 --features 6 --routes --out profiles/gbdt_interactions.jsonl
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_gbdt_contribs import spread, timed  # noqa: E402


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--train-rows", type=int, default=100_000)
    ap.add_argument("--features", type=int, default=32)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-rows", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--routes", action="store_true", help="also time every accumulation route and workgroup size")
    ap.add_argument("--out", default=None, help="append one JSON line per measurement")
    a = ap.parse_args(argv)

    import torch

    from mifx.gbdt import XGBRegressor
    from mifx.ops import gbdt_gpu as G
    from mifx.ops import gbdt_prep as P

    dev = G.device_for(0)  # no GPU: an error, never a CPU number in a GPU column
    r = np.random.default_rng(a.features)
    Xt = r.standard_normal((a.train_rows, a.features))
    y = Xt[:, 0] * Xt[:, 1] + np.abs(Xt[:, 2]) + 0.5 * Xt[:, 3] + r.normal(0, 0.1, a.train_rows)
    model = XGBRegressor(n_estimators=a.trees, max_depth=a.max_depth, device="gpu", n_jobs=a.threads).fit(Xt, y)
    tab = model._path_tables(model._tree_limit())[0]
    m = tab.recs["i"][tab.leaf_off[:-1]].astype(np.float64)
    off, _, _, rec = tab.feature_leaves()
    w = a.features + 1
    ok = True
    with torch.cuda.device(dev):
        for n in a.sizes:
            X = r.standard_normal((n, a.features))
            X[r.random(X.shape) < 0.05] = np.nan
            Xd = torch.from_numpy(X).to(dev)
            t_dev, out = timed(lambda: model.predict_interactions(Xd), a.repeats)
            t_up, _ = timed(lambda: model.predict_interactions(torch.from_numpy(X).to(dev)).cpu(), a.repeats)
            t_phi, _ = timed(lambda: model.predict_contribs(Xd), a.repeats)
            hn = min(n, a.host_rows)
            t0 = time.perf_counter()
            want = model.predict_interactions(X[:hn])
            t_host = time.perf_counter() - t0
            same = bool(np.array_equal(out[:hn].cpu().numpy().view(np.uint64), want.view(np.uint64)))
            ok &= same
            fits = P.contrib_lds_threads(a.features)
            rec_ = {"what": "interactions", "n": n, "features": a.features, "trees": model.n_trees_,
                    "max_depth": a.max_depth, "leaves": int(len(m)), "mean_path_elements": round(float(m.mean()), 3),
                    "list_entries": int(off[-1]), "list_records": int(rec[-1]), "output_bytes": 8 * n * w * w,
                    "route": "lds" if fits else "output", "workgroup": fits or 256, "recs_per_chunk": P.RECS_PER_CHUNK,
                    "device_s": spread(t_dev), "device_with_transfers_s": spread(t_up), "contribs_device_s": spread(t_phi),
                    "over_contribs": round(min(t_dev) / min(t_phi), 2), "host_rows": hn, "host_threads": a.threads,
                    "host_s": round(t_host, 4), "host_over_device_per_row": round((t_host / hn) / (min(t_dev) / n), 1),
                    "equal_bits": same}
            if a.routes:
                dp = model._device_paths(dev, [tab])[0]
                buf = torch.empty((n, w, w), dtype=torch.float64, device=dev)
                for route, threads in [("lds", t) for t in (256, 128, 64) if t <= fits] + \
                                      [("output", t) for t in (256, 128, 64)]:
                    ts, _ = timed(lambda: P.interactions(dp, Xd, model._base_margin, buf, None, None, route, threads),
                                  a.repeats)
                    rec_[f"{route}_{threads}_s"] = spread(ts)
                    ok &= bool(torch.equal(buf.view(torch.int64), out.view(torch.int64)))
                del buf
            print(json.dumps(rec_), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(rec_) + "\n")
            del Xd, out
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
