"""A/B of the general fused Wide&Deep kernel (csrc/wd_general.hip) on one GPU.

Cells (each at B = 40 and B = 65536):
  * the default tower [100, 70, 48, 34]: general kernel vs the chained kernel -- what generality costs;
  * [100, 70, 50, 25], [64, 32], [256, 256, 256]: general kernel vs TorchWideDeepTrainer(device="cuda"), the PyTorch
    eager step, which is all a user could run for such a tower before the general kernel.

Method: all paths of a cell live in one process and are timed alternately, `--rounds` rounds (>= 3); the fused
trainers replay multi-step hipGraphs, the eager trainer runs its steps; every window ends in a device synchronise.
Per path: median and min / max of the rounds' us per step. One JSON line per (cell, path) goes to --out.

`--profile-step TOWER` instead runs a few eager general steps of one tower (for `rocprofv3 --kernel-trace --stats
-- python tools/bench_wd_general.py --profile-step 100,70,50,25`, in a run of its own).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import torch  # noqa: E402

from mifx.data.synthetic import synthetic_records  # noqa: E402
from mifx.models import wide_deep as wdm  # noqa: E402
from mifx.trainer.dispatch import make_wide_deep_trainer  # noqa: E402
from mifx.trainer.torch_wide_deep import TorchWideDeepTrainer  # noqa: E402

DEFAULT = wdm.dnn_hidden_units()
CELLS = [(DEFAULT, "chain"), ([100, 70, 50, 25], "eager"), ([64, 32], "eager"), ([256, 256, 256], "eager")]


def _model(hidden):
    return wdm.WideDeepModel(wdm.WideDeepConfig(hidden_units=list(hidden)), seed=0)


def _fused(hidden, batch, rec, kernel, spg):
    tr = make_wide_deep_trainer(_model(hidden), "cuda", batch=batch, kernel=kernel, shuffle_seed=3)
    tr.set_data(rec)
    tr.capture(warmup=3, steps_per_graph=spg)
    return tr


def _eager(hidden, batch, rec):
    tr = TorchWideDeepTrainer(_model(hidden), batch=batch, device="cuda", shuffle_seed=3)
    tr.set_data(rec)
    tr.run(3)
    return tr


def _time(tr, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.run(steps)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def bench(rounds: int, out: str, batches, spg: int) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        for batch in batches:
            rec = synthetic_records(max(4 * batch, 1 << 16), device="cuda", seed=3)
            for hidden, other in CELLS:
                paths = {"general": _fused(hidden, batch, rec, "general", spg)}
                paths[other] = _fused(hidden, batch, rec, "chain", spg) if other == "chain" \
                    else _eager(hidden, batch, rec)
                steps = {k: (4 * spg if k != "eager" else (40 if batch <= 1024 else 12)) for k in paths}
                times = {k: [] for k in paths}
                for _ in range(rounds):
                    for k, tr in paths.items():  # alternated inside every round
                        times[k].append(_time(tr, steps[k]))
                for k, v in times.items():
                    line = {"cell": f"{hidden}@{batch}", "hidden_units": hidden, "batch": batch, "path": k,
                            "steps_per_window": steps[k], "rounds": rounds, "us_per_step_median": statistics.median(v),
                            "us_per_step_min": min(v), "us_per_step_max": max(v), "us_per_step": v,
                            "grid": getattr(paths[k], "grid", None)}
                    print(json.dumps(line), flush=True)
                    f.write(json.dumps(line) + "\n")
                del paths
                torch.cuda.empty_cache()


def profile_step(hidden, batch: int, steps: int) -> None:
    rec = synthetic_records(max(4 * batch, 1 << 16), device="cuda", seed=3)
    tr = make_wide_deep_trainer(_model(hidden), "cuda", batch=batch, kernel="general", shuffle_seed=3)
    tr.set_data(rec)
    tr.run(steps)
    torch.cuda.synchronize()
    print(f"profiled {steps} general steps of {hidden} at batch {batch}, grid {tr.grid}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/wd_general.jsonl")
    ap.add_argument("--batches", default="40,65536")
    ap.add_argument("--steps-per-graph", type=int, default=50)
    ap.add_argument("--profile-step", default=None, help="comma-separated hidden units: run eager general steps only")
    ap.add_argument("--profile-batch", type=int, default=65536)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wd_general needs a GPU")
    if a.profile_step:
        profile_step([int(x) for x in a.profile_step.split(",")], a.profile_batch, 10)
        return 0
    if a.rounds < 3:
        raise SystemExit("--rounds must be at least 3")
    bench(a.rounds, a.out, [int(b) for b in a.batches.split(",")], a.steps_per_graph)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
