"""What differentially private Wide&Deep training costs on one GPU (csrc/wd_general.hip, DP mode).

Cells: tower [100, 70, 50, 25] and the taxi default [100, 70, 48, 34], each at B = 40, 4096 and 65536. Routes:
  * "dp":      GeneralWideDeepTrainer(dp=DPSpec(C, sigma)) -- per-example clipping inside the fused step, noise in the
               reduce / optimizer pass; multi-step hipGraphs;
  * "general": the same trainer without DP (kernel="general" forced for the taxi tower) -- the baseline the extra
               norm sweep is paid against; multi-step hipGraphs;
  * "dpopt":   privacy.DPOptimizer on WideDeepModel with num_microbatches = B (torch.func.vmap per-example gradients,
               a materialised G[B, P], csrc/dp.hip) -- the only private route before the DP mode. clip_sum_noise takes
               at most 4096 rows per call, so larger batches are processed in chunks of 4096 (recorded as "chunked");
               an out-of-memory failure is recorded, not hidden.

Method: the routes of a cell live in one process and are timed alternately, `--rounds` rounds (>= 3); every window
ends in a device synchronise; all shapes are warmed up first. Per route: median and min / max of the rounds' us per
step. One JSON line per (cell, route) goes to --out.

`--profile-step TOWER` instead runs a few eager DP and non-DP steps of one tower (for `rocprofv3 --kernel-trace
--stats -- python tools/bench_wd_dp.py --profile-step 100,70,50,25`, in a run of its own).
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
from mifx.privacy import DPOptimizer, DPSpec  # noqa: E402
from mifx.trainer.dispatch import make_wide_deep_trainer  # noqa: E402

TOWERS = [[100, 70, 50, 25], wdm.dnn_hidden_units()]
SPEC = DPSpec(l2_norm_clip=1.5, noise_multiplier=1.1, seed=1)  # C near the median norm of a fresh model
FUSED_ROWS = 4096  # clip_sum_noise's row bound


def _model(hidden):
    return wdm.WideDeepModel(wdm.WideDeepConfig(hidden_units=list(hidden)), seed=0)


def _fused(hidden, batch, rec, spg, dp):
    tr = make_wide_deep_trainer(_model(hidden), "cuda", batch=batch, kernel="general", shuffle_seed=3, dp=dp)
    tr.set_data(rec)
    tr.capture(warmup=3, steps_per_graph=spg)
    return tr


class _Packed(torch.nn.Module):
    """WideDeepModel behind the one-tensor input DPOptimizer's vmap route calls: [.., 3 dense floats | 9 ids]."""

    def __init__(self, model):
        super().__init__()
        self.m = model

    def forward(self, x):
        return self.m(x[..., :3], x[..., 3:].long())


class _DPOpt:
    """DPOptimizer(Adagrad) on WideDeepModel, num_microbatches = B, consecutive batches of the record set."""

    def __init__(self, hidden, batch, rec):
        self.model = _Packed(_model(hidden)).cuda()
        dense, ids, label = wdm.records_to_tensors(rec.cpu())
        self.x = torch.cat([dense, ids.float()], 1).cuda()
        self.y = label.cuda()
        self.batch, self.pos = batch, 0
        p = sum(q.numel() for q in self.model.parameters())
        self.chunked = batch > FUSED_ROWS
        self.opt = DPOptimizer(torch.optim.Adagrad(self.model.parameters(), lr=0.05), SPEC.l2_norm_clip,
                               SPEC.noise_multiplier, num_microbatches=batch, seed=SPEC.seed,
                               max_g_bytes=min(8 << 30, FUSED_ROWS * p * 4))
        self.loss_fn = lambda out, y: torch.nn.functional.binary_cross_entropy_with_logits(out, y, reduction="none")

    def run(self, n):
        for _ in range(n):
            if self.pos + self.batch > self.x.shape[0]:
                self.pos = 0
            sl = slice(self.pos, self.pos + self.batch)
            self.opt.step(self.model, self.loss_fn, self.x[sl], self.y[sl])
            self.pos += self.batch


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
            for hidden in TOWERS:
                paths = {"dp": _fused(hidden, batch, rec, spg, SPEC), "general": _fused(hidden, batch, rec, spg, None)}
                failed = {}
                try:
                    paths["dpopt"] = _DPOpt(hidden, batch, rec)
                    paths["dpopt"].run(2 if batch <= 4096 else 1)  # warm-up of every shape
                    torch.cuda.synchronize()
                except (torch.OutOfMemoryError, RuntimeError, ValueError) as e:
                    paths.pop("dpopt", None)
                    failed["dpopt"] = f"{type(e).__name__}: {str(e)[:200]}"
                    torch.cuda.empty_cache()
                # windows of 0.1 s and more; the replaced route at B = 65,536: a few steps only
                steps = {k: (40 * spg if k != "dpopt" else (100 if batch <= 4096 else 5)) for k in paths}
                times = {k: [] for k in paths}
                for _ in range(rounds):
                    for k, tr in paths.items():  # alternated inside every round
                        times[k].append(_time(tr, steps[k]))
                for k, v in times.items():
                    line = {"cell": f"{hidden}@{batch}", "hidden_units": hidden, "batch": batch, "route": k,
                            "steps_per_window": steps[k], "rounds": rounds, "us_per_step_median": statistics.median(v),
                            "us_per_step_min": min(v), "us_per_step_max": max(v), "us_per_step": v,
                            "grid": getattr(paths[k], "grid", None), "chunked": getattr(paths[k], "chunked", None),
                            "l2_norm_clip": SPEC.l2_norm_clip, "noise_multiplier": SPEC.noise_multiplier}
                    if k == "dp":
                        line["clipped_fraction"] = float((paths[k].last_norms() > SPEC.l2_norm_clip).float().mean())
                    print(json.dumps(line), flush=True)
                    f.write(json.dumps(line) + "\n")
                for k, why in failed.items():
                    line = {"cell": f"{hidden}@{batch}", "hidden_units": hidden, "batch": batch, "route": k,
                            "failed": why}
                    print(json.dumps(line), flush=True)
                    f.write(json.dumps(line) + "\n")
                del paths
                torch.cuda.empty_cache()


def profile_step(hidden, batch: int, steps: int) -> None:
    rec = synthetic_records(max(4 * batch, 1 << 16), device="cuda", seed=3)
    for dp in (SPEC, None):
        tr = make_wide_deep_trainer(_model(hidden), "cuda", batch=batch, kernel="general", shuffle_seed=3, dp=dp)
        tr.set_data(rec)
        tr.run(steps)
        torch.cuda.synchronize()
        print(f"profiled {steps} general steps (dp={dp is not None}) of {hidden} at batch {batch}, grid {tr.grid}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/wd_dp.jsonl")
    ap.add_argument("--batches", default="40,4096,65536")
    ap.add_argument("--steps-per-graph", type=int, default=50)
    ap.add_argument("--profile-step", default=None, help="comma-separated hidden units: run eager steps only")
    ap.add_argument("--profile-batch", type=int, default=65536)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_wd_dp needs a GPU")
    if a.profile_step:
        profile_step([int(x) for x in a.profile_step.split(",")], a.profile_batch, 10)
        return 0
    if a.rounds < 3:
        raise SystemExit("--rounds must be at least 3")
    bench(a.rounds, a.out, [int(b) for b in a.batches.split(",")], a.steps_per_graph)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
