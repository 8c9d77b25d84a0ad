"""BERT-base fine-tuning on packed variable-length batches against the padded trainer (mifx/trainer/bert_trainer.py).

Per length distribution, one set of synthetic sequences is trained on by both trainers in the same process, each step
replayed from its hipGraph: padded in batches of B = 32 at S = 128 with the attention mask, packed with as many of the
same sequences per step as fit C = 4096 tokens (plan_train_batches, in order). A timed window is whole passes over the
set, a new batch set before every step (host packing / padding and the H2D copy included: what a training loop pays),
started and ended by a device synchronise and at least `--window` seconds long; the two trainers alternate, `--rounds`
windows each, and the median and the spread (min .. max) are reported. Every batch shape is warmed up (one pass, which
also captures the graphs) before the first window. `step_ms` is the GPU step time of replays of one batch without the
host's feeding (the first batch of the set), `ns_per_token` the fed window time per REAL token.

Usage: python tools/bench_bert_packed_train.py [--dists all128 uniform64 uniform16] [--rounds 5] [--window 0.4]
                                               [--out FILE.jsonl]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mifx.models.bert import BertConfig  # noqa: E402
from mifx.models.bert_infer import _pad_arrays  # noqa: E402
from mifx.trainer.bert_trainer import BertTrainer, load_gemm_table, plan_train_batches, synthetic_sequences  # noqa: E402

DISTS = {"all128": (128, 128), "uniform64": (64, 128), "uniform16": (16, 128)}


def window(feed_pass, min_s: float) -> tuple:
    """(seconds, passes) of whole passes lasting at least min_s, between two device synchronises."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        feed_pass()
        n += 1
        if time.perf_counter() - t0 >= min_s:
            torch.cuda.synchronize()
            return time.perf_counter() - t0, n


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dists", nargs="*", default=list(DISTS), choices=list(DISTS))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--packed-tokens", type=int, default=4096)
    ap.add_argument("--max-seqs", type=int, default=None)
    ap.add_argument("--sequences", type=int, default=512, help="sequences of a pass (a multiple of --batch)")
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_bert_packed_train needs a GPU (no CPU timing is meaningful)")
    if a.sequences % a.batch:
        ap.error("--sequences must be a multiple of --batch")
    torch.manual_seed(a.seed)
    load_gemm_table()
    cfg = BertConfig(layers=a.layers)
    padded = BertTrainer(cfg, a.batch, a.seq, "cuda")
    packed = BertTrainer(cfg, a.batch, a.seq, "cuda", packed_tokens=a.packed_tokens, max_seqs=a.max_seqs, max_len=a.seq)
    rows = []
    for dist in a.dists:
        lo, hi = DISTS[dist]
        seqs, tts, ys = synthetic_sequences(cfg, a.sequences, lo, hi, seed=a.seed + 1)
        tokens = sum(len(s) for s in seqs)
        pad_batches = []
        for i in range(0, a.sequences, a.batch):
            arr = _pad_arrays(seqs[i:i + a.batch], tts[i:i + a.batch], a.seq)
            pad_batches.append([torch.from_numpy(x).pin_memory() for x in arr]
                               + [torch.from_numpy(ys[i:i + a.batch]).pin_memory()])
        groups = list(plan_train_batches([len(s) for s in seqs], packed.packed_tokens, packed.max_seqs))
        pk_batches = [([seqs[j] for j in g], [tts[j] for j in g], ys[g]) for g in groups]

        def pass_padded():
            for b in pad_batches:
                padded.set_batch(*b)
                padded.step()

        def pass_packed():
            for b in pk_batches:
                packed.set_packed_batch(*b)
                packed.step()

        def replay(tr, steps=20):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps

        runs = {"padded": pass_padded, "packed": pass_packed}
        for r in runs.values():  # warm-up: every batch of the pass once (captures the graphs on first use)
            r()
        torch.cuda.synchronize()
        t = {k: [] for k in runs}
        for _ in range(a.rounds):  # alternate the two trainers
            for k, r in runs.items():
                dt, n = window(r, a.window)
                t[k].append(dt / n)
        padded.set_batch(*pad_batches[0])
        packed.set_packed_batch(*pk_batches[0])
        step = {"padded": [], "packed": []}
        for _ in range(a.rounds):
            step["padded"].append(replay(padded))
            step["packed"].append(replay(packed))
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"dist": dist, "length_range": [lo, hi], "sequences": a.sequences, "tokens_real": tokens,
               "padded_steps": len(pad_batches), "padded_rows_per_step": a.batch * a.seq,
               "packed_steps": len(pk_batches), "packed_rows_per_step": packed.packed_tokens,
               "packed_seqs_per_step": a.sequences / len(pk_batches), "packed_max_seqs": packed.max_seqs,
               "loss_padded": float(padded.static_loss), "loss_packed": float(packed.static_loss)}
        if not all(x == x and abs(x) != float("inf") for x in (row["loss_padded"], row["loss_packed"])):
            raise SystemExit(f"non-finite loss: {row}")  # never report the speed of garbage
        for k in runs:
            row[f"{k}_seq_s"] = a.sequences / med[k]
            row[f"{k}_seq_s_min_max"] = [a.sequences / max(t[k]), a.sequences / min(t[k])]
            row[f"{k}_ns_per_token"] = med[k] / tokens * 1e9
            row[f"{k}_step_ms"] = statistics.median(step[k]) * 1e3
            row[f"{k}_step_ms_min_max"] = [min(step[k]) * 1e3, max(step[k]) * 1e3]
        row["speedup"] = med["padded"] / med["packed"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    print("\n| lengths | real tokens | padded steps x rows | packed steps x rows (seqs / step) | padded seq/s (min .. max)"
          " | packed seq/s (min .. max) | padded ns / token | packed ns / token | padded step ms | packed step ms |"
          " packed / padded |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        pm, km = r["padded_seq_s_min_max"], r["packed_seq_s_min_max"]
        print(f"| {r['dist']} {r['length_range']} | {r['tokens_real']} | {r['padded_steps']} x {r['padded_rows_per_step']}"
              f" | {r['packed_steps']} x {r['packed_rows_per_step']} ({r['packed_seqs_per_step']:.1f}) | "
              f"{r['padded_seq_s']:.0f} ({pm[0]:.0f} .. {pm[1]:.0f}) | {r['packed_seq_s']:.0f} ({km[0]:.0f} .. {km[1]:.0f})"
              f" | {r['padded_ns_per_token']:.1f} | {r['packed_ns_per_token']:.1f} | {r['padded_step_ms']:.3f} | "
              f"{r['packed_step_ms']:.3f} | {r['speedup']:.2f}x |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
