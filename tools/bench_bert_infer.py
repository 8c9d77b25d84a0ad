"""Packed variable-length BERT inference against the padded forward (mifx/models/bert_infer.py), BERT-base.

For every (batch, length distribution) cell: sequences/s and tokens/s of `BertInference.graphed()` with the packed
forward (the default on the GPU) and with MIFX_BERT_INFER_PACKED=0 (the training model's eval forward, padded to the
batch's longest sequence rounded up to 64, attention mask), both replayed from hipGraphs and alternated in the same
process. A call is timed on the host around a device synchronise and includes the host's packing / padding and the
H2D copy: that is what a served request pays. Tokens/s counts REAL tokens for both paths; the token counts each path
computes on (packed: the sum of the lengths, and the capacity bucket its kernels are launched for; padded: batch x
padded length) are printed beside the times.

Usage: python tools/bench_bert_infer.py [--batches 1 8 32 128] [--rounds 3] [--window 0.25] [--out FILE.jsonl]
       python tools/bench_bert_infer.py --one-forward 32 uniform     (one packed forward: for a profiler run)"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mifx.models import bert_infer as M  # noqa: E402
from mifx.models.bert import BertConfig, full_init_state  # noqa: E402

DISTS = ("uniform", "short_heavy", "all128")


def lengths_of(dist: str, batch: int, seed: int) -> list:
    """uniform: [64, 128] (the synthetic ExampleGen's at seq_len 128). short_heavy: below 32 except one sequence in
    16 (at least one from batch 8 on) at 512. all128: no padding to remove."""
    g = np.random.default_rng(seed)
    if dist == "uniform":
        return [int(x) for x in g.integers(64, 129, size=batch)]
    if dist == "all128":
        return [128] * batch
    out = [int(x) for x in g.integers(4, 32, size=batch)]
    for i in range(max(1, batch // 16) if batch >= 8 else 0):
        out[int(g.integers(0, batch))] = 512
    return out


def make_seqs(lengths, vocab: int, seed: int) -> list:
    g = np.random.default_rng(seed + 1)
    return [g.integers(1000, vocab, size=L).astype(np.int32) for L in lengths]


def build(cfg, state, packed: bool, max_tokens: int, max_seqs: int):
    old = os.environ.get("MIFX_BERT_INFER_PACKED")
    os.environ["MIFX_BERT_INFER_PACKED"] = "1" if packed else "0"
    try:
        inf = M.BertInference(state, cfg, "cuda", max_tokens=max_tokens, max_seqs=max_seqs)
    finally:
        if old is None:
            del os.environ["MIFX_BERT_INFER_PACKED"]
        else:
            os.environ["MIFX_BERT_INFER_PACKED"] = old
    assert inf.packed == packed
    return inf


def timed(run, seqs, window: float) -> float:
    """Seconds per call over at least `window` seconds of calls, each ending in a device synchronise."""
    n, t0 = 0, time.perf_counter()
    while True:
        run(seqs)
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= window and n >= 3:
            return dt / n


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 32, 128])
    ap.add_argument("--dists", nargs="*", default=list(DISTS), choices=DISTS)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-forward", nargs=2, metavar=("BATCH", "DIST"), default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_bert_infer needs a GPU (no CPU timing is meaningful)")
    torch.manual_seed(a.seed)
    cfg = BertConfig()
    state = full_init_state(cfg, a.seed)
    max_seqs = max(a.batches + [int(a.one_forward[0])] if a.one_forward else a.batches)
    max_tokens = 16384
    packed = build(cfg, state, True, max_tokens, max_seqs)
    if a.one_forward:  # warm-up, then exactly one eager packed forward between two synchronises
        lens = lengths_of(a.one_forward[1], int(a.one_forward[0]), a.seed)
        seqs = make_seqs(lens, cfg.vocab_size, a.seed)
        packed.logits(seqs)
        torch.cuda.synchronize()
        packed.logits(seqs)
        torch.cuda.synchronize()
        print(json.dumps({"one_forward": a.one_forward, "tokens": sum(lens)}))
        return 0
    padded = build(cfg, state, False, max_tokens, max_seqs)
    runs = {"packed": packed.graphed(), "padded": padded.graphed()}
    rows = []
    for dist in a.dists:
        for B in a.batches:
            lens = lengths_of(dist, B, a.seed + 17 * B)
            seqs = make_seqs(lens, cfg.vocab_size, a.seed)
            T = sum(lens)
            cap = M.capacity_bucket(T, max_tokens)
            S = M.length_class(max(lens))
            outs = {k: r(seqs).float().cpu() for k, r in runs.items()}  # warm-up: captures both graphs
            torch.cuda.synchronize()
            diff = float((outs["packed"] - outs["padded"]).abs().max())
            t = {k: [] for k in runs}
            for _ in range(a.rounds):  # alternate the two paths
                for k, r in runs.items():
                    t[k].append(timed(r, seqs, a.window))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = {"dist": dist, "batch": B, "tokens_real": T, "tokens_packed_capacity": cap,
                   "tokens_padded": B * S, "padded_len": S, "packed_ms": med["packed"] * 1e3,
                   "padded_ms": med["padded"] * 1e3, "packed_ms_all": [x * 1e3 for x in t["packed"]],
                   "padded_ms_all": [x * 1e3 for x in t["padded"]],
                   "packed_seq_s": B / med["packed"], "padded_seq_s": B / med["padded"],
                   "packed_tok_s": T / med["packed"], "padded_tok_s": T / med["padded"],
                   "speedup": med["padded"] / med["packed"], "max_abs_logit_diff": diff}
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("\n| lengths | batch | real tokens | packed rows (bucket) | padded rows | packed ms | padded ms | "
          "packed seq/s | padded seq/s | packed tok/s | padded tok/s | packed / padded |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['dist']} | {r['batch']} | {r['tokens_real']} | {r['tokens_real']} ({r['tokens_packed_capacity']}) "
              f"| {r['tokens_padded']} | {r['packed_ms']:.3f} | {r['padded_ms']:.3f} | {r['packed_seq_s']:.0f} | "
              f"{r['padded_seq_s']:.0f} | {r['packed_tok_s']:.0f} | {r['padded_tok_s']:.0f} | {r['speedup']:.2f}x |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
