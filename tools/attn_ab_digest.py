"""sha256 digests of everything the chunked attention kernels write, on seeded inputs: one JSON line per case.

For A/B runs of two builds of csrc/attention.hip, csrc/attn_varlen_train.hip and csrc/bert_infer.hip that must agree to
the bit (select the other build with MIFX_LIB_ATTENTION, MIFX_LIB_ATTN_VARLEN_TRAIN and MIFX_LIB_BERT_INFER): the two
outputs are compared with cmp. The kernels are called through the entry points that mifx.ops.fused_bert,
mifx.ops.attn_varlen and mifx.ops.bert_infer bind, with this script's own buffers, because the statistics and the dsum
workspace never leave the autograd functions. Buffers a kernel may leave rows of untouched start as zeros.

Usage: python tools/attn_ab_digest.py [--out FILE]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mifx.ops import attn_varlen as av  # noqa: E402
from mifx.ops import bert_infer as bi  # noqa: E402
from mifx.ops import fused_bert as fb  # noqa: E402
from mifx.ops._lib import check, ptr, stream_handle  # noqa: E402

DENSE = [(2, 2, 192), (2, 3, 320), (1, 2, 512)]  # B, H, S
LENGTHS = [17, 64, 65, 128, 129, 130, 192, 257, 512, 1]
HEADS = 2  # packed cases
SITE = 3
SCALE = 0.125


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float32).to(torch.bfloat16).cuda()


def dense_case(B, H, S, biased, p):
    gen = torch.Generator().manual_seed(1000 * S + 10 * H + B)
    qkv, dout = randn(gen, B, S, 3, H, 64), randn(gen, B, S, H, 64)
    kb = None
    if biased:  # the last 9 keys of every sequence are padding
        kb = torch.zeros(B, S, dtype=torch.float32)
        kb[:, S - 9:] = -1e30
        kb = kb.cuda()
    rng = torch.tensor([1234, 7], dtype=torch.int64).cuda() if p > 0 else None
    h0, htot, st = 1, H + 2, stream_handle(qkv.device)
    out = torch.empty(B, S, H, 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(2, B, H, S, dtype=torch.float32, device="cuda")
    dqkv = torch.empty_like(qkv)
    dsum = torch.empty(B, H, S, dtype=torch.float32, device="cuda")
    f = fb._attn_fns()
    check(f["fwd"](ptr(qkv), ptr(kb), B, S, H, h0, htot, SCALE, p, ptr(rng), SITE, ptr(out), ptr(lse), st), "fwd")
    check(f["bwd"](ptr(qkv), ptr(kb), ptr(out), ptr(dout), ptr(lse), B, S, H, h0, htot, SCALE, p, ptr(rng), SITE,
                   ptr(dqkv), ptr(dsum), st), "bwd")
    torch.cuda.synchronize()
    return {"case": "dense", "B": B, "H": H, "S": S, "bias": biased, "p": p, "out": sha(out), "lse": sha(lse),
            "dqkv": sha(dqkv), "dsum": sha(dsum)}


def packed_inputs():
    rows = sum(LENGTHS)  # a buffer of exactly T rows: the row after the last sequence is past the allocation
    gen = torch.Generator().manual_seed(4242)
    qkv, dout = randn(gen, rows, 3, HEADS, 64), randn(gen, rows, HEADS, 64)
    cu = torch.tensor(bi.cu_seqlens(LENGTHS), dtype=torch.int32).cuda()
    return rows, qkv, dout, cu


def packed_train_case(p, edges):
    rows, qkv, dout, cu = packed_inputs()
    table, lmax = bi.block_table(LENGTHS), max(LENGTHS)
    if edges:  # a padding entry in the middle of the table, and lmax below the 512-token sequence (skipped)
        table, lmax = table[:5] + [(-1, -1)] + table[5:], 257
    table = torch.tensor(table, dtype=torch.int32).cuda()
    rng = torch.tensor([99, 5], dtype=torch.int64).cuda() if p > 0 else None
    nseq, nent, h0, st = len(LENGTHS), table.shape[0], 1, stream_handle(qkv.device)
    out = torch.zeros(rows, HEADS, 64, dtype=torch.bfloat16, device="cuda")
    stats = torch.zeros(2, HEADS, rows, dtype=torch.float32, device="cuda")
    dqkv = torch.zeros_like(qkv)
    dsum = torch.zeros(HEADS, rows, dtype=torch.float32, device="cuda")
    f = av._fns()
    check(f["fwd"](ptr(qkv), ptr(cu), ptr(table), nseq, nent, rows, lmax, HEADS, h0, SCALE, p, ptr(rng), SITE,
                   ptr(out), ptr(stats), st), "fwd")
    check(f["bwd"](ptr(qkv), ptr(cu), ptr(table), nseq, nent, rows, lmax, HEADS, h0, SCALE, p, ptr(rng), SITE,
                   ptr(out), ptr(dout), ptr(stats), ptr(dqkv), ptr(dsum), st), "bwd")
    torch.cuda.synchronize()
    return {"case": "packed_train", "p": p, "padding_and_lmax": edges, "out": sha(out), "stats": sha(stats),
            "dqkv": sha(dqkv), "dsum": sha(dsum)}


def packed_infer_case():
    rows, qkv, _, cu = packed_inputs()
    table = torch.tensor(bi.block_table(LENGTHS), dtype=torch.int32).cuda()
    out = bi.attn_fwd_varlen(qkv, cu, table, len(LENGTHS), max(LENGTHS), SCALE)
    torch.cuda.synchronize()
    return {"case": "packed_infer", "out": sha(out)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_ab_digest needs a GPU")
    lines = []
    for B, H, S in DENSE:
        for biased in (False, True):
            for p in (0.0, 0.1):
                lines.append(dense_case(B, H, S, biased, p))
    for p in (0.0, 0.1):
        for edges in (False, True):
            lines.append(packed_train_case(p, edges))
    lines.append(packed_infer_case())
    text = "".join(json.dumps(ln) + "\n" for ln in lines)
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
