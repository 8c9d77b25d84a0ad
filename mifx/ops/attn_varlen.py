"""Self-attention for training over packed variable-length sequences (csrc/attn_varlen_train.hip) as an autograd
function: forward with attention-probability dropout and saved softmax statistics, backward as a dq and a dk / dv
kernel.

The layout is the packed inference forward's (mifx.ops.bert_infer): qkv [rows, 3, H, 64] with `rows` the token capacity
of the buffers, cu_seqlens (sequence b owns rows cu[b] .. cu[b + 1] - 1, 1 .. 512 of them) and a block table of
(sequence, 128-row block) pairs (`block_table`, `cu_seqlens` of mifx.ops.bert_infer; entries of -1 are skipped). Rows
that belong to no listed sequence are inert: never read, their output rows and their dqkv rows are zero.

Dropout element (global head g = h0 + h, packed query row t = cu[b] + i, key j inside its sequence) takes the keep
bit of mifx.ops.fused_bert.keep_mask at the flat index

    (g * rows + t) * 512 + j

which depends neither on the head split nor on how the sequences of other packs of the same capacity are ordered.

On CUDA/HIP bf16 tensors with head dim 64 the native kernels run (required -- no silent fallback); on CPU tensors
`attention_varlen_reference` runs: the same math per sequence, differentiable by autograd."""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import _lib
from . import fused_bert as fb
from ._lib import F32, I32, VP, check, ptr, sig, stream_handle
from .bert_infer import HEAD_DIM, MAX_LEN, QBLOCK, block_table, cu_seqlens  # noqa: F401  (re-exported)

MASK_STRIDE = 512  # keys per query row in the dropout mask's flat index (the longest sequence)


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("attn_varlen_train")
    return {
        "fwd": sig(lib, "mifx_attn_fwd_varlen_train", [VP, VP, VP, I32, I32, I32, I32, I32, I32, F32, F32, VP, I32, VP,
                                                       VP, VP]),
        "bwd": sig(lib, "mifx_attn_bwd_varlen", [VP, VP, VP, I32, I32, I32, I32, I32, I32, F32, F32, VP, I32, VP, VP,
                                                 VP, VP, VP, VP]),
    }


def keep_at(index: np.ndarray, rng: torch.Tensor, site: int, p: float) -> np.ndarray:
    """fb.keep_mask at arbitrary flat indices (any shape, non-negative integers), without drawing the elements
    before them: keep_mask(n, ...)[index] for any n > index.max()."""
    seed, ctr = (int(v) for v in rng.detach().cpu().tolist()[:2])
    idx = np.asarray(index).astype(np.uint64)
    with np.errstate(over="ignore"):
        inner = fb._mix64(np.array([(ctr * fb._GOLDEN + site) & fb._M64], dtype=np.uint64))
        key = fb._mix64(np.array([seed & fb._M64], dtype=np.uint64) ^ inner)
        h = fb._mix64(key + (idx >> np.uint64(2)) * np.uint64(fb._GOLDEN))
    lane = (h >> ((idx & np.uint64(3)) * np.uint64(16))) & np.uint64(0xFFFF)
    return lane >= np.uint64(fb.drop_threshold(p))


def seq_keep_mask(rows: int, row0: int, L: int, heads, rng, site: int, p: float) -> torch.Tensor:
    """Bool keep[h, i, j] of one sequence (packed rows row0 .. row0 + L - 1 of a `rows`-row buffer) for the global
    heads `heads`: the documented index (g * rows + row0 + i) * 512 + j."""
    g = np.asarray(list(heads), dtype=np.uint64)[:, None, None]
    i = np.arange(L, dtype=np.uint64)[None, :, None]
    j = np.arange(L, dtype=np.uint64)[None, None, :]
    idx = (g * np.uint64(rows) + np.uint64(row0) + i) * np.uint64(MASK_STRIDE) + j
    return torch.from_numpy(keep_at(idx, rng, site, p))


def attention_varlen_reference(qkv: torch.Tensor, cu, nseq: int, scale: float, p: float = 0.0, rng=None, site: int = 0,
                               h0: int = 0, htot: int | None = None, dtype=None) -> torch.Tensor:
    """qkv [rows, 3, H, Dh] -> [rows, H, Dh]: softmax(q k^T scale), dropout, times v within each of the first `nseq`
    sequences of cu (a tensor or a list); rows of no sequence are zero. Computed in float32 (float64 for float64
    inputs, or in `dtype` when given) and returned in the input dtype (in `dtype` when given)."""
    rows, _, H, Dh = qkv.shape
    cul = [int(v) for v in (cu.tolist() if torch.is_tensor(cu) else cu)][:nseq + 1]
    cdt = dtype or (torch.float64 if qkv.dtype == torch.float64 else torch.float32)
    odt = dtype or qkv.dtype
    pieces, at = [], 0
    for b in range(len(cul) - 1):
        r0, r1 = cul[b], cul[b + 1]
        if r1 <= r0:
            continue
        if r0 < at or r1 > rows:
            raise ValueError(f"sequence {b}: rows {r0} .. {r1} overlap the previous sequence or leave the buffer")
        if r0 > at:
            pieces.append(torch.zeros(r0 - at, H, Dh, dtype=odt, device=qkv.device))
        x = qkv[r0:r1].to(cdt)
        s = torch.einsum("ihd,jhd->hij", x[:, 0], x[:, 1]) * scale
        pr = torch.softmax(s, -1)
        if p > 0:
            keep = seq_keep_mask(rows, r0, r1 - r0, range(h0, h0 + H), rng, site, p).to(pr.device)
            pr = torch.where(keep, pr * fb._drop_scale(p), torch.zeros((), dtype=pr.dtype, device=pr.device))
        pieces.append(torch.einsum("hij,jhd->ihd", pr, x[:, 2]).to(odt))
        at = r1
    if at < rows:
        pieces.append(torch.zeros(rows - at, H, Dh, dtype=odt, device=qkv.device))
    return torch.cat(pieces)


class _AttentionVarlen(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cu, table, nseq, lmax, scale, p, rng, site, h0):
        rows, _, H, Dh = qkv.shape
        qkv = qkv.contiguous()
        # rows of no sequence are never written: they are handed on as zeros (finite for the GEMM that reads them)
        out = torch.zeros(rows, H, Dh, device=qkv.device, dtype=torch.bfloat16)
        # softmax statistics per live query row, by packed row: [0] the row maximum, [1] log2 of the row sum
        stats = torch.empty(2, H, rows, device=qkv.device, dtype=torch.float32)
        check(_fns()["fwd"](ptr(qkv), ptr(cu), ptr(table), int(nseq), table.shape[0], rows, int(lmax), H, int(h0),
                            float(scale), float(p), ptr(rng if p > 0 else None), int(site), ptr(out), ptr(stats),
                            stream_handle(qkv.device)), "mifx_attn_fwd_varlen_train")
        ctx.save_for_backward(qkv, cu, table, out, stats)
        ctx.args = (int(nseq), int(lmax), float(scale), float(p), fb._snap(rng, p), int(site), int(h0))
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, cu, table, out, stats = ctx.saved_tensors
        nseq, lmax, scale, p, rng, site, h0 = ctx.args
        rows, _, H, Dh = qkv.shape
        dout = dout.to(torch.bfloat16).contiguous()
        # the kernels write the rows of the listed sequences, every element once; all other rows stay zero
        dqkv = torch.zeros_like(qkv)
        dsum = torch.empty(H, rows, device=qkv.device, dtype=torch.float32)
        check(_fns()["bwd"](ptr(qkv), ptr(cu), ptr(table), nseq, table.shape[0], rows, lmax, H, h0, scale, p,
                            ptr(rng if p > 0 else None), site, ptr(out), ptr(dout), ptr(stats), ptr(dqkv), ptr(dsum),
                            stream_handle(qkv.device)), "mifx_attn_bwd_varlen")
        return dqkv, None, None, None, None, None, None, None, None, None


def attention_varlen(qkv: torch.Tensor, cu, table, nseq: int, lmax: int, scale: float, p: float = 0.0, rng=None,
                     site: int = 0, h0: int = 0, htot: int | None = None) -> torch.Tensor:
    """Self-attention within each packed sequence: qkv [rows, 3, H, Dh] -> [rows, H, Dh], differentiable.

    cu: int32 [>= nseq + 1] cu_seqlens, table: int32 [n, 2] of (sequence, 128-row block) pairs (block_table(); -1
    entries are skipped), both on qkv's device; lmax: an upper bound of the longest sequence (<= 512; a longer one in
    the table is skipped). p > 0 needs rng = int64 [seed, counter]; mask element (h0 + h, cu[b] + i, j) is
    fb.keep_mask at ((h0 + h) * rows + cu[b] + i) * 512 + j. htot (the model's head count) is accepted for symmetry
    with fb.attention; the index does not need it. Rows of no listed sequence give zero output and zero gradient."""
    if qkv.dim() != 4 or qkv.shape[1] != 3:
        raise ValueError(f"qkv must be [rows, 3, H, Dh], got {tuple(qkv.shape)}")
    if p > 0 and rng is None:
        raise ValueError("attention dropout p > 0 needs an rng state tensor [seed, counter]")
    if not 0 <= p < 1:
        raise ValueError(f"dropout probability {p} outside [0, 1)")
    if not 1 <= lmax <= MAX_LEN:
        raise ValueError(f"longest sequence {lmax} outside 1 .. {MAX_LEN}")
    rows, _, H, Dh = qkv.shape
    if htot is not None and not 0 <= h0 <= htot - H:
        raise ValueError(f"heads {h0} .. {h0 + H - 1} outside the model's {htot}")
    if not qkv.is_cuda:
        return attention_varlen_reference(qkv, cu, nseq, scale, p, rng, site, h0, htot)
    if Dh != HEAD_DIM or qkv.dtype != torch.bfloat16:
        raise ValueError(f"the packed attention kernels take bf16 heads of {HEAD_DIM}, got {qkv.dtype} x {Dh}")
    for t in (cu, table):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.device != qkv.device or not t.is_contiguous():
            raise ValueError("cu and table must be contiguous int32 tensors on qkv's device")
    if cu.numel() < nseq + 1 or nseq < 1 or table.dim() != 2 or table.shape[1] != 2 or table.shape[0] < 1:
        raise ValueError("cu / table do not match nseq")
    from . import native_stats

    native_stats.count("attention_varlen", True)
    return _AttentionVarlen.apply(qkv, cu, table, nseq, lmax, scale, p, rng, site, h0)
