"""Packed variable-length BERT inference kernels (csrc/bert_infer.hip): forward-only attention per sequence from a
cu_seqlens table, and the embedding sum + LayerNorm with explicit position ids.

On CUDA/HIP tensors the native kernels run (required -- no silent fallback); on CPU tensors the PyTorch reference of
the same math runs."""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import F32, I32, VP, check, ptr, sig, stream_handle

QBLOCK = 128  # queries per workgroup of the attention kernel
MAX_LEN = 512  # longest sequence the attention kernel takes
HEAD_DIM = 64


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("bert_infer")
    return {
        "attn": sig(lib, "mifx_attn_fwd_varlen", [VP, VP, VP, I32, I32, I32, I32, I32, F32, VP, VP]),
        "embed": sig(lib, "mifx_bert_embed_ln_packed", [VP, VP, VP, VP, VP, VP, VP, VP, I32, I32, I32, I32, I32, F32,
                                                        VP, VP]),
    }


def block_table(lengths) -> list:
    """The attention kernel's work list: one (sequence, 128-query block) pair per workgroup and head, in pack order."""
    return [(b, q) for b, L in enumerate(lengths) for q in range((int(L) + QBLOCK - 1) // QBLOCK)]


def cu_seqlens(lengths) -> list:
    cu = [0]
    for L in lengths:
        cu.append(cu[-1] + int(L))
    return cu


def attn_varlen_reference(qkv: torch.Tensor, cu, scale: float) -> torch.Tensor:
    """qkv [T, 3, H, Dh] -> [T, H, Dh]: softmax(q k^T scale) v within each sequence cu[b] .. cu[b + 1] - 1."""
    out = torch.zeros(qkv.shape[0], qkv.shape[2], qkv.shape[3], dtype=qkv.dtype, device=qkv.device)
    for b in range(len(cu) - 1):
        x = qkv[int(cu[b]):int(cu[b + 1])].float()
        s = torch.einsum("ihd,jhd->hij", x[:, 0], x[:, 1]) * scale
        out[int(cu[b]):int(cu[b + 1])] = torch.einsum("hij,jhd->ihd", torch.softmax(s, -1), x[:, 2]).to(qkv.dtype)
    return out


def attn_fwd_varlen(qkv: torch.Tensor, cu: torch.Tensor, table: torch.Tensor, nseq: int, lmax: int, scale: float,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """Self-attention over packed sequences. qkv bf16 [T, 3, H, 64] (the fused projection output), cu int32
    [>= nseq + 1] and table int32 [n, 2] on qkv's device (block_table(); entries of -1 are skipped), lmax an upper
    bound of the longest sequence (<= 512). Returns bf16 [T, H, 64]; rows of no sequence keep what `out` held."""
    T, three, H, Dh = qkv.shape
    if three != 3 or Dh != HEAD_DIM or qkv.dtype != torch.bfloat16 or not qkv.is_contiguous():
        raise ValueError(f"qkv must be contiguous bf16 [T, 3, H, {HEAD_DIM}], got {tuple(qkv.shape)} {qkv.dtype}")
    if not 1 <= lmax <= MAX_LEN:
        raise ValueError(f"longest sequence {lmax} outside 1 .. {MAX_LEN}")
    if out is None:
        out = torch.zeros(T, H, Dh, dtype=qkv.dtype, device=qkv.device)
    if not qkv.is_cuda:
        cul = cu[:nseq + 1].tolist()
        out[:cul[-1]] = attn_varlen_reference(qkv[:cul[-1]], cul, scale)
        return out
    for t in (cu, table):
        if t.dtype != torch.int32 or t.device != qkv.device or not t.is_contiguous():
            raise ValueError("cu and table must be contiguous int32 tensors on qkv's device")
    if cu.numel() < nseq + 1 or table.dim() != 2 or table.shape[1] != 2 or out.shape != (T, H, Dh) \
            or out.dtype != qkv.dtype or not out.is_contiguous():
        raise ValueError("cu / table / out do not match qkv")
    check(_fns()["attn"](ptr(qkv), ptr(cu), ptr(table), int(nseq), table.shape[0], T, int(lmax), H, float(scale),
                         ptr(out), stream_handle(qkv.device)), "mifx_attn_fwd_varlen")
    return out


def embed_ln_reference(ids, tts, pos_ids, word, pos, type_, gamma, beta, eps: float) -> torch.Tensor:
    """LayerNorm(word[ids] + pos[pos_ids] + type[tts]) in fp32, rounded once to word's dtype; rows with ids < 0 zero."""
    live = ids >= 0
    i = ids.clamp(min=0).long()
    s = word.float()[i] + pos.float()[pos_ids.clamp(min=0).long()] + type_.float()[tts.clamp(min=0).long()]
    y = F.layer_norm(s, (word.shape[1],), gamma.float(), beta.float(), eps)
    return torch.where(live[:, None], y, torch.zeros(())).to(word.dtype)


def embed_ln_packed(ids: torch.Tensor, tts: torch.Tensor, pos_ids: torch.Tensor, word: torch.Tensor,
                    pos: torch.Tensor, type_: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """x[t] = LayerNorm(word[ids[t]] + pos[pos_ids[t]] + type[tts[t]]) -> bf16 [T, hidden]; ids / tts / pos_ids int32
    [T], tables bf16. A token with ids[t] < 0 is written as a zero row."""
    T, Hd = ids.numel(), word.shape[1]
    if not ids.is_cuda:
        y = embed_ln_reference(ids, tts, pos_ids, word, pos, type_, gamma, beta, eps)
        if out is None:
            return y
        out.copy_(y)
        return out
    for t in (ids, tts, pos_ids):
        if t.dtype != torch.int32 or t.numel() != T or not t.is_contiguous() or t.device != word.device:
            raise ValueError("ids, tts and pos_ids must be contiguous int32 [T] on the tables' device")
    for t in (word, pos, type_, gamma, beta):
        if t.dtype != torch.bfloat16 or not t.is_contiguous() or t.shape[-1] != Hd:
            raise ValueError("embedding tables and LayerNorm parameters must be contiguous bf16 of one width")
    if out is None:
        out = torch.empty(T, Hd, dtype=torch.bfloat16, device=word.device)
    elif out.shape != (T, Hd) or out.dtype != torch.bfloat16 or not out.is_contiguous():
        raise ValueError("out must be contiguous bf16 [T, hidden]")
    check(_fns()["embed"](ptr(ids), ptr(tts), ptr(pos_ids), ptr(word), ptr(pos), ptr(type_), ptr(gamma), ptr(beta), T,
                          Hd, word.shape[0], pos.shape[0], type_.shape[0], float(eps), ptr(out),
                          stream_handle(word.device)), "mifx_bert_embed_ln_packed")
    return out
