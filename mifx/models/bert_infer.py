"""Inference form of the fine-tuned BERT classifier (BASELINE config 4): a forward over PACKED variable-length
sequences.

Requests arrive with their own lengths. The training forward pads every sequence of a batch to one S, so each
projection GEMM, LayerNorm and GELU runs on B x S rows. Here the activations are [T, hidden] with T = sum of the
lengths and no padding rows; attention runs per sequence from a cu_seqlens table (csrc/bert_infer.hip
`mifx_attn_fwd_varlen`, sequences of 1 .. 512 tokens of any length), the embedding sum + LayerNorm takes explicit
position ids that restart in every sequence (`mifx_bert_embed_ln_packed`), and every other op is the training
forward's token-wise kernel at p = 0 (mifx.ops.fused_bert) on T rows.

The host packs a request into one pinned int32 staging buffer (ids, token types, position ids, cu_seqlens, first-token
rows, block table) copied in one H2D copy. The forward runs on static buffers of a token-capacity bucket (a small
ladder of multiples of 256), so `graphed()` captures one hipGraph per (capacity, longest-length class): grids are
sized for the capacity, unused block-table entries are -1 and exit at once, unused token rows have id -1 and are
written as zeros; all of them are rewritten on every call.

Off the GPU, or with MIFX_BERT_INFER_PACKED=0 (kept for A/B), the same weights run through
`BertForSequenceClassification` in eval mode, padded to the batch's longest sequence with the attention mask; that is
what the CPU tests check against."""
from __future__ import annotations

import json
import os
import threading
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

from ..ops import bert_infer as bi
from ..ops import fused_bert as fb
from .bert import BertConfig, BertForSequenceClassification

# token-capacity buckets below max_tokens, multiples of 256 in steps of 256 / 512 / 1024 / 2048: the rows the token-wise
# kernels and GEMMs run on exceed the real tokens by less than 256 up to 2048 tokens and by an eighth beyond
LADDER = tuple(range(256, 2048, 256)) + tuple(range(2048, 4096, 512)) + tuple(range(4096, 8192, 1024)) \
    + tuple(range(8192, 16384 + 1, 2048))
_CFG_KEYS = ("vocab_size", "hidden", "layers", "heads", "intermediate", "max_position", "type_vocab", "num_labels",
             "ln_eps")


def max_length(cfg: BertConfig) -> int:
    return min(cfg.max_position, bi.MAX_LEN)


def validate(seqs, token_types, cfg: BertConfig) -> None:
    """ValueError naming the offending sequence: empty, too long, an id outside the vocabulary, a token type outside
    type_vocab (or a token-type list of another length)."""
    if token_types is not None and len(token_types) != len(seqs):
        raise ValueError(f"{len(token_types)} token-type lists for {len(seqs)} sequences")
    top = max_length(cfg)
    for i, s in enumerate(seqs):
        a = np.asarray(s)
        if a.ndim != 1 or a.size == 0:
            raise ValueError(f"sequence {i}: empty (or not a flat list of token ids)")
        if a.size > top:
            raise ValueError(f"sequence {i}: length {a.size} above the maximum {top}")
        if a.dtype.kind not in "iu":
            raise ValueError(f"sequence {i}: token ids must be integers")
        if int(a.min()) < 0 or int(a.max()) >= cfg.vocab_size:
            raise ValueError(f"sequence {i}: token id outside the vocabulary [0, {cfg.vocab_size})")
        if token_types is not None and token_types[i] is not None:
            t = np.asarray(token_types[i])
            if t.shape != a.shape:
                raise ValueError(f"sequence {i}: {t.size} token types for {a.size} tokens")
            if t.dtype.kind not in "iub" or int(t.min()) < 0 or int(t.max()) >= cfg.type_vocab:
                raise ValueError(f"sequence {i}: token type outside [0, {cfg.type_vocab})")


def capacity_ladder(max_tokens: int) -> tuple:
    if max_tokens < 512 or max_tokens % 256:
        raise ValueError(f"max_tokens must be a multiple of 256 and at least 512, got {max_tokens}")
    return tuple(c for c in LADDER if c < max_tokens) + (max_tokens,)


def capacity_bucket(tokens: int, max_tokens: int) -> int:
    """The smallest rung of the ladder that holds `tokens`."""
    for c in capacity_ladder(max_tokens):
        if tokens <= c:
            return c
    raise ValueError(f"{tokens} tokens above the capacity {max_tokens}")


def plan_packs(lengths, max_tokens: int, max_seqs: int) -> list:
    """Cut a request into consecutive packs [(start, end), ...] of at most max_tokens tokens and max_seqs sequences,
    order preserved (greedy: a pack is closed when the next sequence does not fit)."""
    packs, start, tok = [], 0, 0
    for i, L in enumerate(lengths):
        if L > max_tokens:
            raise ValueError(f"sequence {i}: length {L} above the token capacity {max_tokens}")
        if i > start and (tok + L > max_tokens or i - start >= max_seqs):
            packs.append((start, i))
            start, tok = i, 0
        tok += L
    if len(lengths) > start:
        packs.append((start, len(lengths)))
    return packs


def table_entries(capacity: int, max_seqs: int) -> int:
    """Block-table rows of a capacity: sum ceil(L_i / 128) <= T / 128 + B."""
    return capacity // bi.QBLOCK + max_seqs


def staging_size(capacity: int, max_seqs: int) -> int:
    return 3 * capacity + (max_seqs + 1) + max_seqs + 2 * table_entries(capacity, max_seqs)


@dataclass
class Pack:
    """Views into one int32 staging buffer (`buf`), in this order: ids, token types, position ids [capacity] (ids -1
    beyond the T live tokens), cu_seqlens [max_seqs + 1] (T beyond the B live sequences), first-token rows [max_seqs]
    (0 beyond B), block table [entries, 2] (-1 beyond the live blocks)."""
    buf: object
    ids: object
    tts: object
    pos: object
    cu: object
    first: object
    table: object
    tokens: int = 0
    seqs: int = 0
    capacity: int = 0
    longest: int = 0
    blocks: int = 0


def staging_views(buf, capacity: int, max_seqs: int) -> Pack:
    """`buf`: a flat int32 numpy array or torch tensor of staging_size() elements."""
    o, C, ne = 0, capacity, table_entries(capacity, max_seqs)
    parts = []
    for n in (C, C, C, max_seqs + 1, max_seqs, 2 * ne):
        parts.append(buf[o:o + n])
        o += n
    return Pack(buf, parts[0], parts[1], parts[2], parts[3], parts[4], parts[5].reshape(ne, 2), capacity=capacity)


def pack(seqs, token_types, capacity: int, max_seqs: int, out=None) -> Pack:
    """Pack validated sequences into a staging buffer (a new numpy one, or `out`: a flat int32 numpy array of
    staging_size(capacity, max_seqs) elements, every element of which is rewritten)."""
    lengths = [len(s) for s in seqs]
    T, B = sum(lengths), len(seqs)
    if T > capacity or B > max_seqs:
        raise ValueError(f"{B} sequences / {T} tokens above the capacity {max_seqs} / {capacity}")
    buf = np.empty(staging_size(capacity, max_seqs), np.int32) if out is None else out
    p = staging_views(buf, capacity, max_seqs)
    p.ids[T:] = -1
    p.tts[T:] = 0
    p.pos[T:] = 0
    cu = bi.cu_seqlens(lengths)
    for b, s in enumerate(seqs):
        p.ids[cu[b]:cu[b + 1]] = s
        p.tts[cu[b]:cu[b + 1]] = 0 if token_types is None or token_types[b] is None else token_types[b]
        p.pos[cu[b]:cu[b + 1]] = np.arange(lengths[b], dtype=np.int32)
    p.cu[:B + 1] = cu
    p.cu[B + 1:] = T
    p.first[:B] = cu[:-1]
    p.first[B:] = 0
    tab = bi.block_table(lengths)
    p.table[:] = -1
    if tab:
        p.table[:len(tab)] = tab
    p.tokens, p.seqs, p.longest, p.blocks = T, B, max(lengths), len(tab)
    return p


def length_class(longest: int) -> int:
    """The attention kernel's LDS follows the longest sequence rounded up to 64: one captured graph per class."""
    return (longest + 63) // 64 * 64


def _pad_arrays(seqs, token_types, S: int):
    """ids, token types [B, S] int64 and the attention mask [B, S] fp32 of the padded forward."""
    B = len(seqs)
    ids = np.zeros((B, S), np.int64)
    tt = np.zeros((B, S), np.int64)
    am = np.zeros((B, S), np.float32)
    for b, s in enumerate(seqs):
        ids[b, :len(s)] = s
        am[b, :len(s)] = 1
        if token_types is not None and token_types[b] is not None:
            tt[b, :len(s)] = token_types[b]
    return ids, tt, am


def load_state(path: str):
    """(TP=1 state dict, BertConfig or None) of a `bert_seq_cls` saved-model export or a BertTrainer export dir."""
    from safetensors.torch import load_file

    sm = os.path.join(path, "saved_model.json")
    if os.path.exists(sm):
        with open(sm) as f:
            mc = json.load(f)["model_config"]
        sd = load_file(os.path.join(path, "variables", "variables.safetensors"))
    else:
        with open(os.path.join(path, "config.json")) as f:
            mc = json.load(f)
        sd = load_file(os.path.join(path, "variables.safetensors"))
    return sd, BertConfig(**{k: mc[k] for k in _CFG_KEYS if k in mc})


class BertInference:
    """`logits(seqs, token_types=None)`: a list of token-id lists -> [B, num_labels] fp32 on `device`."""

    def __init__(self, state_or_export_dir, cfg: BertConfig | None = None, device=None, max_tokens: int = 4096,
                 max_seqs: int = 128):
        if isinstance(state_or_export_dir, (str, os.PathLike)):
            state, dcfg = load_state(os.fspath(state_or_export_dir))
            cfg = cfg or dcfg
        else:
            state = state_or_export_dir
        if cfg is None:
            raise ValueError("a state dict needs its BertConfig")
        self.cfg = cfg
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        self.ladder = capacity_ladder(max_tokens)
        if max_seqs < 1:
            raise ValueError(f"max_seqs must be positive, got {max_seqs}")
        self.max_tokens, self.max_seqs = max_tokens, max_seqs
        self.packed = self.device.type == "cuda" and os.environ.get("MIFX_BERT_INFER_PACKED", "1") != "0"
        self._lock = threading.Lock()
        self._bufs: dict = {}
        self._graphs: dict = {}
        self._pool = None  # one memory pool for every captured graph: they replay one at a time, outputs are cloned
        self.model = None
        if self.packed:
            if cfg.hidden != cfg.heads * bi.HEAD_DIM:
                raise ValueError(f"the packed forward needs heads of {bi.HEAD_DIM}, got {cfg.hidden} / {cfg.heads}")
            self.w = {k: v.detach().to(self.device, torch.bfloat16).contiguous() for k, v in state.items()}
        else:
            m = BertForSequenceClassification(cfg, None, seed=None)
            m.load_full({k: v.detach().float() for k, v in state.items()})
            m = m.to(self.device)
            self.model = (m.bfloat16() if self.device.type == "cuda" else m).eval()

    # ------------------------------------------------------------------ padded (off the GPU, or for A/B)
    def _padded(self, seqs, token_types) -> torch.Tensor:
        B, S = len(seqs), max(len(s) for s in seqs)
        if self.device.type == "cuda":  # the fused attention of the training forward takes S % 64 == 0
            S = length_class(S)
        ids, tt, am = _pad_arrays(seqs, token_types, S)
        with torch.no_grad():
            return self.model(*(torch.from_numpy(a).to(self.device) for a in (ids, tt, am))).float()

    # ------------------------------------------------------------------ packed
    def _buffers(self, capacity: int) -> dict:
        b = self._bufs.get(capacity)
        if b is None:
            n, c = staging_size(capacity, self.max_seqs), self.cfg
            host = torch.empty(n, dtype=torch.int32, pin_memory=True)
            dev = torch.empty(n, dtype=torch.int32, device=self.device)
            b = {"host": host, "np": host.numpy(), "dev": dev, "views": staging_views(dev, capacity, self.max_seqs),
                 # attention output: rows of no sequence are never written, so they start (and stay) finite
                 "ctx": torch.zeros(capacity, c.heads, bi.HEAD_DIM, dtype=torch.bfloat16, device=self.device),
                 "copied": torch.cuda.Event()}
            self._bufs[capacity] = b
        return b

    def _stage(self, seqs, token_types):
        """Pack on the host and copy to the capacity bucket's static device buffer: one H2D copy."""
        cap = capacity_bucket(sum(len(s) for s in seqs), self.max_tokens)
        b = self._buffers(cap)
        b["copied"].synchronize()  # the previous copy out of the pinned buffer is done
        p = pack(seqs, token_types, cap, self.max_seqs, out=b["np"])
        b["dev"].copy_(b["host"], non_blocking=True)
        b["copied"].record(torch.cuda.current_stream(self.device))
        return b, p

    def _forward(self, b: dict, lclass: int) -> torch.Tensor:
        """The packed forward on the bucket's static buffers -> fp32 logits [max_seqs, num_labels]."""
        c, w, v = self.cfg, self.w, b["views"]
        C = v.capacity
        x = bi.embed_ln_packed(v.ids, v.tts, v.pos, w["word.weight"], w["pos.weight"], w["tok_type.weight"],
                               w["ln_emb.weight"], w["ln_emb.bias"], c.ln_eps)
        ctx = b["ctx"]
        for i in range(c.layers):
            p = f"layers.{i}."
            qkv = F.linear(x, w[p + "qkv.weight"], w[p + "qkv.bias"]).view(C, 3, c.heads, bi.HEAD_DIM)
            bi.attn_fwd_varlen(qkv, v.cu, v.table, self.max_seqs, lclass, bi.HEAD_DIM ** -0.5, out=ctx)
            a = F.linear(ctx.view(C, c.hidden), w[p + "attn_out.weight"])
            x = fb.bias_dropout_add_layernorm(a, w[p + "attn_out.bias"], x, w[p + "ln1.weight"], w[p + "ln1.bias"],
                                              c.ln_eps)
            f = fb.bias_gelu(F.linear(x, w[p + "ffn_in.weight"]), w[p + "ffn_in.bias"])
            o = F.linear(f, w[p + "ffn_out.weight"])
            x = fb.bias_dropout_add_layernorm(o, w[p + "ffn_out.bias"], x, w[p + "ln2.weight"], w[p + "ln2.bias"],
                                              c.ln_eps)
        pooled = torch.tanh(F.linear(x.index_select(0, v.first), w["pooler.weight"], w["pooler.bias"]))
        return F.linear(pooled, w["classifier.weight"], w["classifier.bias"]).float()

    def _packed(self, seqs, token_types, graphs: bool) -> torch.Tensor:
        b, p = self._stage(seqs, token_types)
        lclass = length_class(p.longest)
        with torch.no_grad():
            if not graphs:
                return self._forward(b, lclass)[:p.seqs].clone()
            key = (p.capacity, lclass)
            g = self._graphs.get(key)
            if g is None:
                g = self._graphs[key] = self._capture(b, lclass)
            g[0].replay()
            return g[1][:p.seqs].clone()

    def _capture(self, b: dict, lclass: int):
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):  # warm-up (library handles, GEMM solution choice) outside the capture
            self._forward(b, lclass)
        torch.cuda.current_stream(self.device).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        if self._pool is None:
            self._pool = torch.cuda.graph_pool_handle()
        with torch.cuda.graph(graph, pool=self._pool):
            out = self._forward(b, lclass)
        return graph, out

    # ------------------------------------------------------------------ public
    def _run(self, seqs, token_types, graphs: bool) -> torch.Tensor:
        seqs = [np.asarray(s) for s in seqs]
        validate(seqs, token_types, self.cfg)
        if not seqs:
            return torch.zeros(0, self.cfg.num_labels, device=self.device)
        outs = []
        with self._lock:
            for s0, s1 in plan_packs([len(s) for s in seqs], self.max_tokens, self.max_seqs):
                tt = None if token_types is None else token_types[s0:s1]
                if self.packed:
                    outs.append(self._packed(seqs[s0:s1], tt, graphs))
                elif graphs:
                    outs.append(self._padded_graphed(seqs[s0:s1], tt))
                else:
                    outs.append(self._padded(seqs[s0:s1], tt))
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def logits(self, seqs, token_types=None) -> torch.Tensor:
        """seqs: a list of token-id lists (1 .. min(max_position, 512) ids each); token_types: None or a list of
        per-sequence lists (None entries: zeros). A request above the capacity runs as several packs, in order."""
        return self._run(seqs, token_types, False)

    def graphed(self):
        """f(seqs, token_types=None) -> logits, the forward replayed from one hipGraph per (token capacity,
        longest-length class), captured on first use (the padded A/B path: per (batch, padded length))."""
        if self.device.type != "cuda":
            raise RuntimeError("graphed() needs a GPU")

        def run(seqs, token_types=None) -> torch.Tensor:
            return self._run(seqs, token_types, True)

        return run

    def _padded_graphed(self, seqs, token_types) -> torch.Tensor:
        B, S = len(seqs), length_class(max(len(s) for s in seqs))
        g = self._graphs.get(("padded", B, S))
        if g is None:
            st = [torch.zeros(B, S, dtype=torch.int64, device=self.device) for _ in range(2)] \
                + [torch.zeros(B, S, dtype=torch.float32, device=self.device)]
            side = torch.cuda.Stream(self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side), torch.no_grad():
                self.model(*st)
            torch.cuda.current_stream(self.device).wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph), torch.no_grad():
                out = self.model(*st).float()
            host = [torch.empty(B, S, dtype=t.dtype, pin_memory=True) for t in st]
            g = self._graphs[("padded", B, S)] = (graph, out, st, host, torch.cuda.Event())
        g[4].synchronize()  # the previous copies out of the pinned buffers are done
        for h, dst, a in zip(g[3], g[2], _pad_arrays(seqs, token_types, S)):
            h.numpy()[...] = a
            dst.copy_(h, non_blocking=True)
        g[4].record(torch.cuda.current_stream(self.device))
        g[0].replay()
        return g[1].clone()
