"""BERT fine-tune trainer (BASELINE config 4): tensor-parallel across the node's GPUs, bf16 autocast
with fp32 master weights, fused AdamW, synthetic GLUE-shaped batches (no dataset downloads).

`python -m torch.distributed.run --nproc-per-node 8 -m mifx.trainer.bert_trainer --steps 50` runs TP=8."""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

from ..models.bert import BertConfig, BertForSequenceClassification
from ..parallel import dist as mdist
from ..parallel.tensor_parallel import TPGroup
from ..utils.meter import heartbeat
from .optim import FlatAdamW


GEMM_TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tunableop_bert_base_gfx950.csv")


def load_gemm_table(path: str = GEMM_TABLE) -> bool:
    """Use the hipBLASLt solutions recorded per BERT-base GEMM shape on an MI355X (PyTorch TunableOp results,
    read-only: no tuning at run time; shapes not in the table keep the library heuristic). Measured: 4592 ->
    4697 seq/s at B=32 S=128 (profiles/bert_base_bench_r2m*.json). Only on gfx950 with the table's library
    versions (TunableOp validates them and ignores a mismatching file)."""
    if not os.path.exists(path) or "gfx950" not in torch.cuda.get_device_properties(0).gcnArchName:
        return False
    import tempfile

    torch.cuda.tunable.enable(True)
    torch.cuda.tunable.tuning_enable(False)
    ok = bool(torch.cuda.tunable.read_file(path))
    # any results file TunableOp writes at exit goes to a scratch path, never over the bundled table
    torch.cuda.tunable.set_filename(os.path.join(tempfile.gettempdir(), f"mifx_tunableop_{os.getpid()}.csv"))
    return ok


def plan_train_batches(lengths, packed_tokens: int, max_seqs: int):
    """Greedily fill packed training batches in the given order: yields lists of indices into `lengths`, each of at
    most `packed_tokens` tokens and `max_seqs` sequences (a batch is closed when the next sequence does not fit)."""
    from ..models.bert_infer import plan_packs

    if packed_tokens < 1 or max_seqs < 1:
        raise ValueError(f"packed_tokens and max_seqs must be positive, got {packed_tokens}, {max_seqs}")
    lengths = [int(L) for L in lengths]
    for i, L in enumerate(lengths):
        if L < 1:
            raise ValueError(f"sequence {i}: empty")
    for s0, s1 in plan_packs(lengths, packed_tokens, max_seqs):
        yield list(range(s0, s1))


def synthetic_sequences(cfg: BertConfig, n: int, lo: int, hi: int, seed: int = 0):
    """n synthetic sequences with lengths uniform on [lo, hi] -> (token-id arrays, token-type arrays, labels)."""
    import numpy as np

    g = np.random.default_rng(seed)
    floor = min(1000, cfg.vocab_size // 4)
    seqs, tts = [], []
    for L in g.integers(lo, hi + 1, size=n):
        s = g.integers(floor, cfg.vocab_size, size=int(L)).astype(np.int64)
        s[0] = min(101, cfg.vocab_size - 1)  # [CLS]
        t = np.zeros(int(L), np.int64)
        t[int(L) // 2:] = 1 if cfg.type_vocab > 1 else 0
        seqs.append(s)
        tts.append(t)
    return seqs, tts, g.integers(0, cfg.num_labels, size=n).astype(np.int64)


def synthetic_batch(cfg: BertConfig, batch: int, seq: int, device, seed: int = 0):
    """Same tokens on every TP rank (TP ranks consume one replicated batch)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(min(1000, cfg.vocab_size // 4), cfg.vocab_size, (batch, seq), generator=g)
    ids[:, 0] = 101  # [CLS]
    tt = torch.zeros(batch, seq, dtype=torch.long)
    tt[:, seq // 2:] = 1
    am = torch.ones(batch, seq)
    y = torch.randint(0, cfg.num_labels, (batch,), generator=g)
    return ids.to(device), tt.to(device), am.to(device), y.to(device)


class BertTrainer:
    """One fine-tuning step = forward + backward + fused AdamW. On the GPU the whole step (HIP LN/GELU /
    bias-grad kernels, hipBLASLt GEMMs, attention, dropout RNG, optimizer, and the TP all-reduces) is
    captured once into a hipGraph and replayed: the eager step is host-bound (12.8 ms wall for 10.0 ms of
    GPU work). The model weights are bf16 views of one flat buffer updated by a single fused HIP AdamW
    launch with fp32 master weights that reads autograd's own gradient tensors in place
    (mifx.trainer.optim.FlatAdamW): no per-step weight/grad cast kernels, no gradient zero-fill, no
    per-parameter accumulate kernels.

    The standard BERT fine-tuning recipe is optional (all off by default): `max_grad_norm` clips by the global
    gradient norm, `warmup_steps` / `total_steps` give linear warmup then linear decay to zero at total_steps
    (total_steps None: constant learning rate), `no_decay_bias_norm` takes biases and LayerNorm parameters
    (`p.ndim <= 1`; the embeddings stay decayed) out of the weight decay. With FlatAdamW the norm, the clip
    coefficient and the learning rate are computed on the device inside the captured step; the stock-PyTorch
    optimizer path does the same on the host (two param groups, clip_grad_norm_, `group["lr"]` set before
    each eager step), so there a schedule cannot be combined with graph=True. `last_lr()` / `last_grad_norm()`
    report the last step's values. Clipping needs TP = 1 (the global norm over sharded plus replicated
    parameters needs a cross-rank reduction); the schedule and the no-decay set work at any TP degree.

    Packed variable-length batches (opt-in: `packed_tokens`; TP = 1): the step runs on [packed_tokens, hidden]
    activations holding up to `max_seqs` sequences of 1 .. `max_len` tokens back to back, no padding inside a
    sequence (BertForSequenceClassification.forward_packed; attention per sequence by
    csrc/attn_varlen_train.hip). `set_packed_batch` packs on the host and rewrites the step's static buffers; the
    captured step launches the grids of the capacity. The loss is the mean over the batch's real sequences."""

    def __init__(self, cfg: BertConfig, batch: int, seq: int, device, tp: TPGroup | None = None, lr: float = 2e-5,
                 graph: bool | None = None, flat_adamw: bool | None = None, sdpa: str | None = None,
                 tp_ipc: bool | None = None, max_grad_norm: float | None = None, warmup_steps: int = 0,
                 total_steps: int | None = None, no_decay_bias_norm: bool = False, packed_tokens: int | None = None,
                 max_seqs: int | None = None, max_len: int | None = None):
        """packed_tokens / max_seqs / max_len (all None: the padded trainer): token capacity of a packed step, its
        sequence slots (default 4 * packed_tokens // seq) and the longest sequence (default seq; at most 512 and
        the position table).
        tp_ipc (TP > 1 on the GPU; default on, MIFX_TP_IPC=0 turns it off): the TP all-reduces run on the
        peer-memory kernels of mifx.parallel.tp_ipc, so the TP step is captured into a hipGraph like the TP=1
        step (otherwise they are torch.distributed collectives and TP > 1 steps eagerly)."""
        self.cfg, self.batch, self.seq, self.device = cfg, batch, seq, torch.device(device)
        self.tp = tp or TPGroup(None)
        cuda = self.device.type == "cuda"
        self.packed = packed_tokens is not None
        if not self.packed and (max_seqs is not None or max_len is not None):
            raise ValueError("max_seqs and max_len belong to the packed path: set packed_tokens")
        if self.packed:
            from ..models import bert_infer as bim

            if self.tp.size > 1 or cfg.sequence_parallel:
                raise ValueError("packed variable-length batches need TP = 1 without sequence parallelism")
            self.max_len = int(seq if max_len is None else max_len)
            if not 1 <= self.max_len <= bim.max_length(cfg):
                raise ValueError(f"max_len {self.max_len} outside 1 .. {bim.max_length(cfg)} (the attention kernels' "
                                 f"512 and the position table)")
            self.packed_tokens = int(packed_tokens)
            self.max_seqs = int(max(1, 4 * self.packed_tokens // seq) if max_seqs is None else max_seqs)
            if self.packed_tokens < self.max_len or self.max_seqs < 1:
                raise ValueError(f"packed_tokens {self.packed_tokens} must hold a sequence of max_len {self.max_len}, "
                                 f"and max_seqs {self.max_seqs} must be positive")
        self.flat = cuda if flat_adamw is None else (flat_adamw and cuda)
        if max_grad_norm is not None and self.tp.size > 1:
            raise ValueError("max_grad_norm needs TP = 1: the global gradient norm over sharded and replicated "
                             "parameters needs a cross-rank reduction, which is not implemented")
        if total_steps is None:
            if warmup_steps:
                raise ValueError("warmup_steps needs total_steps (the step at which the learning rate reaches zero)")
            self.schedule = None
        else:
            if warmup_steps < 0 or total_steps <= warmup_steps:
                raise ValueError(f"need 0 <= warmup_steps < total_steps, got {warmup_steps}, {total_steps}")
            self.schedule = ("linear", int(warmup_steps), int(total_steps))
        if not self.flat and self.schedule is not None and graph:
            raise ValueError("a learning-rate schedule on the stock-PyTorch optimizer path is set from the host before "
                             "each eager step: it cannot be combined with graph=True (use the flat AdamW)")
        self.lr, self.max_grad_norm, self.no_decay_bias_norm = lr, max_grad_norm, bool(no_decay_bias_norm)
        self.model = BertForSequenceClassification(cfg, self.tp, seed=0).to(self.device)
        if tp_ipc is None:
            tp_ipc = os.environ.get("MIFX_TP_IPC", "1") != "0"
        if cuda and self.tp.size > 1 and tp_ipc:
            self.tp.enable_ipc(batch * seq * cfg.hidden, self.device)
        # The whole step is captured once as a hipGraph and replayed by default on the GPU (9.2 ms/step vs
        # 12.8 ms eager: the eager step is host-bound). The embeddings use a scatter-add backward
        # (mifx.ops.fused_bert.embedding): PyTorch's sort/unique embedding backward faults under hipGraph
        # replay on ROCm (rocPRIM partition kernel, diagnosed in round 1) and made the captured step go
        # non-finite after ~10 replays.
        # At TP > 1 the step is captured when the all-reduces are the peer-memory kernels (tp_ipc); over
        # torch.distributed collectives it steps eagerly unless graph=True is passed.
        self.use_graph = (cuda and (self.tp.size == 1 or self.tp.ipc is not None)) if graph is None \
            else (graph and cuda)
        if not self.flat and self.schedule is not None:
            self.use_graph = False  # the host sets group["lr"] before each step
        no_decay = (lambda p: p.ndim <= 1) if self.no_decay_bias_norm else None
        self._host_steps = 0  # stock-PyTorch path: optimizer steps taken (places the schedule)
        self._host_norm = None
        if self.flat:  # bf16 weights/grads as flat-buffer views + fp32 master, one fused HIP update
            self.opt = FlatAdamW(self.model.parameters(), lr=lr, weight_decay=0.01, max_grad_norm=max_grad_norm,
                                 schedule=self.schedule, no_decay=no_decay)
        else:
            params = list(self.model.parameters())
            if no_decay is not None:
                params = [{"params": [p for p in params if not no_decay(p)], "weight_decay": 0.01},
                          {"params": [p for p in params if no_decay(p)], "weight_decay": 0.0}]
            self.opt = torch.optim.AdamW(params, lr=lr, weight_decay=0.01, fused=cuda, capturable=self.use_graph)
        if self.model.sequence_parallel:
            if getattr(self.opt, "overlap", False):
                raise ValueError("sequence parallelism: the overlapped AdamW buckets would update the token-shard "
                                 "parameters before their gradients are summed over the group")
            if self.tp.ipc is not None and not self.tp.ipc.shard_ok(batch * seq * cfg.hidden):
                raise ValueError(f"sequence parallelism on the peer-memory path: batch x seq x hidden must split into "
                                 f"{self.tp.size} shards of whole {self.tp.ipc.chunk}-element chunks")
        # transposed copies of the projection weights for the dX GEMMs, refreshed in one launch before each backward
        self.tcache = None
        if self.flat:
            from ..ops import gemm as hg

            ws = [m.weight for layer in self.model.layers for m in (layer.qkv, layer.attn_out, layer.ffn_in,
                                                                      layer.ffn_out)]
            self.tcache = hg.TransposeCache(ws)
        self.data = None if self.packed else synthetic_batch(cfg, batch, seq, self.device)
        if self.packed:
            self._init_packed(cuda)
        self.amp = cuda
        self.sdpa = sdpa  # None = PyTorch's choice; "math" / "efficient" / "flash" pins the SDPA backend
        self.graph = None
        self.static_loss = None
        # MIFX_BERT_ASYNC_DW=1: weight gradients on a side stream (mifx.ops.gemm.async_weight_grads)
        self.async_dw = cuda and os.environ.get("MIFX_BERT_ASYNC_DW", "0") == "1"
        # deferred weight gradients (mifx.ops.gemm.deferred_weight_grads; MIFX_DEFER_DW=0 turns it off): the flat
        # optimizer resets every gradient to None each step, which the flush relies on
        self.defer_dw = cuda and self.flat and not self.async_dw and os.environ.get("MIFX_DEFER_DW", "1") != "0"
        # (TP ranks sharing one device -- the one-GPU rehearsals -- used to need it off: the grouped launch's
        # workgroups need a whole CU's register file, which the other ranks' spinning all-reduce waves held. The IPC
        # all-reduce now switches itself to split waits when ranks share a device (mifx.parallel.tp_ipc: no
        # data-moving workgroup spins, one wave waits), so the flush always finds whole CUs and the rehearsed step is
        # the shipped one.)

    def set_batch(self, ids, tt, am, y) -> None:
        """Next training batch, copied INTO the step's input tensors (a captured hipGraph reads these same
        buffers on every replay)."""
        for dst, src in zip(self.data, (ids, tt, am, y)):
            dst.copy_(src.to(dst.dtype), non_blocking=True)

    def _init_packed(self, cuda: bool) -> None:
        """Static buffers of the packed step: one int32 staging buffer (mifx.models.bert_infer.staging_views: ids,
        token types, position ids, cu_seqlens, first rows, block table; then max_seqs labels), pinned on the host and
        mirrored on the device, and a first synthetic batch of full-length sequences."""
        from ..models import bert_infer as bim

        C, B = self.packed_tokens, self.max_seqs
        n = bim.staging_size(C, B)
        self._phost = torch.empty(n + B, dtype=torch.int32, pin_memory=cuda)
        self._pnp = self._phost.numpy()
        self._pdev = torch.empty(n + B, dtype=torch.int32, device=self.device) if cuda else self._phost
        self.pviews = bim.staging_views(self._pdev[:n], C, B)
        self.plabels = self._pdev[n:]
        self._pcopied = torch.cuda.Event() if cuda else None
        self.packed_batch = (0, 0)  # (tokens, sequences) of the current batch
        k = max(1, min(B, C // self.max_len))
        seqs, tts, y = synthetic_sequences(self.cfg, k, self.max_len, self.max_len)
        self.set_packed_batch(seqs, tts, y)

    def set_packed_batch(self, seqs, token_types, labels) -> None:
        """Next packed training batch: `seqs` a list of token-id lists (1 .. max_len ids each, at most max_seqs of
        them and packed_tokens tokens in all), `token_types` None or per-sequence lists (None entries: zeros),
        `labels` one class per sequence. Packed on the host and copied INTO the step's static buffers in one copy
        (a captured hipGraph reads the same buffers on every replay). Padding rows carry id 0 and position 0, empty
        sequence slots label -100."""
        import numpy as np

        from ..models import bert_infer as bim

        if not self.packed:
            raise ValueError("set_packed_batch needs a trainer built with packed_tokens")
        seqs = [np.asarray(s) for s in seqs]
        if not seqs:
            raise ValueError("a packed batch needs at least one sequence")
        bim.validate(seqs, token_types, self.cfg)
        lens = [len(s) for s in seqs]
        for i, L in enumerate(lens):
            if L > self.max_len:
                raise ValueError(f"sequence {i}: length {L} above max_len {self.max_len}")
        if len(seqs) > self.max_seqs:
            raise ValueError(f"{len(seqs)} sequences above max_seqs {self.max_seqs}")
        if sum(lens) > self.packed_tokens:
            raise ValueError(f"{sum(lens)} tokens above packed_tokens {self.packed_tokens}")
        y = np.asarray(labels)
        if y.shape != (len(seqs),) or y.dtype.kind not in "iu":
            raise ValueError(f"{y.size} labels for {len(seqs)} sequences (one integer class each)")
        if int(y.min()) < 0 or int(y.max()) >= self.cfg.num_labels:
            raise ValueError(f"label outside [0, {self.cfg.num_labels})")
        if self._pcopied is not None:
            self._pcopied.synchronize()  # the previous copy out of the pinned buffer is done
        n = bim.staging_size(self.packed_tokens, self.max_seqs)
        p = bim.pack(seqs, token_types, self.packed_tokens, self.max_seqs, out=self._pnp[:n])
        p.ids[p.tokens:] = 0  # a valid id: the embedding lookup reads every row (inference marks them -1)
        self._pnp[n:n + len(seqs)] = y
        self._pnp[n + len(seqs):] = -100
        if self._pcopied is not None:
            self._pdev.copy_(self._phost, non_blocking=True)
            self._pcopied.record(torch.cuda.current_stream(self.device))
        self.packed_batch = (p.tokens, p.seqs)

    @torch.no_grad()
    def predict(self, ids, tt, am) -> torch.Tensor:
        """Eval-mode logits (every TP rank must call it: the forward all-reduces)."""
        self.model.eval()
        try:
            with torch.autocast(self.device.type, dtype=torch.bfloat16, enabled=self.amp):
                return self.model(ids.to(self.device), tt.to(self.device), am.to(self.device).float()).float()
        finally:
            self.model.train()

    def _eager_step(self) -> torch.Tensor:
        if not self.packed:
            ids, tt, am, y = self.data
        if self.flat:
            self.opt.zero_grad()  # in-place (gradients are views of one flat buffer): part of the step
        # the autocast weight-cast cache must be off for a step that is captured into a graph (PyTorch's
        # CUDA-graph rules: cached casts created outside the capture must not be referenced by it)
        with torch.autocast(self.device.type, dtype=torch.bfloat16, enabled=self.amp,
                            cache_enabled=not self.use_graph), self._sdpa_ctx():
            if self.packed:
                v = self.pviews
                logits = self.model.forward_packed(v.ids, v.tts, v.pos, v.cu, v.table, self.max_seqs, self.max_len,
                                                   v.first)
            else:
                logits = self.model(ids, tt, am)
        if self.packed:  # the mean over the real sequences (empty slots: label -100), on the device
            loss = F.cross_entropy(logits.float(), self.plabels.long(), ignore_index=-100)
        else:
            loss = F.cross_entropy(logits.float(), y)
        from ..ops import gemm as hg

        if self.tcache is not None:
            # the transposed weight copies the dX GEMMs read, refreshed from the CURRENT weights right before the
            # backward (once per step, inside the captured graph): a weight change between steps (an update, a
            # load_state_dict, a warm start) can never leave the backward with stale transposes
            self.tcache.refresh()
        with hg.use_transposes(self.tcache):
            if self.async_dw:  # weight-gradient GEMMs on a side stream beside the backward's dX chain
                with hg.async_weight_grads():
                    loss.backward()
                hg.join_weight_grads(self.device)
            elif self.defer_dw:  # every weight gradient in ONE grouped launch after the backward
                with hg.deferred_weight_grads():
                    loss.backward()
                hg.flush_weight_grads()
            else:
                loss.backward()
        # sequence parallelism: the LayerNorm / row-parallel-bias gradients are per-shard partial sums
        self.model.sync_sequence_parallel_grads()
        if not self.flat:  # the recipe on the stock optimizer (FlatAdamW does it on the device, inside its step)
            if self.max_grad_norm is not None:
                self._host_norm = torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.max_grad_norm)
            if self.schedule is not None:
                from ..ops.adamw import scheduled_lr

                for group in self.opt.param_groups:
                    group["lr"] = scheduled_lr(self.lr, self.schedule, self._host_steps)
            self._host_steps += 1
        self.opt.step()
        return loss.detach()

    def last_lr(self) -> float:
        """Learning rate of the last optimizer step (host sync on the flat path: for logging)."""
        if self.flat:
            return self.opt.last_lr()
        from ..ops.adamw import scheduled_lr

        return scheduled_lr(self.lr, self.schedule, max(0, self._host_steps - 1))

    def last_grad_norm(self) -> float | None:
        """Global gradient norm before clipping at the last step; None without max_grad_norm (host sync)."""
        if self.flat:
            return self.opt.last_grad_norm()
        return None if self._host_norm is None else float(self._host_norm)

    def _sdpa_ctx(self):
        if self.sdpa is None:
            return contextlib.nullcontext()
        from torch.nn.attention import SDPBackend, sdpa_kernel

        return sdpa_kernel({"math": SDPBackend.MATH, "efficient": SDPBackend.EFFICIENT_ATTENTION,
                            "flash": SDPBackend.FLASH_ATTENTION}[self.sdpa])

    def _capture(self, warmup: int = 3) -> None:
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):  # warm up on a side stream: lazy state (AdamW moments, caches)
            for _ in range(warmup):
                self.opt.zero_grad(set_to_none=True)
                self._eager_step()
        torch.cuda.current_stream(self.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        self.opt.zero_grad(set_to_none=True)
        if hasattr(self.opt, "begin_capture"):  # FlatAdamW: bucket updates overlapped with the backward
            self.opt.begin_capture()
        with torch.cuda.graph(self.graph):
            self.static_loss = self._eager_step()

    # TP health check cadence: the peer-memory all-reduce reports a peer that never arrived through a sticky device
    # flag (its later kernels then write NaN); reading it is a host sync, so step() reads it every CHECK_EVERY steps
    CHECK_EVERY = 100

    def check(self) -> None:
        """Raise if a TP all-reduce of this trainer's group timed out (no-op at TP = 1 / without the IPC path)."""
        self.tp.check()

    def step(self) -> torch.Tensor:
        self.steps_done = getattr(self, "steps_done", 0) + 1
        if self.tp.ipc is not None and self.steps_done % self.CHECK_EVERY == 0:
            self.check()
        if self.use_graph:
            if self.graph is None:
                self._capture()
            self.graph.replay()
            return self.static_loss
        self.opt.zero_grad(set_to_none=True)
        return self._eager_step()

    def load_weights(self, state: dict) -> None:
        """Load a (full or TP-sharded) state dict into the model and refresh everything derived from the weights
        (the transposed copies of the dX GEMMs). Use this instead of model.load_state_dict after construction."""
        self.model.load_state_dict(state)
        if self.flat and hasattr(self.opt, "reload_master"):
            self.opt.reload_master()
        if self.tcache is not None:
            self.tcache.refresh()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--graph", action="store_true", help="capture the step as one hipGraph also at TP>1")
    ap.add_argument("--no-graph", action="store_true", help="eager steps instead of one captured hipGraph")
    ap.add_argument("--no-flat-adamw", action="store_true",
                    help="eager mode: fp32 params + torch fused AdamW instead of the flat HIP AdamW")
    ap.add_argument("--tunable", default=None, metavar="CSV",
                    help="enable PyTorch TunableOp: benchmark hipBLASLt/rocBLAS solutions per GEMM shape during "
                         "warmup and keep the best (results cached in CSV)")
    ap.add_argument("--no-gemm-table", action="store_true",
                    help="do not load the bundled per-shape GEMM solution table (tunableop_bert_base_gfx950.csv)")
    ap.add_argument("--seed", type=int, default=None, help="torch.manual_seed before building the trainer")
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--sequence-parallel", action="store_true",
                    help="at TP > 1: split the residual stream / LayerNorms / dropouts over the ranks by token")
    ap.add_argument("--sdpa", choices=["math", "efficient", "flash"], default=None,
                    help="pin the scaled-dot-product-attention backend (default: PyTorch's choice)")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip gradients by this global L2 norm")
    ap.add_argument("--warmup-steps", type=int, default=0, help="linear learning-rate warmup (needs --total-steps)")
    ap.add_argument("--total-steps", type=int, default=None,
                    help="linear decay of the learning rate to zero at this step (default: constant)")
    ap.add_argument("--no-decay-bias-norm", action="store_true",
                    help="no weight decay on biases and LayerNorm parameters")
    ap.add_argument("--packed-tokens", type=int, default=None, metavar="C",
                    help="packed variable-length batches: token capacity of a step (TP = 1; default: padded batches)")
    ap.add_argument("--max-seqs", type=int, default=None,
                    help="sequence slots of a packed step (default 4 * packed-tokens / seq)")
    ap.add_argument("--length-range", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                    help="synthetic sequences with lengths uniform on [LO, HI] (seeded), a new batch every step: "
                         "padded to --seq with the attention mask, or packed with --packed-tokens")
    a = ap.parse_args(argv)
    if a.max_seqs is not None and a.packed_tokens is None:
        ap.error("--max-seqs needs --packed-tokens")
    if a.length_range is not None and not 1 <= a.length_range[0] <= a.length_range[1] <= a.seq:
        ap.error("--length-range needs 1 <= LO <= HI <= --seq")
    if a.seed is not None:
        torch.manual_seed(a.seed)
    if a.tunable and torch.cuda.is_available():
        torch.cuda.tunable.enable(True)
        torch.cuda.tunable.tuning_enable(True)
        torch.cuda.tunable.set_filename(a.tunable)
        torch.cuda.tunable.set_max_tuning_iterations(30)
    elif not a.no_gemm_table and os.environ.get("MIFX_BERT_GEMM_TABLE", "1") != "0" and torch.cuda.is_available():
        load_gemm_table()
    env = mdist.init()
    # MIFX_SHARED_GPU=1 (with MIFX_DIST_BACKEND=gloo): the multi-rank flow rehearsed with every rank on cuda:0
    local = 0 if os.environ.get("MIFX_SHARED_GPU") == "1" else env.local_rank
    dev = torch.device("cuda", local) if torch.cuda.is_available() else torch.device("cpu")
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    tp = TPGroup(torch.distributed.group.WORLD if env.world_size > 1 else None)
    cfg = BertConfig(layers=a.layers, dropout=a.dropout, sequence_parallel=a.sequence_parallel)
    tr = BertTrainer(cfg, a.batch, a.seq, dev, tp,
                     graph=False if a.no_graph else (True if a.graph else None),
                     flat_adamw=False if a.no_flat_adamw else None, sdpa=a.sdpa, max_grad_norm=a.max_grad_norm,
                     warmup_steps=a.warmup_steps, total_steps=a.total_steps, no_decay_bias_norm=a.no_decay_bias_norm,
                     packed_tokens=a.packed_tokens, max_seqs=a.max_seqs)
    from ..ops import native_stats

    # the batches of the run: None (the trainer's own static batch, as always), or a cycle over synthetic
    # variable-length sequences, packed greedily or padded in groups of --batch
    feed = None
    if a.length_range is not None or a.packed_tokens is not None:
        lo, hi = a.length_range or (a.seq, a.seq)
        seqs, tts, ys = synthetic_sequences(cfg, 16 * a.batch, lo, hi, seed=0 if a.seed is None else a.seed)
        if a.packed_tokens is not None:
            groups = list(plan_train_batches([len(s) for s in seqs], tr.packed_tokens, tr.max_seqs))
        else:
            groups = [list(range(i, i + a.batch)) for i in range(0, len(seqs), a.batch)]
        feed = [([seqs[j] for j in g], [tts[j] for j in g], ys[g]) for g in groups]
    n_seq = n_tok = 0

    def next_batch(i: int) -> tuple:
        """Set step i's batch; returns its (sequences, real tokens)."""
        if feed is None:
            return a.batch, a.batch * a.seq
        b = feed[i % len(feed)]
        if tr.packed:
            tr.set_packed_batch(*b)
        else:
            from ..models.bert_infer import _pad_arrays

            tr.set_batch(*(torch.from_numpy(x) for x in _pad_arrays(b[0], b[1], a.seq)), torch.from_numpy(b[2]))
        return len(b[0]), sum(len(s) for s in b[0])

    per_step = None
    with heartbeat("bert warmup"):
        for i in range(a.warmup):
            if i == 0:
                native_stats.reset()
            next_batch(i)
            tr.step()
            if i == 0:  # the first step runs every dispatch in Python: which path each GEMM / attention call took
                per_step = native_stats.snapshot()
        if dev.type == "cuda":
            torch.cuda.synchronize()
    tr.check()  # a timed-out TP all-reduce during warmup fails the run here (outside the timed region)
    mdist.barrier()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    trace = os.environ.get("MIFX_BERT_TRACE") == "1"  # diagnostic: per-step loss (adds a sync per step)
    sync_each = os.environ.get("MIFX_BERT_SYNC") == "1"  # diagnostic: device sync after every step
    t0 = time.perf_counter()
    for i in range(a.steps):
        ns, nt = next_batch(a.warmup + i)
        n_seq, n_tok = n_seq + ns, n_tok + nt
        loss = tr.step()
        if sync_each and dev.type == "cuda":
            torch.cuda.synchronize()
        if trace and env.rank == 0:
            print(f"[bert] step {i} loss {float(loss):.5f}", file=sys.stderr, flush=True)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    mdist.barrier()
    dt = mdist.max_over_ranks(time.perf_counter() - t0)
    tr.check()  # ... and during the timed steps: never report a throughput of garbage activations
    if env.rank == 0:
        print(json.dumps({"metric": "BERT-base fine-tune sequences/sec (TP over the node)", "value": n_seq / dt,
                          "unit": "sequences/s", "sequences/s": n_seq / dt, "tokens/s": n_tok / dt,
                          "packed_tokens": a.packed_tokens, "max_seqs": tr.max_seqs if tr.packed else None,
                          "length_range": a.length_range, "mean_sequences_per_step": n_seq / max(1, a.steps),
                          "n_gpus": env.world_size, "tp": tp.size,
                          "sequence_parallel": tr.model.sequence_parallel, "batch": a.batch,
                          "seq_len": a.seq, "ms_per_step": 1e3 * dt / a.steps, "loss": float(loss),
                          "dtype": "bf16", "data": "synthetic", "layers": a.layers,
                          "hipgraph": tr.graph is not None,
                          "lr_schedule": "constant" if tr.schedule is None else
                          {"kind": "linear", "warmup_steps": tr.schedule[1], "total_steps": tr.schedule[2]},
                          "max_grad_norm": a.max_grad_norm, "grad_norm": tr.last_grad_norm(),
                          "no_decay_bias_norm": a.no_decay_bias_norm,
                          "calls_per_step_native_vs_fallback": per_step,
                          "optimizer": "flat bf16 AdamW (fp32 master)" if tr.flat else "torch fused AdamW"}),
              flush=True)
    mdist.shutdown()


if __name__ == "__main__":
    main()
