"""TF-semantics optimizers for the PyTorch reference path.

The canned DNNLinearCombinedClassifier (`taxi_utils.py:186-191`) trains its DNN with Adagrad
(lr 0.05, initial accumulator 0.1) and its linear part with FTRL (lr = min(0.2, 1/sqrt(#cols)),
lr_power -0.5, initial accumulator 0.1). These match TF's ApplyAdagrad / ApplyFtrl update rules
exactly (no epsilon), as does the fused HIP optimizer in csrc/wide_deep.hip.
"""
from __future__ import annotations

import functools
import os

import torch


class TFAdagrad(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 0.05, initial_accumulator_value: float = 0.1):
        super().__init__(params, dict(lr=lr, init=initial_accumulator_value))

    @torch.no_grad()
    def step(self, closure=None):
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "acc" not in st:
                    st["acc"] = torch.full_like(p, g["init"])
                st["acc"].addcmul_(p.grad, p.grad)
                p.addcdiv_(p.grad, st["acc"].sqrt(), value=-g["lr"])


class Ftrl(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 0.2, lr_power: float = -0.5, initial_accumulator_value: float = 0.1,
                 l1: float = 0.0, l2: float = 0.0):
        super().__init__(params, dict(lr=lr, lr_power=lr_power, init=initial_accumulator_value, l1=l1, l2=l2))

    @torch.no_grad()
    def step(self, closure=None):
        for g in self.param_groups:
            lr, pw, l1, l2 = g["lr"], g["lr_power"], g["l1"], g["l2"]
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "acc" not in st:
                    st["acc"] = torch.full_like(p, g["init"])
                    st["lin"] = torch.zeros_like(p)
                acc, lin, grad = st["acc"], st["lin"], p.grad
                new_acc = acc + grad * grad
                if pw == -0.5:
                    sq_new, sq_old = new_acc.sqrt(), acc.sqrt()
                else:
                    sq_new, sq_old = new_acc.pow(-pw), acc.pow(-pw)
                lin.add_(grad - (sq_new - sq_old) / lr * p)
                quad = sq_new / lr + 2 * l2
                p.copy_(torch.where(lin.abs() > l1, (torch.sign(lin) * l1 - lin) / quad, torch.zeros_like(p)))
                acc.copy_(new_acc)


def make_optimizer(kind: str, params, lr: float, **kw) -> torch.optim.Optimizer:
    kind = kind.lower()
    if kind == "adagrad":
        return TFAdagrad(params, lr=lr, **kw)
    if kind == "ftrl":
        return Ftrl(params, lr=lr, **kw)
    if kind == "adam":
        return torch.optim.Adam(params, lr=lr, **kw)
    if kind == "sgd":
        return torch.optim.SGD(params, lr=lr, **kw)
    raise ValueError(f"unknown optimizer {kind}")


class FlatAdamW:
    """AdamW over a model whose parameters are re-homed as bf16 views of ONE flat buffer, with fp32 master
    weights / moments kept here. `step()` is a single fused HIP launch (mifx.ops.adamw).

    Gradients (`grads=`):
      * "own" (default on the GPU): autograd's own per-parameter gradient tensors are read in place by the
        chunked kernel (a per-step table of their addresses), `zero_grad()` sets them to None -- no zero-fill
        and no `grad += new` accumulate kernel per parameter per step;
      * "views": gradients are views of one flat gradient buffer that autograd accumulates into (one memset
        per `zero_grad()`); the flat kernel is then hipGraph-capturable (device-side step counter).

    Fine-tuning recipe (all off by default; with them off the step is the plain update, bit for bit):
      * `max_grad_norm`: clip by the global L2 norm of all gradients (torch.nn.utils.clip_grad_norm_ semantics,
        error_if_nonfinite=False). Two extra launches per step (per-chunk sums of squares, then one workgroup
        that writes {coef, norm}); no atomics, bit-reproducible;
      * `schedule=("linear", warmup_steps, total_steps)`: linear warmup from 0, then linear decay to 0 at
        total_steps, stepped once per update (LambdaLR with the usual lambda). The kernel evaluates it from the
        device-side step counter, so a captured step follows the schedule on every replay;
      * `no_decay`: parameters for which it returns true get weight decay 0 (a per-parameter table).
    On the GPU these need grads="own" without overlap (a bucket launched during the backward cannot know the
    global norm; the "views" kernel has no parameter boundaries). On the CPU they run through the PyTorch
    reference (mifx.ops.adamw.adamw_recipe_reference_), which reads each parameter's `.grad`.
    `last_grad_norm()` / `last_lr()` report the last step's values (a host sync each: for logging).
    `state_dict()` carries the step counter, so `load_state_dict()` resumes the schedule where it stopped."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 dtype: torch.dtype = torch.bfloat16, grads: str | None = None, overlap: bool | None = None,
                 bucket_elems: int = 8 << 20, max_grad_norm: float | None = None, schedule: tuple | None = None,
                 no_decay=None):
        self.params = [p for p in params if p.requires_grad]
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        dev = self.params[0].device
        if schedule is not None:
            if len(schedule) != 3 or schedule[0] != "linear":
                raise ValueError('schedule must be None or ("linear", warmup_steps, total_steps)')
            warmup, total = int(schedule[1]), int(schedule[2])
            if warmup < 0 or total < 0 or total <= warmup:
                raise ValueError(f"schedule needs 0 <= warmup_steps < total_steps, got {warmup}, {total}")
            schedule = ("linear", warmup, total)
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.schedule = schedule
        self.recipe = max_grad_norm is not None or schedule is not None or no_decay is not None
        if self.recipe and overlap:
            raise ValueError("FlatAdamW: max_grad_norm / schedule / no_decay cannot be combined with overlap=True "
                             "(a bucket updated during the backward cannot know the global gradient norm)")
        if grads is None:
            grads = "own" if dev.type == "cuda" and dtype == torch.bfloat16 else "views"
        if grads not in ("own", "views"):
            raise ValueError("grads must be 'own' or 'views'")
        if grads == "own" and (dev.type != "cuda" or dtype != torch.bfloat16):
            raise ValueError("grads='own' needs bf16 parameters on the GPU")
        if self.recipe and grads == "views" and dev.type == "cuda":
            raise ValueError("FlatAdamW: max_grad_norm / schedule / no_decay on the GPU need grads='own' (the flat "
                             "'views' kernel has no parameter boundaries)")
        self.mode = grads
        align = 8 if grads == "own" else 1  # 16-byte aligned bf16 / 32-byte fp32 vectors per parameter
        offs, off = [], 0
        for p in self.params:
            offs.append(off)
            off += (p.numel() + align - 1) // align * align
        n = off
        self.n = n
        self.flat = torch.zeros(n, device=dev, dtype=dtype)
        self.flat_grad = torch.zeros(n, device=dev, dtype=dtype) if grads == "views" else None
        self.master = torch.zeros(n, device=dev, dtype=torch.float32)
        self.m = torch.zeros(n, device=dev, dtype=torch.float32)
        self.v = torch.zeros(n, device=dev, dtype=torch.float32)
        self.step_count = torch.zeros((), device=dev, dtype=torch.int32)
        self._offs = offs
        self._pwd_host = None if no_decay is None else [0.0 if no_decay(p) else float(weight_decay)
                                                        for p in self.params]
        self._cpu_norm = None
        with torch.no_grad():
            for p, off in zip(self.params, offs):
                k = p.numel()
                self.master[off:off + k].copy_(p.detach().reshape(-1).float())
                self.flat[off:off + k].copy_(p.detach().reshape(-1))
                p.data = self.flat[off:off + k].view(p.shape)
                p.grad = self.flat_grad[off:off + k].view(p.shape) if grads == "views" else None
        if grads == "own":
            from ..ops.adamw import chunk_size

            ch = chunk_size()
            bp, bo, bn = [], [], []
            for i, p in enumerate(self.params):
                for o in range(0, p.numel(), ch):
                    bp.append(i)
                    bo.append(o)
                    bn.append(min(ch, p.numel() - o))
            self.poff = torch.tensor(offs, dtype=torch.int64, device=dev)
            self._gptr = torch.zeros(len(self.params), dtype=torch.int64, device=dev)  # grad addresses
            self._capture_host = torch.zeros(len(self.params), dtype=torch.int64).pin_memory()
            self._addr = None
            self.bp, self.bo, self.bn = (torch.tensor(x, dtype=torch.int32, device=dev) for x in (bp, bo, bn))
            # overlap (opt-in: overlap=True or MIFX_ADAMW_OVERLAP=1): in a CAPTURED step, the update of each bucket of
            # ~bucket_elems consecutive parameters is launched on a side stream as soon as autograd has accumulated
            # the last gradient of the bucket (post-accumulate-grad hooks), so the memory-bound update of layer L
            # runs under the compute-bound backward of layers < L; step() launches what is left, joins the side
            # stream and advances the step counter once. Every bucket reads the same step value, so the update is
            # the single-launch update, bucket by bucket (same kernel, same per-element math). Measured SLOWER in the
            # BERT-base step (7.18 vs 6.38 ms on MI355X, profiles/archive/bert_adamw_overlap_r3.txt): the bucket launches fill
            # every CU with memory-bound blocks beside the backward's one-workgroup-per-CU GEMMs, which lose more
            # than the ~0.5 ms update that is hidden.
            if overlap is None:
                overlap = os.environ.get("MIFX_ADAMW_OVERLAP", "0") == "1"
            self.overlap = bool(overlap)
            if self.overlap and self.recipe:
                raise ValueError("FlatAdamW: max_grad_norm / schedule / no_decay cannot be combined with the "
                                 "overlapped update (MIFX_ADAMW_OVERLAP=1)")
            # recipe buffers, allocated here: nothing may allocate during a capture
            self.pwd = None if self._pwd_host is None else torch.tensor(self._pwd_host, dtype=torch.float32,
                                                                        device=dev)
            self.clip = self._partial = None
            if self.max_grad_norm is not None:
                self._partial = torch.zeros(len(bp), dtype=torch.float32, device=dev)  # per-chunk sums of squares
                self.clip = torch.zeros(2, dtype=torch.float32, device=dev)  # {coef, norm} of the last step
            if self.overlap:
                self._buckets, cur, acc = [], [], 0
                for i, p in enumerate(self.params):
                    cur.append(i)
                    acc += p.numel()
                    if acc >= bucket_elems:
                        self._buckets.append(cur)
                        cur, acc = [], 0
                if cur:
                    self._buckets.append(cur)
                self._bucket_of = {i: b for b, idx in enumerate(self._buckets) for i in idx}
                self._bchunks = []
                for idx in self._buckets:
                    sel = [k for k, pi in enumerate(bp) if idx[0] <= pi <= idx[-1]]
                    self._bchunks.append(tuple(torch.tensor([x[k] for k in sel], dtype=torch.int32, device=dev)
                                               for x in (bp, bo, bn)))
                self._ov_host = torch.zeros(len(self.params), dtype=torch.int64).pin_memory()
                self._ov_side = torch.cuda.Stream(dev)
                self._ov_ready = [0] * len(self._buckets)
                self._ov_launched = [False] * len(self._buckets)
                self._ov_active = False
                self._ov_captured = False
                for i, p in enumerate(self.params):
                    p.register_post_accumulate_grad_hook(functools.partial(self._on_grad, i))

    @torch.no_grad()
    def reload_master(self) -> None:
        """Re-derive the fp32 master weights from the bf16 parameters after they were written from outside the
        optimizer (load_state_dict into the flat views, a warm start): otherwise the next step would overwrite the
        loaded weights with the stale master copy."""
        self.master.copy_(self.flat.float())

    # ---------------------------------------------------------------- overlapped update (captured steps)
    def _on_grad(self, i: int, p: torch.Tensor) -> None:
        if not (self._ov_active and torch.cuda.is_current_stream_capturing()):
            return
        b = self._bucket_of[i]
        self._ov_ready[b] += 1
        if self._ov_ready[b] == len(self._buckets[b]) and not self._ov_launched[b]:
            self._launch_bucket(b)

    def _launch_bucket(self, b: int) -> None:
        from ..ops.adamw import adamw_chunks_

        idx = self._buckets[b]
        i0, i1 = idx[0], idx[-1] + 1
        host = self._ov_host.numpy()
        for i in idx:
            g = self.params[i].grad
            if g is not None and (g.dtype != torch.bfloat16 or not g.is_contiguous() or g.device != self.flat.device):
                raise RuntimeError("FlatAdamW(grads='own') needs contiguous bf16 gradients on the parameter's device")
            host[i] = 0 if g is None else g.data_ptr()
        cur = torch.cuda.current_stream(self.flat.device)
        self._ov_side.wait_stream(cur)  # the bucket's gradients (and the backward kernels that read its weights)
        with torch.cuda.stream(self._ov_side):
            # captured H2D copy: reads the pinned table on every replay (the captured gradients keep their
            # addresses, so the table is written once, here)
            self._gptr[i0:i1].copy_(self._ov_host[i0:i1], non_blocking=True)
            bpb, bob, bnb = self._bchunks[b]
            adamw_chunks_(self.flat, self._gptr, self.poff, bpb, bob, bnb, self.master, self.m, self.v,
                          self.step_count, self.lr, self.betas[0], self.betas[1], self.eps, self.wd, advance=False)
        self._ov_launched[b] = True

    def begin_capture(self) -> None:
        """Arm the overlapped update for the step about to be captured (one captured step per optimizer)."""
        if self.mode == "own" and self.overlap:
            if self._ov_captured:
                raise RuntimeError("FlatAdamW overlap: one captured step per optimizer")
            self._ov_ready = [0] * len(self._buckets)
            self._ov_launched = [False] * len(self._buckets)
            self._ov_active = True

    def zero_grad(self, set_to_none: bool = True) -> None:
        if self.mode == "own":
            for p in self.params:
                p.grad = None
        else:  # grads stay views of the flat buffer
            self.flat_grad.zero_()

    def step(self) -> None:
        from ..ops.adamw import adamw_chunks_, adamw_flat_

        if self.mode == "views" and self.recipe:  # CPU: the PyTorch reference, parameter by parameter
            from ..ops.adamw import adamw_recipe_reference_

            with torch.no_grad():
                sl = [slice(o, o + p.numel()) for o, p in zip(self._offs, self.params)]
                self._cpu_norm, _ = adamw_recipe_reference_(
                    [self.flat[s] for s in sl], [p.grad for p in self.params], [self.master[s] for s in sl],
                    [self.m[s] for s in sl], [self.v[s] for s in sl], self.step_count, self.lr, self.betas[0],
                    self.betas[1], self.eps, self.wd if self._pwd_host is None else self._pwd_host,
                    max_grad_norm=self.max_grad_norm, schedule=self.schedule)
            return
        if self.mode == "views":
            adamw_flat_(self.flat, self.flat_grad, self.master, self.m, self.v, self.step_count, self.lr,
                        self.betas[0], self.betas[1], self.eps, self.wd)
            return
        addr = []
        for p in self.params:
            g = p.grad
            if g is not None and (g.dtype != torch.bfloat16 or not g.is_contiguous() or g.device != p.device):
                raise RuntimeError("FlatAdamW(grads='own') needs contiguous bf16 gradients on the parameter's device")
            addr.append(0 if g is None else g.data_ptr())
        addr = tuple(addr)
        if self.overlap and self._ov_active and torch.cuda.is_current_stream_capturing():
            from ..ops.adamw import adamw_advance_

            for b in range(len(self._buckets)):  # buckets whose last gradient never arrived (unused parameters)
                if not self._ov_launched[b]:
                    self._launch_bucket(b)
            torch.cuda.current_stream(self.flat.device).wait_stream(self._ov_side)
            adamw_advance_(self.step_count)
            self._ov_active, self._ov_captured = False, True
            self._capture_host = None
            return
        if torch.cuda.is_current_stream_capturing():
            # hipGraph capture: no pinned allocation is allowed here, so the table goes through the pinned
            # buffer reserved at construction; the captured copy reads it on every replay, so it is never
            # written again (the captured gradients keep their addresses on every replay)
            if self._capture_host is None:
                raise RuntimeError("FlatAdamW(grads='own') supports one captured step per optimizer")
            self._capture_host.numpy()[:] = addr
            self._gptr.copy_(self._capture_host, non_blocking=True)
            # the pinned table must outlive the graph: once released, the host allocator hands the block to the next
            # pinned allocation of its size (another optimizer's eager address upload, a pinned batch), and every
            # replay of this step would copy that tensor's contents in as gradient addresses
            self._captured_table = self._capture_host
            self._capture_host, self._addr = None, addr
        elif addr != self._addr:  # eager: upload only when autograd handed out new gradient addresses
            self._gptr.copy_(torch.tensor(addr, dtype=torch.int64).pin_memory(), non_blocking=True)
            self._addr = addr
        if self.recipe:
            from ..ops.adamw import adamw_chunks_ex_, clip_coef_

            if self.max_grad_norm is not None:
                clip_coef_(self._gptr, self.bp, self.bo, self.bn, self._partial, self.max_grad_norm, self.clip)
            adamw_chunks_ex_(self.flat, self._gptr, self.poff, self.bp, self.bo, self.bn, self.master, self.m, self.v,
                             self.step_count, self.lr, self.betas[0], self.betas[1], self.eps, self.wd,
                             clip=self.clip, pwd=self.pwd, schedule=self.schedule)
            return
        adamw_chunks_(self.flat, self._gptr, self.poff, self.bp, self.bo, self.bn, self.master, self.m, self.v,
                      self.step_count, self.lr, self.betas[0], self.betas[1], self.eps, self.wd)

    def last_grad_norm(self) -> float | None:
        """Global gradient norm (before clipping) of the last step; None without max_grad_norm. Host sync."""
        if self.max_grad_norm is None:
            return None
        return float(self.clip[1]) if self.mode == "own" else self._cpu_norm

    def last_lr(self) -> float:
        """Learning rate the last step used (the schedule at step_count - 1). Host sync."""
        from ..ops.adamw import scheduled_lr

        return scheduled_lr(self.lr, self.schedule, max(0, int(self.step_count) - 1))

    def state_dict(self) -> dict:
        return {"master": self.master, "m": self.m, "v": self.v, "step": self.step_count}

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """Resume from a state_dict() of an optimizer over the same parameters: master weights, moments and the step
        counter (which also places the learning-rate schedule); the model weights are re-derived from the master."""
        for k, dst in (("master", self.master), ("m", self.m), ("v", self.v), ("step", self.step_count)):
            dst.copy_(sd[k])
        self.flat.copy_(self.master.to(self.flat.dtype))
