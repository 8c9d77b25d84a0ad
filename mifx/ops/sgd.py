"""Multi-tensor fused SGD (csrc/sgd.hip): weight decay, momentum, dampening and Nesterov for a list of fp32
parameters in ONE launch, learning rate read from a device tensor (graph-capturable). `FusedSGDTables` builds the
per-tensor address / chunk tables once, outside any capture; `sgd_reference_` is the torch.optim.SGD foreach
update it replaces (the parity check of tests/test_sgd_fused.py).

Large-batch recipe (tests/test_sgd_lars.py): `FusedSGDTables(..., lars=...)` + `step_ex` evaluate LARS trust ratios
and the learning-rate schedule on the device from an int64 step counter, so a captured step follows both with no
host write between replays; `scheduled_lr` is the schedule's Python twin and `lars_reference_` the same update from
stock torch ops (CPU runs, eager steps, the parity checks)."""
from __future__ import annotations

import ctypes
import functools
import math

import torch

from . import _lib
from ._lib import F32, I32, I64, VP, check, ptr, sig, stream_handle

F64 = ctypes.c_double
SCHEDULES = ("constant", "cosine", "poly")


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("sgd")
    return {"chunk": sig(lib, "mifx_sgd_chunk_size", []),
            "run": sig(lib, "mifx_sgd_chunks", [VP, VP, VP, VP, VP, VP, VP, I32, VP, F32, F32, I32, VP]),
            "run_ex": sig(lib, "mifx_sgd_step_ex", [VP, VP, VP, VP, VP, VP, VP, I32, VP, VP, I32, VP, VP, VP, VP, VP,
                                                    VP, I32, I64, I64, F64, F64, F64, F64, I32, F32, F32, I32, VP])}


def scheduled_lr(kind: str, base: float, warmup: int, total: int | None, end: float, t: int) -> float:
    """Learning rate of the update that follows `t` completed ones, in double (the twin of lr_at in csrc/sgd.hip,
    operation for operation). Every kind starts with the linear warmup base * min(1, (t + 1) / max(1, warmup));
    "constant" keeps that rule forever, "cosine" and "poly" (power 2) decay from base at t = warmup to `end` at
    t = total and stay there."""
    if kind not in SCHEDULES:
        raise ValueError(f"lr schedule must be one of {SCHEDULES}, got {kind!r}")
    base, end, warmup, t = float(base), float(end), int(warmup), int(t)
    if base < 0 or end < 0 or warmup < 0 or t < 0 or (total is not None and int(total) < 0):
        raise ValueError("lr schedule: base, end, warmup, total and t must be non-negative")
    if kind != "constant" and (total is None or int(total) <= warmup):
        raise ValueError(f'lr schedule "{kind}" needs total > warmup, got total={total} warmup={warmup}')
    if kind == "constant" or t < warmup:
        return base * min(1.0, (t + 1) / max(1, warmup))
    total = int(total)
    if t >= total:
        return end
    x = (t - warmup) / (total - warmup)
    if kind == "cosine":
        return end + (base - end) * 0.5 * (1.0 + math.cos(math.pi * x))
    q = 1.0 - x
    return end + (base - end) * (q * q)


def _check_schedule(schedule) -> tuple:
    kind, base, warmup, total, end = schedule
    scheduled_lr(kind, base, warmup, total, end, 0)  # raises on an invalid combination
    return SCHEDULES.index(kind), float(base), int(warmup), int(total or 0), float(end)


def _dense(t: torch.Tensor) -> bool:
    """Non-overlapping and dense: the strides, sorted, are the running products of the sizes (any dim order)."""
    expect = 1
    for st, sz in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1):
        if st != expect:
            return False
        expect *= sz
    return True


class FusedSGDTables:
    """Device tables for one fused update of `params` (fp32, CUDA) with their momentum `bufs` and a per-tensor
    weight decay; the gradients' addresses are set per step (`set_grads`). The tables hold raw addresses: rebuild
    them (`matches`) when a parameter or momentum buffer is reallocated.

    lars = dict(eta=0.001, eps=1e-8, clip=False, adapt=[bool per tensor]) adds the per-tensor tables of `step_ex`:
    tensor i's gradient is scaled by the trust ratio eta ||w|| / (||g|| + wd_i ||w|| + eps) when adapt[i] (default:
    tensors with more than one dimension) and both norms are non-zero, else by exactly 1; clip=True is LARC
    clipping, min(ratio / lr_t, 1)."""

    CAPTURES = 4  # graph captures one table set can serve (each keeps its own pinned address buffer)

    def __init__(self, params, bufs, wds, grads=None, lars=None):
        dev = params[0].device
        if lars is not None:
            unknown = set(lars) - {"eta", "eps", "clip", "adapt"}
            if unknown:
                raise ValueError(f"fused SGD: unknown lars option(s) {sorted(unknown)}")
            eta, eps = float(lars.get("eta", 0.001)), float(lars.get("eps", 1e-8))
            if not (eta > 0 and math.isfinite(eta)) or not (eps >= 0 and math.isfinite(eps)):
                raise ValueError("fused SGD: lars needs eta > 0 and eps >= 0")
            adapt = lars.get("adapt")
            adapt = [p.ndim > 1 for p in params] if adapt is None else [bool(a) for a in adapt]
            if len(adapt) != len(params):
                raise ValueError("fused SGD: lars adapt needs one flag per tensor")
            if any(float(w) < 0 for w in wds):
                raise ValueError("fused SGD: lars needs non-negative weight decays")
        # the update is elementwise, so any dense layout works (channels_last convolution weights) as long as a
        # parameter, its gradient and its momentum buffer share it: element i of one is element i of the others
        for t in (*params, *bufs):
            if t.dtype != torch.float32 or not t.is_cuda or not _dense(t):
                raise ValueError("fused SGD: dense fp32 CUDA tensors only")
        for p, b in zip(params, bufs):
            if not (p.shape == b.shape and p.stride() == b.stride()):
                raise ValueError("fused SGD: param / momentum layouts differ")
        ch = int(_fns()["chunk"]())
        tp, to, tn = [], [], []
        for i, p in enumerate(params):
            for o in range(0, p.numel(), ch):
                tp.append(i)
                to.append(o)
                tn.append(min(ch, p.numel() - o))
        self.params, self.bufs = list(params), list(bufs)  # the addresses stay valid while the tables live
        self.key = tuple(t.data_ptr() for t in (*params, *bufs))
        addr = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=dev)  # noqa: E731
        self.pp, self.bp = addr(params), addr(bufs)
        self.gp = torch.zeros(len(params), dtype=torch.int64, device=dev)
        self._gp_host = torch.zeros(len(params), dtype=torch.int64).pin_memory()
        self.wd = torch.tensor([float(w) for w in wds], dtype=torch.float32, device=dev)
        self.tp, self.to, self.tn = (torch.tensor(x, dtype=torch.int32, device=dev) for x in (tp, to, tn))
        self.nblocks = len(tp)
        # step_ex: {-lr_t, lr_t} written by the finalize kernel (read by the update, kept for last_lr)
        self.lr_out = torch.zeros(2, dtype=torch.float32, device=dev)
        self.lars = None
        if lars is not None:
            # a tensor's chunks are consecutive in the tables: tensor i owns partials [first[i], first[i + 1])
            first = [0]
            for p in params:
                first.append(first[-1] + (p.numel() + ch - 1) // ch)
            self.lars = {"eta": eta, "eps": eps, "clip": bool(lars.get("clip", False)), "adapt": adapt}
            self.first = torch.tensor(first, dtype=torch.int32, device=dev)
            self.adapt = torch.tensor([int(a) for a in adapt], dtype=torch.int32, device=dev)
            self.pw = torch.zeros(self.nblocks, dtype=torch.float32, device=dev)
            self.pg = torch.zeros(self.nblocks, dtype=torch.float32, device=dev)
            self.ratio = torch.ones(len(params), dtype=torch.float32, device=dev)
            self.norms = torch.zeros(len(params), 2, dtype=torch.float32, device=dev)
        self._stepped_ex = False
        self.grads = None
        self._captured_hosts: list = []
        self._spare_hosts = [torch.zeros(len(params), dtype=torch.int64).pin_memory() for _ in range(self.CAPTURES)]
        if grads is not None:
            self.set_grads(grads)

    def matches(self, params, bufs) -> bool:
        return self.key == tuple(t.data_ptr() for t in (*params, *bufs))

    def grads_ok(self, grads) -> bool:
        return len(grads) == len(self.params) and all(
            g is not None and g.dtype == torch.float32 and g.shape == p.shape and g.stride() == p.stride()
            for g, p in zip(grads, self.params))

    def set_grads(self, grads) -> None:
        """Point the update at this step's gradient tensors: a pinned-host -> device copy of their addresses,
        so inside a capture it becomes a graph node (gradients produced in the graph's private pool keep their
        addresses on every replay)."""
        if not self.grads_ok(grads):
            raise ValueError("fused SGD: gradient layouts differ from their parameters'")
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            # the copy node re-reads its host buffer on every replay: give each capture a buffer of its own (pinned
            # ahead of time: no host allocation inside a capture), never written again, so a later set_grads cannot
            # retarget a captured graph
            if not self._spare_hosts:
                raise RuntimeError("fused SGD: more captures than reserved address buffers; rebuild the tables")
            host = self._spare_hosts.pop()
            self._captured_hosts.append(host)
        else:  # eager: the pinned buffer may still feed an earlier asynchronous copy
            torch.cuda.current_stream(self.gp.device).synchronize()
            host = self._gp_host
        for i, g in enumerate(grads):
            host[i] = g.data_ptr()
        self.gp.copy_(host, non_blocking=True)
        self.grads = list(grads)

    def step(self, neg_lr: torch.Tensor, momentum: float, dampening: float, nesterov: bool) -> None:
        """One update. The kernel writes the parameters through raw addresses, so their version counters are bumped
        here (at call / capture time): consumers keyed on w._version (mifx.ops.weight_prep bf16 images) then see
        the weights as changed instead of serving images from before the update."""
        if self.grads is None:
            raise RuntimeError("fused SGD: set_grads() before step()")
        check(_fns()["run"](ptr(self.pp), ptr(self.gp), ptr(self.bp), ptr(self.wd), ptr(self.tp), ptr(self.to),
                            ptr(self.tn), self.nblocks, ptr(neg_lr), float(momentum), float(dampening),
                            int(bool(nesterov)), stream_handle(neg_lr.device)), "mifx_sgd_chunks")
        torch.autograd.graph.increment_version(self.params)

    def step_ex(self, step_dev: torch.Tensor, schedule, momentum: float, dampening: float, nesterov: bool) -> None:
        """One update with the recipe evaluated on the device, so a captured step replays it: the learning rate is
        `scheduled_lr(*schedule, t)` with schedule = (kind, base, warmup, total, end) and t = step_dev[0] (int64
        device tensor: updates completed so far; read, not advanced), and with `lars` the gradients are scaled by
        their tensors' trust ratios. Launches the norm pass, the finalize and the extended update on the current
        stream; bumps the parameters' versions as `step` does."""
        if self.grads is None:
            raise RuntimeError("fused SGD: set_grads() before step_ex()")
        if step_dev.dtype != torch.int64 or step_dev.device != self.pp.device or step_dev.numel() < 1:
            raise ValueError("fused SGD: step_dev must be an int64 tensor on the parameters' device")
        kind, base, warmup, total, end = _check_schedule(schedule)
        L = self.lars
        tabs = (self.first, self.adapt, self.pw, self.pg, self.ratio, self.norms) if L else (None,) * 6
        check(_fns()["run_ex"](ptr(self.pp), ptr(self.gp), ptr(self.bp), ptr(self.wd), ptr(self.tp), ptr(self.to),
                               ptr(self.tn), self.nblocks, ptr(tabs[0]), ptr(tabs[1]), len(self.params),
                               ptr(tabs[2]), ptr(tabs[3]), ptr(tabs[4]), ptr(tabs[5]), ptr(step_dev),
                               ptr(self.lr_out), kind, warmup, total, base, end, L["eta"] if L else 0.0,
                               L["eps"] if L else 0.0, int(L["clip"]) if L else 0, float(momentum), float(dampening),
                               int(bool(nesterov)), stream_handle(step_dev.device)), "mifx_sgd_step_ex")
        torch.autograd.graph.increment_version(self.params)
        self._stepped_ex = True

    def last_lr(self) -> float | None:
        """The learning rate the last `step_ex` (or replay of a graph that holds one) used; None before any."""
        return float(self.lr_out[1]) if self._stepped_ex else None

    def last_trust_ratios(self) -> torch.Tensor | None:
        """[P] fp32 (CPU) trust ratios of the last `step_ex`; None without `lars` or before any."""
        return self.ratio.cpu() if self.lars and self._stepped_ex else None

    def last_norms(self) -> torch.Tensor | None:
        """[P, 2] fp32 (CPU) {||w||, ||g||} of the last `step_ex`; None without `lars` or before any."""
        return self.norms.cpu() if self.lars and self._stepped_ex else None


@torch.no_grad()
def lars_reference_(params, grads, bufs, wds, adapt, eta: float, eps: float, clip: bool, momentum: float,
                    dampening: float, nesterov: bool, lr) -> list:
    """The update of `FusedSGDTables.step_ex` from stock torch ops, in the tensors' own device and dtype:
    g' = (g + wd w) * r with r = eta ||w|| / (||g|| + wd ||w|| + eps) for an adapted tensor with non-zero norms
    (clip: min(r / lr, 1)), else 1; then `sgd_reference_` with wd = 0 on g'. `lr` is a float or a 0-dim tensor
    (no host synchronisation, so it captures). Returns the ratios, one 0-dim tensor per parameter."""
    scaled, ratios = [], []
    p0 = params[0]  # (one dtype and device for the whole list)
    lr_t = lr.to(p0.dtype) if isinstance(lr, torch.Tensor) else torch.tensor(float(lr), dtype=p0.dtype,
                                                                              device=p0.device)
    for p, g, wd, a in zip(params, grads, wds, adapt):
        gg = g.add(p, alpha=wd) if wd else g
        r = torch.ones((), dtype=p.dtype, device=p.device)
        if a:
            wn, gn = torch.linalg.vector_norm(p), torch.linalg.vector_norm(g)
            q = eta * wn / (gn + wd * wn + eps)
            if clip:
                q = torch.clamp(q / lr_t, max=1.0)
            r = torch.where((wn != 0) & (gn != 0), q, r)
            gg = gg * r
        scaled.append(gg)
        ratios.append(r)
    sgd_reference_(list(params), scaled, list(bufs), 0.0, momentum, dampening, nesterov, -lr_t)
    return ratios


@torch.no_grad()
def sgd_reference_(params, grads, bufs, wd: float, momentum: float, dampening: float, nesterov: bool,
                   neg_lr: torch.Tensor) -> None:
    """torch.optim.SGD's foreach update with the learning rate as a device tensor (-lr)."""
    if wd:
        grads = torch._foreach_add(grads, params, alpha=wd)
    torch._foreach_mul_(bufs, momentum)
    torch._foreach_add_(bufs, grads, alpha=1 - dampening)
    upd = torch._foreach_add(grads, bufs, alpha=momentum) if nesterov else [b.clone() for b in bufs]
    torch._foreach_mul_(upd, neg_lr)
    torch._foreach_add_(params, upd)
