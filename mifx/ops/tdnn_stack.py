"""ctypes bindings for csrc/tdnn_stack.hip (KFP taxi DNN with hidden layers H1..HL, L > 1: exact-f32 MFMA layers
2..L, their head and the fused weight-gradient + Adagrad) and for the first-layer entry points of csrc/embag_mlp.hip
that a stack runs (gather forward, sparse-row / dense-row / b1 Adagrad)."""
from __future__ import annotations

import ctypes
import functools

import torch

from . import _lib
from ._lib import F32, I32, I64, U64, VP, check, ptr, sig, stream_handle
from .embag_mlp import _feed
from .embag_mlp import _fns as _l1_chunks


@functools.lru_cache(maxsize=None)
def _fns():
    lib = _lib.load("tdnn_stack")
    l1 = _lib.load("embag_mlp")
    return {
        "limits": sig(lib, "mifx_tdnn_stack_limits", [VP]),
        "fwd": sig(lib, "mifx_tdnn_stack_fwd", [I32, VP, I32, VP, VP, VP, VP]),
        "head": sig(lib, "mifx_tdnn_stack_head", [VP, VP, VP, VP, VP, VP, I64, VP, I64, I32, I32, F32, I32, F32, VP, VP,
                                                  VP, VP, I64, I64, U64, VP]),
        "bwd": sig(lib, "mifx_tdnn_stack_bwd", [I32, VP, I32, VP, VP, VP, VP, VP, VP, F32, VP]),
        "l1_fwd": sig(l1, "mifx_tdnn_l1_fwd", [VP, VP, VP, I32, VP, I32, I32, I64, VP, I64, I32, I32, VP, I64, I64, U64,
                                               VP]),
        "l1_adagrad": sig(l1, "mifx_tdnn_l1_adagrad", [VP, VP, VP, VP, VP, I32, VP, I32, I32, I64, VP, I64, VP, I32,
                                                       I32, F32, VP, I64, I64, U64, VP]),
    }


def limits() -> dict:
    out = (ctypes.c_int * 3)()
    _fns()["limits"](out)
    return {"max_layers": out[0], "max_hidden": out[1], "max_batch": out[2]}


def validate(hidden_units, batch: int) -> None:
    """ValueError for a stack or batch outside the kernels' limits (nothing is launched)."""
    lim = limits()
    units = [int(h) for h in hidden_units]
    if not 1 <= len(units) <= lim["max_layers"]:
        raise ValueError(f"{len(units)} hidden layers: csrc/tdnn_stack.hip takes 1..{lim['max_layers']}")
    if min(units) < 1 or max(units) > lim["max_hidden"]:
        raise ValueError(f"hidden_units {units}: every width must be in [1, {lim['max_hidden']}]")
    if not 1 <= int(batch) <= lim["max_batch"]:
        raise ValueError(f"batch {batch}: csrc/tdnn_stack.hip takes 1..{lim['max_batch']}")


def _ptrs(ts):
    return (ctypes.c_void_p * max(1, len(ts)))(*[t.data_ptr() for t in ts])


class Stack:
    """The tensors of one model + batch size, laid out for the entry points: parameters and accumulators (training
    only), per-layer activation / gradient buffers, and the host arrays of device pointers the launches read."""

    def __init__(self, params: dict, accs: dict | None, hidden_units, batch: int, D: int, device):
        validate(hidden_units, batch)
        self.units = [int(h) for h in hidden_units]
        self.L, self.B, self.D = len(self.units), int(batch), int(D)
        self.widths = (ctypes.c_int * self.L)(*self.units)
        self.p, self.acc = params, accs
        self.Wh = [params[f"Wh.{k}"] for k in range(self.L - 1)]
        self.bh = [params[f"bh.{k}"] for k in range(self.L - 1)]
        self.act = [torch.empty(batch, h, device=device) for h in self.units]
        self._act, self._Wh, self._bh = _ptrs(self.act), _ptrs(self.Wh), _ptrs(self.bh)
        self.logit = torch.empty(batch, device=device)
        if accs is not None:
            self.dz = [torch.empty(batch, h, device=device) for h in self.units]
            self.dlogit = torch.empty(batch, device=device)
            self.loss = torch.empty(batch, device=device)
            self.dpart = torch.empty(_l1_chunks()["chunks"](batch) * (D + 2) * self.units[0], device=device)
            self._dz = _ptrs(self.dz)
            self._accWh = _ptrs([accs[f"Wh.{k}"] for k in range(self.L - 1)])
            self._accbh = _ptrs([accs[f"bh.{k}"] for k in range(self.L - 1)])


def forward(s: Stack, rows, xd, dense_row0: int, step_ctr=None, start: int = 0, feed=None) -> None:
    """Every forward of the step (record selection as embag_mlp.fwd_bwd): fills s.act."""
    n, F = rows.shape
    st = stream_handle(rows.device)
    p = s.p
    check(_fns()["l1_fwd"](ptr(p["W1"]), ptr(p["b1"]), ptr(rows), F, ptr(xd), s.D, dense_row0, n, ptr(step_ctr),
                           int(start), s.B, s.units[0], ptr(s.act[0]), *_feed(feed, s.B), st), "mifx_tdnn_l1_fwd")
    check(_fns()["fwd"](s.L, s.widths, s.B, s._act, s._Wh, s._bh, st), "mifx_tdnn_stack_fwd")


def logits(s: Stack, rows, xd, dense_row0: int) -> torch.Tensor:
    """Forward only over the B = len(rows) examples given: s.logit."""
    forward(s, rows, xd, dense_row0)
    p = s.p
    check(_fns()["head"](ptr(s.act[-1]), ptr(p["w2"]), None, ptr(p["b2"]), None, None, s.B, None, 0, s.B, s.units[-1],
                         1.0, 0, 0.0, None, ptr(s.logit), None, None, s.B, 0, 0, stream_handle(rows.device)),
          "mifx_tdnn_stack_head")
    return s.logit


def train_step(s: Stack, rows, xd, y, dense_row0: int, grad_scale: float, lr: float, step_ctr, feed) -> None:
    """One training step on one stream, no host work: every forward; the head (loss, dz_L, w2 / b2 update); for
    k = L..2 the input gradient of layer k, then its fused weight-gradient + Adagrad; the first layer's sparse-row
    and dense-row / b1 updates, whose last launch advances `step_ctr` once."""
    n, F = rows.shape
    st = stream_handle(rows.device)
    p, a = s.p, s.acc
    fd = _feed(feed, s.B)
    forward(s, rows, xd, dense_row0, step_ctr=step_ctr, feed=feed)
    check(_fns()["head"](ptr(s.act[-1]), ptr(p["w2"]), ptr(a["w2"]), ptr(p["b2"]), ptr(a["b2"]), ptr(y), n,
                         ptr(step_ctr), 0, s.B, s.units[-1], float(grad_scale), 1, float(lr), ptr(s.dz[-1]),
                         ptr(s.logit), ptr(s.dlogit), ptr(s.loss), *fd, st), "mifx_tdnn_stack_head")
    check(_fns()["bwd"](s.L, s.widths, s.B, s._act, s._dz, s._Wh, s._accWh, s._bh, s._accbh, float(lr), st),
          "mifx_tdnn_stack_bwd")
    check(_fns()["l1_adagrad"](ptr(p["W1"]), ptr(a["W1"]), ptr(p["b1"]), ptr(a["b1"]), ptr(rows), F, ptr(xd), s.D,
                               dense_row0, n, ptr(step_ctr), 0, ptr(s.dz[0]), s.B, s.units[0], float(lr),
                               ptr(s.dpart), *fd, st), "mifx_tdnn_l1_adagrad")
