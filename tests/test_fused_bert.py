"""csrc/fused_bert.hip against a float64 reference, per row, per 16 columns and per workgroup.

Every kernel of the file (fused bias + dropout + residual + LayerNorm forward and backward with the col_reduce_y
tail, bias + GELU forward and backward, standalone dropout, the col_sum bias gradients, the deterministic embedding
gradient) is compared with `_ref64`: the operation written from its definition in float64 on the inputs as the
kernel reads them (bf16 inputs are bf16-rounded), gradients by autograd, the dropout mask from fb.keep_mask sliced
by eoff. The yardstick of the bound is `_emulate`: the same computation in float32 with the kernels' rounding points
(outputs to the activation dtype, parameter gradients to the parameter dtype, dbias and the GELU db summed over the
rounded stored values; x_hat, mean and rstd stay fp32). Every reduction of the emulation, the column sums over rows
and the row sums of the LayerNorm statistics alike, is SEQUENTIAL in fp32, in index order: the least accurate order
a correct kernel could use. With E the emulation's error against `_ref64`, a kernel must stay within

    err_unit <= MARGIN * E_unit + FLOOR

for every unit of every output. A unit is one row for row outputs (y, dr, da, GELU y / dx: one wave's work in the
LayerNorm kernels), 16 consecutive columns for column outputs (dw, db, dbias, GELU db, col_sum, each embedding row:
one col_reduce block), 4 consecutive rows for mean / rstd (one workgroup). err is the unit's L2 error over the unit's
L2 norm in the reference. E is computed here from the emulation, never from a kernel. FLOOR is one extra rounding of
the output type: 2^-9 for bf16, 2^-24 for fp32. A unit whose reference norm is zero or below TINY = 1e-6 of the
output's largest unit (an embedding row no token uses) is compared absolutely, against the largest unit's norm:
below that, fp32 partial sums at the scale of the large units no longer resolve the unit. No case, unit or element
is left out.

The LayerNorm has two emulations, and E is the larger of their errors, unit by unit. The second one is the first
with its mean and rstd replaced by the exact ones moved by one standard deviation of the sequential sum's error
(`_ln_stat_sigma`, from the partial sums of the float64 reference). The reason: a row's mean is ONE number whose
error is one draw of a rounding noise, and on rows whose mean is far above their spread (the mean-100 family: s near
100, ulp 7.6e-6, spread 1.4) that one draw, passed on by s - mean, is the whole error of the row's y, dr and da too.
One draw says nothing about the next: measured with the first emulation alone, the H = 100, R = 1 row's mean needed
17.8 (the sequential sum happened to land 18 times closer than the kernel, whose error was one rounding of a
partial sum of size 8), and y / dr / da of the mean-100 rows with fp32 activations needed 3.1 .. 4.7 at H = 100 and
3.6 at H = 256 (kernel errors of 4e-6 .. 8e-6: half an ulp of the stored fp32 mean over the spread; the sequential
emulation's own rows range from 1.2e-6 to 6e-5). No other unit of any output needed more than 2.9. With the
expected size of the draw in E these units need 0.6 .. 1.7, and the one-pass-variance and padded-width mutants
below still fail at MARGIN + 1 by a wide factor.

MARGIN = 3. Measured on an MI355X over every case of this file, the margin a kernel needs, max over units of
(err - FLOOR) / E:

    LayerNorm      y     mean  rstd  dr    da    dw    db    dbias
    vector NC 1-4  0.60  0.81  0.61  0.56  0.60  0.77  0.68  1.07
    scalar PER     1.73  1.70  0.98  1.50  1.69  1.12  0.93  1.07

    bias + GELU    y     dx    db          col_sum 1.00    embedding 1.54
    vector VW 4/8  1.14  1.85  1.03        identities: db (LayerNorm and GELU) 0.95, dbias 1.16
    scalar         0.24  0.11  1.00

(MIFX_BERT_LN_RPW = 1 and 16 included.) Every worst value comes from an fp32 output, where FLOOR is 6e-8 and E is a
few 1e-8 .. 1e-7: the bf16 outputs need at most 0.69, as both sides round nearly the same fp32 value. The scalar
LayerNorm's 1.5 .. 1.7 are the worst of the 16389 rows of H = 64, where a row's E is the noise of 64 elements, and
a mean at H = 100; the GELU's 1.85 is a row of 8 fp32 elements (M 1025, N 8), device erff / expf against the
host's. The column sums (blocked in the kernels, sequential here) stay near 1, the embedding's 1.54 being one
16-column unit of the scalar path at H = 2048.
2 would leave 1.08x over the worst 1.85, so 3 it is: 1.62x. No family needs more than 4, and the tests found no bug
in csrc/fused_bert.hip or mifx/ops/fused_bert.py. The CPU tests below hold the margin honest: the unmodified
emulation with torch's blocked reductions passes at MARGIN, and eight wrong variants (one-pass variance, statistics
over the lane-padded width, bias added after the dropout scale, a mask drawn without eoff, dw / db without the last
row, tanh GELU, GELU db without a chunk's last M % 4 rows, an embedding id without its last partial chunk) all
exceed the bound at MARGIN + 1 on cases the GPU tests run.
"""
import functools
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from mifx.ops import fused_bert as fb

F32, BF16 = torch.float32, torch.bfloat16
FLOOR = {F32: 2.0 ** -24, BF16: 2.0 ** -9}
MARGIN = 3
TINY = 1e-6
EPS = 1e-5  # large enough to matter on the rows of scale 1e-3 (variance 1e-6)
SEED_CTR, SITE, P = (1234, 7), 11, 0.1
EOFF_ROWS = 5  # every dropout case is a shard that starts at row 5 of a larger activation: eoff = 5 H
VARIANTS = {"plain": (False, 0.0), "bias": (True, 0.0), "drop": (False, P), "biasdrop": (True, P)}


def _rng_cpu():
    return torch.tensor(SEED_CTR, dtype=torch.int64)


def _rt(x, dt):
    """x rounded to dt, as float32."""
    return x.to(dt).float()


def _seq_sum(x, dim):
    """Sum over dim, sequentially in index order, every partial sum rounded to float32."""
    xt = x.float().movedim(dim, 0).contiguous()
    acc = torch.zeros_like(xt[0])
    for i in range(xt.shape[0]):
        acc += xt[i]
    return acc


def _sum(x, dim, seq):
    return _seq_sum(x, dim) if seq else x.float().sum(dim)


# ---- metric and bound -------------------------------------------------------------------------------------------
def _unit_norms(x, unit):
    """L2 norms of the units of x, float64. unit "row": x [R, C], one per row. "col": x [A, C] or [C], 16
    consecutive columns of each row (the last group of a ragged C is shorter). "stat": x [R], 4 consecutive rows."""
    x = x.double()
    if unit == "row":
        return x.reshape(x.shape[0], -1).pow(2).sum(-1).sqrt()
    g = 16 if unit == "col" else 4
    x = x.reshape(-1, x.shape[-1])
    pad = (-x.shape[-1]) % g
    if pad:
        x = torch.cat([x, x.new_zeros(x.shape[0], pad)], -1)
    return x.reshape(x.shape[0], -1, g).pow(2).sum(-1).sqrt()


def _unit_rel(diff, ref, unit):
    """Per-unit L2 norm of diff relative to the reference unit's norm; zero and tiny units (below TINY of the
    largest) absolutely, against the largest unit's norm."""
    n = _unit_norms(ref, unit)
    top = n.max()
    den = torch.where(n >= TINY * top, n, top)
    den = torch.where(den > 0, den, torch.ones_like(den))
    return _unit_norms(diff, unit) / den


def _unit_err(got, ref, unit):
    return _unit_rel(got.double() - ref.double(), ref, unit)


def _yardstick(emu, ref, unit):
    """E per unit: the emulation's error against the reference; the largest of them where emu is a list of
    emulations (the LayerNorm's two, see _ln_case)."""
    emus = emu if isinstance(emu, (list, tuple)) else [emu]
    return torch.stack([_unit_err(e, ref, unit) for e in emus]).amax(0)


def _excess(got, emu, ref, unit, floor, margin=MARGIN):
    """max over units of err - (margin E + FLOOR): positive means outside the bound."""
    return float((_unit_err(got, ref, unit) - (margin * _yardstick(emu, ref, unit) + floor)).max())


def _assert_within(tag, family, got, emu, ref, spec):
    """got, ref: dicts of outputs; emu: such a dict or a list of them; spec: name -> (unit, output dtype). Prints
    the measured ratios, then asserts the bound for every unit of every output."""
    emus = emu if isinstance(emu, (list, tuple)) else [emu]
    bad = []
    for name, (unit, dt) in spec.items():
        if ref[name] is None:
            continue
        assert bool(torch.isfinite(got[name].float()).all()), f"{tag}: {name} is not finite"
        fl = FLOOR[dt]
        err = _unit_err(got[name], ref[name], unit)
        e = _yardstick([m[name] for m in emus], ref[name], unit)
        need = float(((err - fl).clamp(min=0) / e.clamp(min=1e-300)).max()) if bool((err > fl).any()) else 0.0
        print(f"FB_RATIO family={family} out={name} dt={'bf16' if dt == BF16 else 'f32'} need={need:.3f} "
              f"maxerr={float(err.max()):.3e} maxE={float(e.max()):.3e} case={tag}")
        if not bool((err <= MARGIN * e + fl).all()):
            i = int((err - MARGIN * e).argmax())
            bad.append(f"{name}: unit {i} of {err.numel()} err {float(err.flatten()[i]):.4g} > {MARGIN} * "
                       f"{float(e.flatten()[i]):.4g} + {fl:.4g} (needs margin {need:.2f})")
    assert not bad, f"{tag}: " + "; ".join(bad)


# ---- LayerNorm: inputs, reference, emulation ----------------------------------------------------------------------
def LN_SPEC(adt, pdt):
    return {"y": ("row", adt), "mean": ("stat", F32), "rstd": ("stat", F32), "dr": ("row", adt), "da": ("row", adt),
            "dw": ("col", pdt), "db": ("col", pdt), "dbias": ("col", pdt)}


def _ln_path(H, off):
    return "ln_vec" if H % 256 == 0 and H // 256 <= 4 and not off else "ln_scalar"


@functools.lru_cache(maxsize=6)
def _ln_case(H, R, adt, pdt, variant, family="randn", off=False):
    """Inputs in the dtypes the kernel reads them in, the keep mask, `_ref64` and `_emulate` of one LayerNorm
    case. off: `a` lives one element into its buffer (the alignment fallback). Families: randn; mean100 (rows of
    mean 100 and unit variance); scales (row i scaled by 10^(-3 .. 3)); gamma (a third of gamma zero, a third
    negative)."""
    has_bias, p = VARIANTS[variant]
    g = torch.Generator().manual_seed(100003 * H + 17 * R + len(family) + 5 * len(variant))
    a, r, dy = (torch.randn(R, H, generator=g) for _ in range(3))
    if family == "mean100":
        r = r + 100.0
    elif family == "scales":
        s = torch.logspace(-3, 3, R)[:, None]
        a, r = a * s, r * s
    w = 1.0 + 0.5 * torch.randn(H, generator=g)
    b = 0.5 * torch.randn(H, generator=g)
    bias = 0.5 * torch.randn(H, generator=g).to(pdt) if has_bias else None
    if family == "gamma":
        w[0::3] = 0.0
        w[1::3] = -w[1::3].abs() - 0.1
    c = types.SimpleNamespace(H=H, R=R, adt=adt, pdt=pdt, variant=variant, family=family, off=off, p=p,
                              a=a.to(adt), r=r.to(adt), dy=dy.to(adt), w=w.to(pdt), b=b.to(pdt), bias=bias,
                              eoff=EOFF_ROWS * H if p > 0 else 0)
    c.keep = fb.keep_mask(c.eoff + R * H, _rng_cpu(), SITE, p)[c.eoff:].view(R, H) if p > 0 else None
    c.ref, sigma = _ln_ref64(c)
    c.emu = [_ln_emulate(c, c.keep),
             _ln_emulate(c, c.keep, stats={n: (c.ref[n] + sigma[n]).float()[:, None] for n in ("mean", "rstd")})]
    c.tag = (f"H{H}{'off' if off else ''}/R{R}/{'bf16' if adt == BF16 else 'f32'}.{'bf16' if pdt == BF16 else 'f32'}"
             f"/{variant}/{family}")
    return c


def _ln_ref64(c):
    a, r, w, b = (t.double().requires_grad_() for t in (c.a, c.r, c.w, c.b))
    bias = None if c.bias is None else c.bias.double().requires_grad_()
    x = a if bias is None else a + bias
    if c.p > 0:
        x = x * (c.keep.double() * fb._drop_scale(c.p))
    s = x + r
    mean = s.mean(-1, keepdim=True)
    var = (s - mean).pow(2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    y = (s - mean) * rstd * w + b
    y.backward(c.dy.double())
    return {"y": y.detach(), "mean": mean.detach().squeeze(-1), "rstd": rstd.detach().squeeze(-1), "dr": r.grad,
            "da": a.grad, "dw": w.grad, "db": b.grad,
            "dbias": None if bias is None else bias.grad}, _ln_stat_sigma(s.detach(), mean.detach(), rstd.detach())


def _ln_stat_sigma(s, mean, rstd):
    """The standard deviation of the error of mean and rstd under the emulation's sequential fp32 sums, per row.
    The k-th addition rounds a partial sum S_k: an error uniform within half an ulp of S_k, of standard deviation at
    most 2^-24 |S_k| / sqrt(3); the sum's is the root of their squares, and rstd = (var + eps)^-1/2 passes the
    variance's on with the factor rstd^3 / 2."""
    u = 2.0 ** -24 / math.sqrt(3.0)
    H = s.shape[-1]
    sig_mean = u * s.cumsum(-1).pow(2).sum(-1).sqrt() / H
    sig_var = u * (s - mean).pow(2).cumsum(-1).pow(2).sum(-1).sqrt() / H
    return {"mean": sig_mean, "rstd": 0.5 * rstd.squeeze(-1).pow(3) * sig_var}


def _ln_emulate(c, keep, seq=True, mutant=None, stats=None):
    """The fused LayerNorm in float32 with the kernels' rounding points. seq: sequential reductions (the
    yardstick) or torch's blocked ones. mutant: one of the wrong variants of the sensitivity tests. stats: mean and
    rstd [R, 1] to use in place of the computed ones."""
    H, R = c.H, c.R
    a, r, dy, w, b = (t.float() for t in (c.a, c.r, c.dy, c.w, c.b))
    sc = fb._drop_scale(c.p) if c.p > 0 else 1.0
    x = a if c.bias is None else a + c.bias.float()
    x = x * sc
    if mutant == "bias_after_scale" and c.bias is not None:
        x = a * sc + c.bias.float()
    if c.p > 0:
        x = torch.where(keep, x, torch.zeros(()))
    s = x + r
    width = 64 * ((H + 63) // 64) if mutant == "padded_width" else H
    mean = (_sum(s, -1, seq) / width)[:, None]
    if mutant == "onepass_var":
        var = _sum(s * s, -1, seq)[:, None] / width - mean * mean
    else:
        d = s - mean
        var = _sum(d * d, -1, seq)[:, None] / width
    rstd = 1.0 / torch.sqrt(var + EPS)
    if stats is not None:
        mean, rstd = stats["mean"], stats["rstd"]
    xh = (s - mean) * rstd
    y = _rt(xh * w + b, c.adt)
    g = dy * w
    mg = (_sum(g, -1, seq) / width)[:, None]
    mgx = (_sum(g * xh, -1, seq) / width)[:, None]
    o = rstd * (g - mg - xh * mgx)
    oa = o * sc if c.p == 0 else torch.where(keep, o * sc, torch.zeros(()))
    da = _rt(oa, c.adt)
    rows = slice(0, R - 1) if mutant == "drop_last_row" and R % 4 != 0 else slice(0, R)
    dw = _rt(_sum((dy * xh)[rows], 0, seq), c.pdt)
    db = _rt(_sum(dy[rows], 0, seq), c.pdt)
    dbias = None if c.bias is None else _rt(_sum(da, 0, seq), c.pdt)
    return {"y": y, "mean": mean.squeeze(-1), "rstd": rstd.squeeze(-1), "dr": _rt(o, c.adt), "da": da, "dw": dw,
            "db": db, "dbias": dbias}


def _ln_excess(c, got, margin, names=None):
    spec = LN_SPEC(c.adt, c.pdt)
    return {n: _excess(got[n], [m[n] for m in c.emu], c.ref[n], spec[n][0], FLOOR[spec[n][1]], margin)
            for n in (names or spec) if c.ref[n] is not None}


# H -> instantiation; "768off": `a` one element into its buffer, so the pointer check sends H = 768 to PER 12
LN_H = [(64, False), (100, False), (256, False), (320, False), (512, False), (768, False), (768, True), (1000, False),
        (1024, False), (1280, False), (4096, False)]
PAIRS = {"f32.f32": (F32, F32), "bf16.f32": (BF16, F32), "bf16.bf16": (BF16, BF16), "f32.bf16": (F32, BF16)}


def _ln_cases():
    seen = set()

    def add(H, off, R, pair, variant, family="randn"):
        key = (H, R, *PAIRS[pair], variant, family, off)
        if key not in seen:
            seen.add(key)
            out.append(pytest.param(*key, id=f"H{H}{'off' if off else ''}-R{R}-{pair}-{variant}-{family}"))

    out = []
    for H, off in LN_H:
        for R in (1, 3, 37):
            pairs = PAIRS if H in (100, 768) else ("f32.f32", "bf16.bf16")
            for pair in pairs:
                for variant in (VARIANTS if H in (100, 768) else ("plain", "biasdrop")):
                    add(H, off, R, pair, variant)
    for H in (64, 256):  # forward and backward grid-stride; 127 / 128 / 129 partial rows at 2 rows per wave
        for R in (16389, 1016, 1024, 1025):
            for pair in ("f32.f32", "bf16.bf16"):
                for variant in ("plain", "biasdrop"):
                    add(H, False, R, pair, variant)
    for family in ("mean100", "scales", "gamma"):
        for H in (100, 256, 1000, 1024):
            for pair in ("f32.f32", "bf16.bf16", "f32.bf16"):
                add(H, False, 37, pair, "biasdrop", family)
    return out


# ---- GELU -------------------------------------------------------------------------------------------------------
PLANTED = (0.0, 1e-4, -1e-4, 5.5, -5.5, 9.0, -9.0, 13.0, -13.0)


def GELU_SPEC(adt, pdt):
    return {"y": ("row", adt), "dx": ("row", adt), "db": ("col", pdt)}


def _gelu_chunks(M):
    return 1 if M < 16 else min(M // 16, 512)


def _gelu_vec(N, adt, off):
    return N % (16 // (2 if adt == BF16 else 4)) == 0 and not off


@functools.lru_cache(maxsize=4)
def _gelu_case(M, N, adt, pdt, off=False):
    """3 randn with x + bias = 0, +-1e-4, +-5.5, +-9, +-13 planted (erf saturates from |v| of about 5.5 on)."""
    g = torch.Generator().manual_seed(7919 * M + N)
    x = 3.0 * torch.randn(M, N, generator=g)
    bias = (0.1 * torch.randn(N, generator=g)).to(pdt)
    for i, v in enumerate(PLANTED[:M * N]):
        j = (i * 37) % (M * N) if M * N > 37 * len(PLANTED) else i
        x.view(-1)[j] = v - float(bias[j % N])
    dy = torch.randn(M, N, generator=g)
    c = types.SimpleNamespace(M=M, N=N, adt=adt, pdt=pdt, off=off, x=x.to(adt), bias=bias, dy=dy.to(adt))
    xx, bb = c.x.double().requires_grad_(), c.bias.double().requires_grad_()
    v = xx + bb
    y = 0.5 * v * (1.0 + torch.erf(v / math.sqrt(2.0)))
    y.backward(c.dy.double())
    c.ref = {"y": y.detach(), "dx": xx.grad, "db": bb.grad}
    c.emu = _gelu_emulate(c)
    c.tag = f"M{M}/N{N}{'off' if off else ''}/{'bf16' if adt == BF16 else 'f32'}.{'bf16' if pdt == BF16 else 'f32'}"
    return c


def _gelu_emulate(c, mutant=None):
    v = c.x.float() + c.bias.float()
    if mutant == "tanh":
        t = torch.tanh(0.7978845608028654 * (v + 0.044715 * v * v * v))
        y = 0.5 * v * (1.0 + t)
        grad = 0.5 * (1.0 + t) + 0.5 * v * (1.0 - t * t) * 0.7978845608028654 * (1.0 + 3 * 0.044715 * v * v)
    else:
        y = 0.5 * v * (1.0 + torch.erf(v * 0.70710678118654752))
        grad = 0.5 * (1.0 + torch.erf(v * 0.70710678118654752)) + v * 0.3989422804014327 * torch.exp(-0.5 * v * v)
    dx = _rt(c.dy.float() * grad, c.adt)
    part = dx
    if mutant == "chunk_tail":  # the scalar kernel's rows past the last full group of 4 of each chunk
        part, ch = dx.clone(), _gelu_chunks(c.M)
        for k in range(ch):
            r0, r1 = c.M * k // ch, c.M * (k + 1) // ch
            part[r1 - (r1 - r0) % 4:r1] = 0.0
    return {"y": _rt(y, c.adt), "dx": dx, "db": _rt(_seq_sum(part, 0), c.pdt)}


GELU_SHAPES = [(1, 8, False), (15, 520, False), (17, 512, False), (33, 12, False), (70, 3070, False), (17, 512, True),
               (1025, 8, False), (8211, 16, False)]


def _gelu_cases():
    out = []
    for M, N, off in GELU_SHAPES:
        for pair in (PAIRS if (M, N) in ((17, 512), (70, 3070)) and not off else ("f32.f32", "bf16.bf16")):
            out.append(pytest.param(M, N, *PAIRS[pair], off, id=f"M{M}-N{N}{'off' if off else ''}-{pair}"))
    return out


# ---- embedding gradient -----------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 128, 129, 700)


def _emb_ids(struct, N):
    """counts: ids 0 .. 6 occur exactly 1, 63, 64, 65, 128, 129 and 700 times, interleaved with each other and
    with single-use ids by a fixed permutation, so no chunk's occurrences are contiguous. rand: N draws from N / 3 +
    1 ids. one: a single id. two: id 1 at every third token, id 3 at the others."""
    g = torch.Generator().manual_seed(N)
    if struct == "counts":
        ids = torch.cat([torch.full((n,), i) for i, n in enumerate(COUNTS)])
        ids = torch.cat([ids, torch.arange(len(COUNTS) + 2, len(COUNTS) + 2 + N - ids.numel())])
        ids = ids[torch.randperm(N, generator=g)]
        assert [int((ids == i).sum()) for i in range(len(COUNTS))] == list(COUNTS)
        return ids, int(ids.max()) + 3
    if struct == "rand":
        V = N // 3 + 1
        return torch.randint(0, V, (N,), generator=g), V + 2
    if struct == "one":
        return torch.full((N,), 2), 4
    assert struct == "two"
    return torch.where(torch.arange(N) % 3 == 0, 1, 3), 5


@functools.lru_cache(maxsize=2)
def _emb_case(struct, N, H, ddt, wdt):
    ids, V = _emb_ids(struct, N)
    assert 0 <= int(ids.min()) and int(ids.max()) < V
    dy = torch.randn(N, H, generator=torch.Generator().manual_seed(N + H)).to(ddt)
    c = types.SimpleNamespace(struct=struct, N=N, H=H, V=V, ddt=ddt, wdt=wdt, ids=ids, dy=dy)
    c.ref = {"g": torch.zeros(V, H, dtype=torch.float64).index_add_(0, ids, dy.double())}
    c.emu = {"g": _emb_emulate(c)}
    c.tag = f"{struct}/N{N}/H{H}/{'bf16' if ddt == BF16 else 'f32'}.{'bf16' if wdt == BF16 else 'f32'}"
    return c


def _emb_emulate(c, mutant=None):
    """Every id's rows added in token order in fp32, rounded to the weight dtype. mutant "lost_tail": an id keeps
    only its full chunks of 64 occurrences (an id with fewer than 64 keeps all)."""
    g = torch.zeros(c.V, c.H)
    dy = c.dy.float()
    seen = {}
    total = {int(i): int(n) for i, n in zip(*torch.unique(c.ids, return_counts=True))}
    for n, i in enumerate(c.ids.tolist()):
        k = seen.get(i, 0)
        seen[i] = k + 1
        if mutant == "lost_tail" and total[i] > 64 and k >= total[i] - total[i] % 64:
            continue
        g[i] += dy[n]
    return _rt(g, c.wdt)


EMB_CASES = [
    # structure, N, H, dy dtype, weight dtype
    ("counts", 5000, 96, "bf16.bf16"), ("counts", 5000, 100, "f32.f32"), ("counts", 5000, 768, "bf16.f32"),
    ("counts", 5000, 8, "f32.bf16"), ("counts", 5000, 8, "f32.f32"), ("counts", 5000, 2048, "bf16.f32"),
    ("counts", 5000, 2048, "f32.f32"), ("counts", 5000, 2056, "bf16.bf16"), ("counts", 5000, 2056, "bf16.f32"),
    ("rand", 1, 96, "f32.f32"), ("rand", 255, 96, "f32.f32"), ("rand", 256, 96, "f32.f32"),
    ("rand", 257, 96, "f32.f32"), ("rand", 1, 96, "bf16.bf16"), ("rand", 255, 100, "bf16.bf16"),
    ("rand", 256, 768, "bf16.bf16"), ("rand", 257, 8, "bf16.bf16"),
    ("one", 255, 96, "f32.f32"), ("one", 256, 96, "f32.f32"), ("one", 257, 96, "bf16.f32"),
    ("one", 32768, 8, "f32.f32"), ("one", 32768, 8, "bf16.bf16"),
    ("two", 32768, 96, "f32.f32"), ("two", 32768, 96, "bf16.f32"),
    ("two", 32769, 8, "f32.f32"),  # one token too many for the kernels: the index_add_ route
]


# ---- CPU: the references are what they claim to be, and the margin is honest ----------------------------------------
def test_seq_sum_is_sequential_fp32():
    x = torch.tensor([[1.0, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -24]])
    assert float(_seq_sum(x, -1)) == 1.0  # each addend is half an ulp of the running sum: all are lost in order
    assert float(x.double().sum()) > 1.0
    y = torch.randn(257, 33, generator=torch.Generator().manual_seed(0))
    acc = np.zeros(33, dtype=np.float32)
    for row in y.numpy():
        acc = acc + row
    assert torch.equal(_seq_sum(y, 0), torch.from_numpy(acc))


def test_ref64_matches_library_references():
    """_ref64 of the LayerNorm against the package's CPU composition (F.layer_norm, the same mask and eoff), values
    and gradients; the GELU one against F.gelu."""
    c = _ln_case(100, 37, F32, F32, "biasdrop")
    a, r, w, b, bias = (t.double().requires_grad_() for t in (c.a, c.r, c.w, c.b, c.bias))
    y = fb.bias_dropout_add_layernorm(a, bias, r, w, b, EPS, c.p, _rng_cpu(), SITE, None, c.eoff)
    y.backward(c.dy.double())
    got = {"y": y.detach(), "dr": r.grad, "da": a.grad, "dw": w.grad, "db": b.grad, "dbias": bias.grad}
    for n, t in got.items():
        torch.testing.assert_close(t, c.ref[n], rtol=1e-9, atol=1e-9)
    assert 0.05 < 1 - c.keep.float().mean() < 0.15
    assert not torch.equal(c.keep, fb.keep_mask(c.R * c.H, _rng_cpu(), SITE, c.p).view(c.R, c.H))  # eoff matters
    g = _gelu_case(17, 512, F32, F32)
    x = g.x.double().requires_grad_()
    torch.nn.functional.gelu(x + g.bias.double()).backward(g.dy.double())
    torch.testing.assert_close(x.grad, g.ref["dx"], rtol=1e-10, atol=1e-12)


CPU_LN = [(100, 37, "f32.f32", "biasdrop", "randn"), (100, 37, "bf16.bf16", "biasdrop", "randn"),
          (256, 37, "f32.f32", "biasdrop", "mean100"), (1000, 37, "f32.bf16", "biasdrop", "scales"),
          (1024, 37, "bf16.bf16", "biasdrop", "gamma"), (256, 1025, "f32.f32", "biasdrop", "randn")]


@pytest.mark.parametrize("H,R,pair,variant,family", CPU_LN)
def test_ln_emulation_within_bound(H, R, pair, variant, family):
    """The unmodified emulation with torch's blocked reductions in place of the sequential ones (another order, as
    a kernel's is) stays within the bound the GPU tests use, on every input family."""
    c = _ln_case(H, R, *PAIRS[pair], variant, family)
    ex = _ln_excess(c, _ln_emulate(c, c.keep, seq=False), MARGIN)
    assert all(v <= 0 for v in ex.values()), ex


def test_other_emulations_within_bound():
    for args in ((70, 3070, F32, F32), (70, 3070, BF16, BF16), (8211, 16, F32, BF16)):
        c = _gelu_case(*args)
        blocked = dict(c.emu, db=_rt(c.emu["dx"].sum(0), c.pdt))
        for n, (unit, dt) in GELU_SPEC(c.adt, c.pdt).items():
            assert _excess(blocked[n], c.emu[n], c.ref[n], unit, FLOOR[dt]) <= 0, (args, n)
    for struct, N, H, pair in (("counts", 5000, 100, "f32.f32"), ("counts", 5000, 96, "bf16.bf16")):
        c = _emb_case(struct, N, H, *PAIRS[pair])
        blocked = _rt(torch.zeros(c.V, H).index_add_(0, c.ids, c.dy.float()), c.wdt)
        assert _excess(blocked, c.emu["g"], c.ref["g"], "col", FLOOR[c.wdt]) <= 0


def _ln_mutant_excess(case, mutant, keep=None):
    c = _ln_case(*case[:2], *PAIRS[case[2]], *case[3:])
    return _ln_excess(c, _ln_emulate(c, c.keep if keep is None else keep(c), mutant=mutant), MARGIN + 1)


def test_mutant_onepass_variance():
    """Variance as E[x^2] - mean^2: visible only with fp32 activations on the rows of mean 100 (with bf16 output
    the rounding of y hides it)."""
    ex = _ln_mutant_excess((256, 37, "f32.f32", "biasdrop", "mean100"), "onepass_var")
    assert ex["y"] > 0 and ex["rstd"] > 0 and ex["dr"] > 0, ex
    assert _ln_mutant_excess((1000, 37, "f32.bf16", "biasdrop", "mean100"), "onepass_var")["y"] > 0


@pytest.mark.parametrize("H", [100, 1000])
@pytest.mark.parametrize("pair", ["f32.f32", "bf16.bf16"])
def test_mutant_padded_width(H, pair):
    """Mean and variance over the lane-padded width 64 ceil(H / 64) instead of H."""
    ex = _ln_mutant_excess((H, 37, pair, "biasdrop", "randn"), "padded_width")
    assert all(ex[n] > 0 for n in ("y", "mean", "rstd", "dr", "da")), ex


@pytest.mark.parametrize("pair", ["f32.f32", "bf16.bf16"])
def test_mutant_bias_after_scale(pair):
    """a scale + bias instead of (a + bias) scale."""
    ex = _ln_mutant_excess((768, 37, pair, "biasdrop", "randn"), "bias_after_scale")
    assert ex["y"] > 0 and ex["dr"] > 0, ex


@pytest.mark.parametrize("H", [100, 768])
@pytest.mark.parametrize("pair", ["f32.f32", "bf16.bf16"])
def test_mutant_mask_without_eoff(H, pair):
    """The mask drawn at the shard's own indices, not at eoff + index."""
    ex = _ln_mutant_excess((H, 37, pair, "drop", "randn"), None,
                           keep=lambda c: fb.keep_mask(c.R * c.H, _rng_cpu(), SITE, c.p).view(c.R, c.H))
    assert ex["y"] > 0 and ex["da"] > 0, ex


@pytest.mark.parametrize("case", [(768, 37, "bf16.bf16", "biasdrop", "randn"), (768, 3, "f32.f32", "plain", "randn"),
                                  (64, 16389, "f32.f32", "biasdrop", "randn"),
                                  (256, 1025, "bf16.bf16", "biasdrop", "randn")], ids=str)
def test_mutant_dw_db_lose_last_row(case):
    """dw / db without the last row when R is not a multiple of 4 (a workgroup's rows)."""
    ex = _ln_mutant_excess(case, "drop_last_row")
    assert ex["dw"] > 0 and ex["db"] > 0, ex


def test_mutant_tanh_gelu():
    """tanh GELU instead of erf: outside the bound with fp32 activations (within the bf16 rounding otherwise)."""
    for M, N in ((17, 512), (70, 3070)):
        c = _gelu_case(M, N, F32, F32)
        m = _gelu_emulate(c, "tanh")
        for n in ("y", "dx"):
            assert _excess(m[n], c.emu[n], c.ref[n], "row", FLOOR[F32], MARGIN + 1) > 0, (M, N, n)


@pytest.mark.parametrize("pair", ["f32.f32", "bf16.bf16"])
def test_mutant_gelu_db_chunk_tail(pair):
    """GELU db without the final M % 4 rows of each chunk (the scalar kernel's remainder loop)."""
    c = _gelu_case(70, 3070, *PAIRS[pair])
    m = _gelu_emulate(c, "chunk_tail")
    assert _excess(m["db"], c.emu["db"], c.ref["db"], "col", FLOOR[c.pdt], MARGIN + 1) > 0


@pytest.mark.parametrize("struct,N,H,pair", [("counts", 5000, 100, "f32.f32"), ("counts", 5000, 96, "bf16.bf16"),
                                             ("one", 257, 96, "bf16.f32")])
def test_mutant_embedding_lost_tail(struct, N, H, pair):
    """An id that loses its occurrences past the last full chunk of 64."""
    c = _emb_case(struct, N, H, *PAIRS[pair])
    assert _excess(_emb_emulate(c, "lost_tail"), c.emu["g"], c.ref["g"], "col", FLOOR[c.wdt], MARGIN + 1) > 0


# ---- GPU: LayerNorm ---------------------------------------------------------------------------------------------
def _rng_gpu():
    return torch.tensor(SEED_CTR, dtype=torch.int64, device="cuda")


def _place(t, off=False):
    """t on the GPU; off: one element into a larger buffer (contiguous, so .contiguous() keeps the offset)."""
    if not off:
        return t.cuda()
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v.detach()


def _ln_run(c, r0=0, r1=None):
    """Rows [r0, r1) of the case through fb.bias_dropout_add_layernorm (forward and backward) and through the raw
    forward entry point, mirroring the wrapper, for mean and rstd. Outputs on the CPU in their own dtypes."""
    r1 = c.R if r1 is None else r1
    R, H = r1 - r0, c.H
    a = _place(c.a[r0:r1], c.off).requires_grad_()
    r, w, b = c.r[r0:r1].cuda().requires_grad_(), c.w.cuda().requires_grad_(), c.b.cuda().requires_grad_()
    bias = None if c.bias is None else c.bias.cuda().requires_grad_()
    rng = _rng_gpu() if c.p > 0 else None
    eoff = c.eoff + r0 * H
    y0 = torch.full_like(r, float("nan"))
    mean = torch.full((R,), float("nan"), device="cuda")
    rstd = torch.full_like(mean, float("nan"))
    fb.check(fb._fns()["ln_fwd2"](fb._dt(a), fb._dt(w), fb.ptr(a), fb.ptr(bias), fb.ptr(r), fb.ptr(w), fb.ptr(b), R, H,
                                  EPS, c.p, fb.ptr(rng), SITE, eoff, fb.ptr(y0), fb.ptr(mean), fb.ptr(rstd),
                                  fb.stream_handle(a.device)), "mifx_bert_bdaln_fwd2")
    y = fb.bias_dropout_add_layernorm(a, bias, r, w, b, EPS, c.p, rng, SITE, None, eoff)
    y.backward(c.dy[r0:r1].cuda())
    assert torch.equal(y, y0)
    got = {"y": y.detach(), "mean": mean, "rstd": rstd, "dr": r.grad, "da": a.grad, "dw": w.grad, "db": b.grad,
           "dbias": None if bias is None else bias.grad}
    assert got["dw"].dtype == c.pdt and got["da"].dtype == c.adt
    return {n: None if t is None else t.cpu() for n, t in got.items()}


def _ln_identities(c, got):
    """dbias against the float64 column sum of the kernel's own stored da, db against that of dy: the yardstick is
    the sequential fp32 sum of the same addends alone."""
    pairs = [("db", c.dy)] + ([("dbias", got["da"])] if c.bias is not None else [])
    for name, addends in pairs:
        ref = {name: addends.double().sum(0)}
        emu = {name: _rt(_seq_sum(addends, 0), c.pdt)}
        _assert_within(c.tag + "/identity", "identity", got, emu, ref, {name: ("col", c.pdt)})


@pytest.mark.gpu
@pytest.mark.parametrize("H,R,adt,pdt,variant,family,off", _ln_cases())
def test_layernorm_gpu(H, R, adt, pdt, variant, family, off):
    """y, mean, rstd, dr, da, dw, db, dbias of every LayerNorm instantiation against _ref64: NC 1 .. 4, PER 4 / 12 /
    16 / 64, the pointer-alignment fallback (H768off), all four dtype pairs, the forward and backward grid-stride
    (R 16389), 127 / 128 / 129 partial rows in col_reduce_y (R 1016 / 1024 / 1025), a mask offset eoff = 5 H in
    every dropout case, and the four input families."""
    c = _ln_case(H, R, adt, pdt, variant, family, off)
    got = _ln_run(c)
    _assert_within(c.tag, _ln_path(H, off), got, c.emu, c.ref, LN_SPEC(adt, pdt))
    _ln_identities(c, got)
    if c.p > 0:  # dropped elements carry no gradient at all
        assert bool((~c.keep).any()) or R * H < 40
        assert bool((got["da"][~c.keep] == 0).all())
    elif c.bias is None:
        assert torch.equal(got["da"], got["dr"])


@pytest.mark.gpu
def test_layernorm_rejects_wide_rows_gpu():
    """H = 4160 > 64 * 64 is refused by the entry point (before any launch) and raised by check."""
    a = torch.randn(2, 4160, device="cuda")
    w = torch.ones(4160, device="cuda")
    with pytest.raises(RuntimeError, match="mifx_bert_bdaln_fwd"):
        fb.add_layernorm(a, a, w, w)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("H", [768, 100])
@pytest.mark.parametrize("pair", ["f32.f32", "bf16.bf16"])
def test_layernorm_shard_is_bitwise_gpu(H, pair):
    """A row shard [r0, r1) called with eoff = (5 + r0) H equals the same rows of the full call bit for bit (vector
    and scalar kernels, bias + dropout); two runs of the full call are bit-identical in every output."""
    c = _ln_case(H, 37, *PAIRS[pair], "biasdrop")
    full, again = _ln_run(c), _ln_run(c)
    for n in full:
        assert torch.equal(full[n], again[n]), n
    for r0, r1 in ((5, 23), (12, 37), (36, 37)):
        assert r0 * H % 4 == 0
        part = _ln_run(c, r0, r1)
        for n in ("y", "mean", "rstd", "dr", "da"):
            assert torch.equal(part[n], full[n][r0:r1]), (n, r0, r1)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("pair", ["f32.f32", "bf16.bf16"])
def test_layernorm_first_rows_of_large_call_gpu(H, pair):
    """The first k rows of a grid-striding call (R = 16389) equal a k-row call bit for bit."""
    c = _ln_case(H, 16389, *PAIRS[pair], "biasdrop")
    full = _ln_run(c)
    for k in (1, 37):
        part = _ln_run(c, 0, k)
        for n in ("y", "mean", "rstd", "dr", "da"):
            assert torch.equal(part[n], full[n][:k]), (n, k)


_RPW_CHILD = """
import os, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import test_fused_bert as t
t._rpw_cases()
"""


def _rpw_cases():
    for R in (37, 1025):
        for pair in ("f32.f32", "bf16.bf16"):
            c = _ln_case(768, R, *PAIRS[pair], "biasdrop")
            got = _ln_run(c)
            _assert_within(c.tag + f"/rpw{os.environ.get('MIFX_BERT_LN_RPW')}", "ln_vec", got, c.emu, c.ref,
                           LN_SPEC(c.adt, c.pdt))
            _ln_identities(c, got)


@pytest.mark.gpu
@pytest.mark.parametrize("rpw", [1, 16])
def test_layernorm_rows_per_wave_gpu(rpw):
    """MIFX_BERT_LN_RPW = 1 and 16 (read once per process, so each value runs in a fresh child): H = 768, R = 37 and
    1025 with bias + dropout under the same bound (257 and 17 rows of partials for R = 1025)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _RPW_CHILD, root], env={**os.environ, "MIFX_BERT_LN_RPW": str(rpw)},
                         cwd=root, timeout=300, capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.count("FB_RATIO") >= 4 * 8


# ---- GPU: bias + GELU -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,adt,pdt,off", _gelu_cases())
def test_bias_gelu_gpu(M, N, adt, pdt, off):
    """y, dx and db against _ref64: one row and one column group, M < 16 (one chunk), VW = 4 and 8, the scalar
    kernel by width (N 3070) and by pointer (off), the forward chunk cap (M 1025 > 1024), the backward cap of 512
    uneven chunks (M 8211), erf saturation at +-5.5, +-9, +-13 (finite gradients), and db against the float64 sum of
    the stored dx."""
    c = _gelu_case(M, N, adt, pdt, off)
    x, bias = _place(c.x, off).requires_grad_(), c.bias.cuda().requires_grad_()
    y = fb.bias_gelu(x, bias)
    y.backward(c.dy.cuda())
    got = {"y": y.detach().cpu(), "dx": x.grad.cpu(), "db": bias.grad.cpu()}
    assert got["db"].dtype == pdt
    fam = "gelu_vec" if _gelu_vec(N, adt, off) else "gelu_scalar"
    _assert_within(c.tag, fam, got, c.emu, c.ref, GELU_SPEC(adt, pdt))
    _assert_within(c.tag + "/identity", "identity", got, {"db": _rt(_seq_sum(got["dx"], 0), pdt)},
                   {"db": got["dx"].double().sum(0)}, {"db": ("col", pdt)})


# ---- GPU: standalone dropout ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.1, 0.5, 2.0 ** -17, 0.999995], ids=["p0.1", "p0.5", "thr1", "thr65536"])
@pytest.mark.parametrize("n", [1, 3, 4, 7007, 2097157])
def test_dropout_bitwise_gpu(n, p):
    """fb.dropout equals where(keep, round(x scale), 0) bit for bit in both dtypes, the last n striding the 2048-block
    grid; the backward draws the forward's mask after the live counter has advanced; the kept fraction is within 5
    binomial standard deviations of 1 - thr / 65536 (thr = 1: p = 2^-17 rounds up; thr = 65536: all dropped)."""
    thr = fb.drop_threshold(p)
    assert thr == {0.1: 6554, 0.5: 32768, 2.0 ** -17: 1, 0.999995: 65536}[p]
    keep = fb.keep_mask(n, _rng_cpu(), SITE, p)
    scale = fb._drop_scale(p)
    g = torch.Generator().manual_seed(n)
    for dt in (F32, BF16):
        x, dy = torch.randn(n, generator=g).to(dt), torch.randn(n, generator=g).to(dt)
        rng = _rng_gpu()
        xg = x.cuda().requires_grad_()
        y = fb.dropout(xg, p, rng, SITE)
        rng[1] += 1  # the live counter advances between forward and backward
        y.backward(dy.cuda())
        for got, src in ((y.detach().cpu(), x), (xg.grad.cpu(), dy)):
            want = torch.where(keep, (src.float() * scale).to(dt), torch.zeros((), dtype=dt))
            assert torch.equal(got, want)
    if n == 2097157:
        q = 1 - thr / 65536
        assert abs(float(keep.double().mean()) - q) <= 5 * math.sqrt(max(q * (1 - q), 0) / n)


# ---- GPU: col_sum -----------------------------------------------------------------------------------------------
COL_SHAPES = [(1, 768), (7, 3072), (32, 3072), (64, 2304), (65, 768), (4096, 2304), (8211, 16), (64, 12), (65, 12),
              (70, 3), (129, 520), (2032, 16), (2048, 16), (2071, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,off", [(M, N, False) for M, N in COL_SHAPES] + [(7, 3072, True), (65, 768, True),
                                                                             (129, 520, True)])
def test_col_sum_gpu(M, N, off):
    """fb.col_sum per 16 columns against the float64 sum: the one-pass kernel (M <= 64) and the two-pass one on
    either side of the limit, 512 uneven chunks (M 8211), VW = 4 at N = 12 in fp32 and the scalar kernel in bf16,
    N = 3, 127 / 128 / 129 rows of partials on either side of col_reduce2's unrolled batch of 128 (M 2032 / 2048 /
    2071), and a misaligned input (the scalar kernel); all four dtype pairs."""
    g = torch.Generator().manual_seed(M * N)
    for pair, (dt, odt) in PAIRS.items():
        x = torch.randn(M, N, generator=g).to(dt)
        got = fb.col_sum(_place(x, off), odt)
        assert got.dtype == odt
        _assert_within(f"M{M}/N{N}{'off' if off else ''}/{pair}", "col_sum", {"s": got.cpu()},
                       {"s": _rt(_seq_sum(x, 0), odt)}, {"s": x.double().sum(0)}, {"s": ("col", odt)})


# ---- GPU: embedding gradient ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("struct,N,H,pair", EMB_CASES, ids=[f"{s}-N{n}-H{h}-{p}" for s, n, h, p in EMB_CASES])
def test_embedding_grad_gpu(struct, N, H, pair):
    """The embedding gradient per (row, 16 columns) against the float64 scatter-add: ids with exactly 1, 63, 64, 65,
    128, 129 and 700 occurrences interleaved (one chunk, the chunk edge, 2, 3 and 11 chunks), N around the
    256-token scan block, 32768 tokens on one id (512 chunks: the capacity of the leader list) and on two interleaved
    ids, the vector (H 8, 96, 768, 2048 in bf16) and scalar (H 100, 2056, 2048 in fp32) column paths, bf16 dy into
    an fp32 weight, and the index_add_ route above 32768 tokens. Rows of unused ids stay exactly zero."""
    ddt, wdt = PAIRS[pair]
    c = _emb_case(struct, N, H, ddt, wdt)
    ids, dy = c.ids.cuda(), c.dy.cuda()
    if ddt == wdt:
        w = torch.zeros(c.V, H, device="cuda", dtype=wdt).requires_grad_()
        fb.embedding(ids.view(1, -1), w).backward(dy.view(1, N, H))
        g = w.grad
    else:  # autograd would cast dy to the weight's dtype first: the mixed kernels are reached from the backward
        ctx = types.SimpleNamespace(saved_tensors=(ids,), wshape=(c.V, H), wdtype=wdt)
        g = fb._Embedding.backward(ctx, dy)[1]
    assert g.dtype == wdt and g.shape == (c.V, H)
    got = {"g": g.cpu()}
    _assert_within(c.tag, "embedding", got, c.emu, c.ref, {"g": ("col", wdt)})
    unused = torch.ones(c.V, dtype=torch.bool)
    unused[c.ids] = False
    assert bool(unused.any()) and bool((got["g"][unused] == 0).all())
