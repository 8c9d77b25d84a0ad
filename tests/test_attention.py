"""csrc/attention.hip against a float64 reference, per 16-token tile.

The five kernels (attn_fwd / attn_bwd for S = 64 and 128: "short"; attn_fwd_long / attn_bwd_dq_long /
attn_bwd_dkv_long for S = 192 .. 512: "long") are compared with `_ref64`, attention written from its definition in
float64 on the bf16-rounded inputs, gradients by autograd. The yardstick of the bound is `_emulate`: the same
computation in float32 with the kernels' bf16 rounding points. With E its error against `_ref64`, a kernel must stay
within

    err_tile <= MARGIN * E_tile + FLOOR

for every tile of out, dq, dk and dv. A tile is (batch, head, 16 consecutive tokens): one wave's rows in every kernel,
so a wrong wave, lane group or chunk edge cannot hide in a global norm. err is the tile's L2 error relative to the
tile's L2 norm in the reference (`_tile_err` states the rule for zero and tiny tiles). E is computed here from the
emulation, never from a kernel. FLOOR = 2^-9 is one extra bf16 rounding of every element of the tile (a tile the
emulation happens to produce exactly may still be rounded once more by a kernel that sums in another order).

MARGIN = 3. Measured on an MI355X over every case of this file, the margin a kernel needs, max over tiles of
(err - FLOOR) / E, and in brackets the plain max of err / E over tiles with E >= FLOOR:

    kernels   out           dq            dk            dv
    short     0.34 (1.01)   0.95 (1.04)   0.97 (1.03)   0.34 (1.01)
    long      0.28 (1.09)   1.61 (2.18)   1.52 (2.03)   0.44 (1.03)

The short kernels round where the emulation rounds and follow it tile by tile. The long kernels' worst tiles are all
dq and dk of the peaky family and of the single live key (dq 1.50; its reference dq is zero); without those two,
no kernel needs more than 0.45 for any tensor. Where one key takes nearly all of a row, dS = P (dP - D) cancels,
and what is left is the rounding of the output that D = rowsum(dO o O) is formed from. attn_fwd_long rounds the
unnormalised P, so its output's rounding error is as large as the emulation's but independent of it, and a tile's
error is a ratio of two such noises (the supposed cause; the numbers are the same before and after the change to
the saved statistics).
2 would leave 1.24x over the worst 1.61, so 3 it is: 1.86x (1.38x or more on the plain ratio). The CPU tests below
hold the margin honest: four subtly wrong variants of the emulation (dropout scale off by 2 %, one chunk's rescale
of the running output dropped, the keep bits of one 4-key group permuted, P = 1 on a fully masked row in the
backward) must all exceed the same bound at the ceiling, margin 4.

A sequence whose keys are all masked (bias -1e30 everywhere) gets uniform attention and finite gradients in
`_ref64`. The kernels used to save lse = m + log(l) in one float; with m = -1e30 the log(l) term is absorbed, the
backward recomputed P = exp(0) = 1 instead of 1 / S and dq, dk, dv of such a sequence came out S times too large
(measured: per-tile errors of 63.0 at S = 64, 127 at 128, 255 at 256 and 319 at 320 in each of dq, dk and dv, short
and long kernels alike, against a bound of about 0.01; out was right). The row maximum and log2(l) are now saved
apart (stats [2, B, H, S]) and the backward takes them off one after the other, which is exact for such rows and
changes no measured ratio of any other case.
"""
import functools
import math
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

from mifx.ops import fused_bert as fb

DH = 64
SCALE = DH ** -0.5
H0, SITE, SEED_CTR = 1, 3, (5, 17)  # htot = H + 2: the global head offset and the b * Htot term both matter
NEG = -1e30  # the trainer's padding bias (mifx/models/bert.py)
TILE = 16
FLOOR = 2.0 ** -9
MARGIN = 3
# below 1e-6 of the tensor's largest tile, fp32 partial sums of the large tiles' scale no longer resolve the tile
TINY = 1e-6


def _rng_cpu():
    return torch.tensor(SEED_CTR, dtype=torch.int64)


def _bf(t):
    return t.bfloat16().float()


# ---- inputs -----------------------------------------------------------------------------------------------------
def _qkv(family, B, H, S, seed=0):
    """[B, S, 3, H, 64] bf16. diffuse: 0.7 randn (scaled scores of std 0.5, near-uniform softmax). peaky: q and k of
    variance 5, scaled scores of std 5, a few keys dominate each row. rising / falling: dim 0 of q is 4 and dim 0
    of k is -24 * (distance in 64-key chunks from the last / first chunk), so the row maximum moves by 12 +- 1 from
    chunk to chunk: every chunk of the online softmax rescales by alpha ~ e^-12 (rising), or none does and later
    chunks enter through exp(s - m) only (falling). The dominant chunk has 0 there, not the largest value: softmax
    does not see a constant added to k along a direction all queries share, but dq = dS K does, as sum_j dS_ij = 0
    times that constant, which the bf16 rounding of dS turns into noise (with +24 per chunk towards the dominant
    one instead, the emulation's own dq error E was 3 to 15 % per tile, and a bound on a ratio of two such noises
    says nothing)."""
    g = torch.Generator().manual_seed(1000 * S + 10 * H + seed)
    x = torch.randn(B, S, 3, H, DH, generator=g) * 0.7
    if family == "peaky":
        x[:, :, :2] *= 5 ** 0.5 / 0.7
    elif family in ("rising", "falling"):
        c = torch.arange(S) // 64
        dist = c if family == "falling" else (S // 64 - 1) - c
        x[:, :, 0, :, 0] = 4.0
        x[:, :, 1, :, 0] = (-24.0 * dist)[None, :, None]
    else:
        assert family == "diffuse"
    return x.bfloat16()


MASKS = ("none", "tail9", "tailhalf", "left64", "leftmost", "hole", "one", "rand", "full")


def _kbias(mask, B, S):
    """Additive key bias [B, S] fp32 (None for "none"). Except for "rand" and "full" the last sequence of the batch
    is masked and the others are not, so the b * S offset into the bias matters."""
    if mask == "none":
        return None
    kb = torch.zeros(B, S)
    if mask == "tail9":
        kb[-1, S - 9:] = NEG
    elif mask == "tailhalf":
        kb[-1, S // 2:] = NEG
    elif mask == "left64":  # a whole first chunk: the running maximum starts at -1e30 and is rescaled away
        kb[-1, :64] = NEG
    elif mask == "leftmost":
        kb[-1, :S - 64] = NEG
    elif mask == "hole":  # not aligned to the 4-key lane groups
        kb[-1, 37:91] = NEG
    elif mask == "one":  # a single live key
        kb[-1] = NEG
        kb[-1, 5] = 0.0
    elif mask == "rand":  # the bias is additive, not a boolean
        kb = torch.rand(B, S, generator=torch.Generator().manual_seed(S)) * 6 - 3
    elif mask == "full":  # a fully masked sequence next to a normal one
        kb[0] = NEG
    else:
        raise ValueError(mask)
    return kb


@functools.lru_cache(maxsize=8)
def _keep(B, H, S, p):
    """keep[b, h, i, j] of this rank's heads: fb.keep_mask at ((b Htot + h0 + h) S + i) S + j."""
    htot = H + 2
    return fb.keep_mask(B * htot * S * S, _rng_cpu(), SITE, p).view(B, htot, S, S)[:, H0:H0 + H]


# ---- references -------------------------------------------------------------------------------------------------
def _ref64(qkv, kb, p, keep, dout):
    """out, dqkv, lse in float64 from the definition: scores, key bias, softmax, keep mask * 1 / (1 - p), P V."""
    x = qkv.double().requires_grad_()
    q, k, v = x.unbind(2)
    s = torch.einsum("bihd,bjhd->bhij", q, k) * SCALE
    if kb is not None:
        s = s + kb.double()[:, None, None, :]
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    pr = e / l
    if p > 0:
        pr = pr * (keep.double() * fb._drop_scale(p))
    out = torch.einsum("bhij,bjhd->bihd", pr, v)
    out.backward(dout.double())
    return out.detach(), x.grad, (m + torch.log(l)).squeeze(-1).detach()


def _emulate(qkv, kb, p, keep, dout, drop_scale=None, keep_bwd=None, masked_row_p_one=False):
    """The same in float32 with the kernels' rounding points: P_d to bf16 before P V, the output to bf16; in the
    backward P_d and dS to bf16 before their GEMMs, D = rowsum(dO o O) from the rounded output, dq / dk / dv to
    bf16. The keyword arguments are the mutants of the sensitivity check."""
    q, k, v = (t.float() for t in qkv.unbind(2))
    s = torch.einsum("bihd,bjhd->bhij", q, k) * SCALE
    if kb is not None:
        s = s + kb.float()[:, None, None, :]
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    pr = e / e.sum(-1, keepdim=True)
    dsc = (fb._drop_scale(p) if drop_scale is None else drop_scale) if p > 0 else 1.0
    mf = keep.float() if p > 0 else torch.ones(())
    out = _bf(torch.einsum("bhij,bjhd->bihd", _bf(pr * dsc * mf), v))
    if masked_row_p_one:  # lse = -1e30 + log(S) == -1e30 in fp32: the backward's exp(s - lse) is 1
        pr = torch.where(m < 0.5 * NEG, torch.ones(()), pr)
    mb = mf if keep_bwd is None else keep_bwd.float()
    do = dout.float()
    dsum = (do * out).sum(-1).permute(0, 2, 1)[..., None]  # [B, H, S, 1]
    dp = torch.einsum("bihd,bjhd->bhij", do, v) * dsc * mb
    ds = _bf(pr * (dp - dsum) * SCALE)
    pd = _bf(pr * dsc * mb)
    dq = torch.einsum("bhij,bjhd->bihd", ds, k)
    dk = torch.einsum("bhij,bihd->bjhd", ds, q)
    dv = torch.einsum("bhij,bihd->bjhd", pd, do)
    return out, _bf(torch.stack((dq, dk, dv), 2))


def _emulate_fwd_chunked(qkv, kb, p, keep, skip_rescale=None):
    """The forward as attn_fwd_long computes it: 64-key chunks, running maximum and row sum, the output accumulator
    rescaled by alpha = exp(m_old - m_new) per chunk, the unnormalised P rounded to bf16. skip_rescale: the chunk
    whose rescale of the accumulator is left out (mutant)."""
    q, k, v = (t.float() for t in qkv.unbind(2))
    B, S, H, _ = q.shape
    s = torch.einsum("bihd,bjhd->bhij", q, k) * SCALE
    if kb is not None:
        s = s + kb.float()[:, None, None, :]
    m = torch.full((B, H, S, 1), -3.0e38)
    l = torch.zeros(B, H, S, 1)
    o = torch.zeros(B, H, S, DH)
    for c in range(0, S, 64):
        sc = s[..., c:c + 64]
        mc = torch.maximum(m, sc.amax(-1, keepdim=True))
        alpha = torch.exp(m - mc)
        m, l = mc, l * alpha
        if c // 64 != skip_rescale:
            o = o * alpha
        pe = torch.exp(sc - m)
        l = l + pe.sum(-1, keepdim=True)
        if p > 0:
            pe = pe * keep[..., c:c + 64].float()
        o = o + torch.einsum("bhij,bjhd->bhid", _bf(pe), v[:, c:c + 64])
    dsc = fb._drop_scale(p) if p > 0 else 1.0
    return _bf(o * (dsc / l)).permute(0, 2, 1, 3)


# ---- metric and bound -------------------------------------------------------------------------------------------
def _tile_norms(x):
    """L2 norms over (16 consecutive tokens, head dim) of a [B, S, H, 64] tensor -> [B, S / 16, H], float64."""
    B, S, H, D = x.shape
    return x.double().reshape(B, S // TILE, TILE, H, D).pow(2).sum((2, 4)).sqrt()


def _tile_err(got, ref):
    """Per-tile L2 error relative to the reference tile's norm. A reference tile that is zero or tiny (below TINY
    of the tensor's largest tile: a row whose live keys were all dropped, dq / dk of masked keys, keys that e^-24
    of a rising family leaves without weight) is compared absolutely, against the largest tile norm."""
    n = _tile_norms(ref)
    top = n.max()
    return _tile_norms(got.double() - ref.double()) / torch.where(n >= TINY * top, n, top)


def _split(out, dqkv):
    return {"out": out, "dq": dqkv[:, :, 0], "dk": dqkv[:, :, 1], "dv": dqkv[:, :, 2]}


def _excess(got, emu, ref, margin=MARGIN):
    """max over tiles of err - (margin E + FLOOR): positive means outside the bound."""
    return float((_tile_err(got, ref) - (margin * _tile_err(emu, ref) + FLOOR)).max())


def _assert_within(tag, got, emu, ref):
    """got, emu, ref: dicts of out / dq / dk / dv. Prints the measured ratios before asserting."""
    bad = []
    for name in ("out", "dq", "dk", "dv"):
        err, e = _tile_err(got[name], ref[name]), _tile_err(emu[name], ref[name])
        need = float(((err - FLOOR).clamp(min=0) / e.clamp(min=1e-30)).max())
        big = e >= FLOOR
        plain = float((err[big] / e[big]).max()) if bool(big.any()) else 0.0
        print(f"ATTN_RATIO {tag} tensor={name} need={need:.3f} plain={plain:.3f} "
              f"maxerr={float(err.max()):.3e} maxE={float(e.max()):.3e}")
        if not bool((err <= MARGIN * e + FLOOR).all()):
            i = int((err - MARGIN * e).argmax())
            bad.append(f"{name}: tile {i} err {float(err.flatten()[i]):.4g} > {MARGIN} * "
                       f"{float(e.flatten()[i]):.4g} + {FLOOR:.4g} (needs margin {need:.2f})")
    assert not bad, f"{tag}: " + "; ".join(bad)


@functools.lru_cache(maxsize=4)
def _case(family, mask, B, H, S, p):
    qkv = _qkv(family, B, H, S)
    kb = _kbias(mask, B, S)
    dout = torch.randn(B, S, H, DH, generator=torch.Generator().manual_seed(S + 1)).bfloat16()
    keep = _keep(B, H, S, p) if p > 0 else None
    out, dqkv, lse = _ref64(qkv, kb, p, keep, dout)
    eo, ed = _emulate(qkv, kb, p, keep, dout)
    return types.SimpleNamespace(family=family, mask=mask, B=B, H=H, S=S, p=p, qkv=qkv, kb=kb, dout=dout, keep=keep,
                                 ref=_split(out, dqkv), emu=_split(eo, ed), lse=lse)


# ---- CPU: the references are what they claim to be ---------------------------------------------------------------
def test_ref64_matches_library_references():
    """_ref64 against scaled_dot_product_attention (p = 0) and fb.attention_reference (p = 0 and p > 0, same
    counter-based mask, head offset), values and gradients."""
    B, H, S, p = 2, 2, 48, 0.25
    qkv = _qkv("peaky", B, H, S)
    kb = _kbias("rand", B, S)
    kb[1, 40:] = NEG
    dout = torch.randn(B, S, H, DH, generator=torch.Generator().manual_seed(7)).bfloat16()
    out, dqkv, lse = _ref64(qkv, kb, 0.0, None, dout)
    x = qkv.double().requires_grad_()
    q, k, v = (t.transpose(1, 2) for t in x.unbind(2))
    sd = F.scaled_dot_product_attention(q, k, v, attn_mask=kb.double()[:, None, None, :], scale=SCALE).transpose(1, 2)
    sd.backward(dout.double())
    torch.testing.assert_close(out, sd, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(dqkv, x.grad, rtol=1e-9, atol=1e-11)
    s = torch.einsum("bihd,bjhd->bhij", qkv.double()[:, :, 0], qkv.double()[:, :, 1]) * SCALE + kb.double()[:, None,
                                                                                                           None]
    torch.testing.assert_close(lse, torch.logsumexp(s, -1), rtol=1e-12, atol=1e-12)
    for pp in (0.0, p):
        keep = _keep(B, H, S, pp) if pp > 0 else None
        out, dqkv, _ = _ref64(qkv, kb, pp, keep, dout)
        x = qkv.float().requires_grad_()
        r = fb.attention_reference(x, kb, SCALE, pp, _rng_cpu(), SITE, H0, H + 2)
        r.backward(dout.float())
        torch.testing.assert_close(r.double(), out, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(x.grad.double(), dqkv, rtol=1e-4, atol=1e-4)
        if pp > 0:  # some probabilities are dropped, and rows differ
            assert 0.15 < 1 - keep.float().mean() < 0.35


CPU_SHAPE = (2, 2, 256)  # four 64-key chunks


@pytest.mark.parametrize("family", ["diffuse", "peaky", "rising", "falling"])
@pytest.mark.parametrize("mask", ["tail9", "full"])
def test_emulation_within_bound(family, mask):
    """The unmutated emulations stay within the bound the GPU tests use: the chunked forward (another summation
    order, the unnormalised P rounded) against E of the one-pass emulation, even at margin 2."""
    for p in (0.0, 0.1):
        c = _case(family, mask, *CPU_SHAPE, p)
        got = _emulate_fwd_chunked(c.qkv, c.kb, p, c.keep)
        assert _excess(got, c.emu["out"], c.ref["out"], margin=2) <= 0


def _mutant_excess(c, **kw):
    out, dqkv = _emulate(c.qkv, c.kb, c.p, c.keep, c.dout, **kw)
    got = _split(out, dqkv)
    return {n: _excess(got[n], c.emu[n], c.ref[n], margin=4) for n in got}


def test_mutant_dropout_scale():
    """a. dropout scale * 1.02: outside the bound (at the ceiling margin 4) even in the diffuse family, in the
    forward and in every gradient."""
    ex = _mutant_excess(_case("diffuse", "tail9", *CPU_SHAPE, 0.1), drop_scale=fb._drop_scale(0.1) * 1.02)
    assert all(v > 0 for v in ex.values()), ex


def test_mutant_chunk_rescale():
    """b. one chunk's rescale of the running output omitted: outside the bound where the maximum rises from chunk
    to chunk. The last chunk's
    rescale is the one that shows: what an earlier chunk failed to scale down, the later ones still scale by
    e^-12 each. So every chunk index is tried as the last one of a shorter sequence."""
    for S in (128, 192, 256):
        c = _case("rising", "tail9", 2, 2, S, 0.0)
        got = _emulate_fwd_chunked(c.qkv, c.kb, 0.0, None, skip_rescale=S // 64 - 1)
        assert _excess(got, c.emu["out"], c.ref["out"], margin=4) > 0, S


@pytest.mark.parametrize("family", ["diffuse", "peaky"])
def test_mutant_keep_bits(family):
    """c. the keep bits of one 4-key group (keys 84 .. 87 of one head) permuted: rotated by one key, in every query
    row, as a lane-group or quad-exchange mix-up would do it."""
    c = _case(family, "tail9", *CPU_SHAPE, 0.1)
    keep = c.keep.clone()
    keep[0, 1, :, 84:88] = torch.roll(c.keep[0, 1, :, 84:88], 1, -1)
    assert 0 < int((keep != c.keep).sum()) < 4 * CPU_SHAPE[2]
    out, dqkv = _emulate(c.qkv, c.kb, 0.1, keep, c.dout)
    got = _split(out, dqkv)
    ex = {n: _excess(got[n], c.emu[n], c.ref[n], margin=4) for n in got}
    assert ex["out"] > 0 and ex["dq"] > 0, ex
    ex = _mutant_excess(c, keep_bwd=keep)  # only the backward's mask: the dK / dV exchange of the long kernel
    assert ex["dq"] > 0, ex


def test_mutant_masked_row_probability():
    """d. P = 1 instead of 1 / S on a fully masked row in the backward."""
    c = _case("diffuse", "full", *CPU_SHAPE, 0.0)
    ex = _mutant_excess(c, masked_row_p_one=True)
    assert ex["out"] <= 0 and all(ex[n] > 0 for n in ("dq", "dk", "dv")), ex


# ---- GPU ---------------------------------------------------------------------------------------------------------
def _kernels(S):
    return "short" if S <= 128 else "long"


def _run_gpu(c):
    from mifx.ops import native_stats

    qkv = c.qkv.cuda().requires_grad_()
    kb = None if c.kb is None else c.kb.cuda()
    rng = torch.tensor(SEED_CTR, dtype=torch.int64, device="cuda")
    native_stats.reset()
    out = fb.attention(qkv, kb, SCALE, c.p, rng, SITE, H0, c.H + 2)
    assert native_stats.snapshot()["attention"] == {"native": 1, "fallback": 0}  # the HIP kernels ran
    out.backward(c.dout.cuda())
    got = _split(out.detach().float().cpu(), qkv.grad.float().cpu())
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), name
    return got


# B H nqb (nqb 128-query blocks per head) is a multiple of 8 at (2, 2, 192), 256, 448 and 512 and is not at
# (2, 3, 192) and 320: both branches of xcd_block, with a half-idle last block (192, 320, 448) in either
SHAPES = [(2, 3, 64), (2, 2, 128), (2, 3, 192), (2, 2, 192), (2, 2, 256), (2, 3, 320), (2, 2, 448), (2, 3, 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,H,S", SHAPES)
@pytest.mark.parametrize("family", ["diffuse", "peaky", "rising", "falling"])
def test_attention_families_gpu(family, B, H, S, p):
    """Forward and backward per tile against _ref64, tail padding of 9 keys on the last sequence. Measured need
    (see the file's docstring) for out / dq / dk / dv: short kernels 0.33 / 0.81 / 0.80 / 0.33, long kernels
    0.28 / 1.61 / 1.16 / 0.40, the peaky family the worst in each; rising and falling stay below 0.43."""
    c = _case(family, "tail9", B, H, S, p)
    _assert_within(f"kernels={_kernels(S)} case={family}/tail9/S{S}/H{H}/p{p}", _run_gpu(c), c.emu, c.ref)


MASK_SHAPES = [(2, 3, 64), (2, 2, 128), (2, 2, 256), (2, 3, 320)]


def _mask_cases():
    for B, H, S in MASK_SHAPES:
        for mask in MASKS:
            if mask == "tail9" or (mask == "left64" and S == 64) or (mask == "leftmost" and S < 256):
                continue  # tail9: test_attention_families_gpu; left64 at S = 64 is "full"
            yield pytest.param(mask, B, H, S, id=f"{mask}-{S}")


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("family", ["diffuse", "peaky"])
@pytest.mark.parametrize("mask,B,H,S", list(_mask_cases()))
def test_attention_masks_gpu(mask, B, H, S, family, p):
    """No bias at all, padding at either end (a whole masked first chunk; all but the last chunk), a hole that is not
    4-aligned, a single live key, a finite random bias, and a fully masked sequence next to a normal one: all per
    tile against _ref64. The fully masked sequence failed before the row maximum and log(l) were saved apart:
    dq / dk / dv tile errors of S - 1 (63 at S = 64, 319 at S = 320) against a bound of about 0.01. Measured need
    for out / dq / dk / dv: short kernels 0.34 / 0.95 / 0.97 / 0.34, long kernels 0.28 / 1.50 / 1.52 / 0.40."""
    c = _case(family, mask, B, H, S, p)
    got = _run_gpu(c)
    _assert_within(f"kernels={_kernels(S)} case={family}/{mask}/S{S}/H{H}/p{p}", got, c.emu, c.ref)
    if mask == "one":
        v5 = c.qkv[-1, 5, 2].float()  # [H, 64]
        o = got["out"][-1]  # [S, H, 64]
        if p == 0:  # out[b, i] == v_5 to bf16 rounding, for every query
            assert bool(((o - v5).abs() <= 2.0 ** -8 * v5.abs()).all())
        else:  # rows whose only live key is dropped are exactly 0
            dropped = ~c.keep[-1, :, :, 5].T  # [S, H]
            assert bool(dropped.any()) and bool((o[dropped] == 0).all())
            assert bool((o[~dropped].abs().sum(-1) > 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("S", [64, 128, 192, 512])
def test_attention_dropout_mask_bits_gpu(S, p):
    """The dropout mask bit for bit. With q = 0, P is uniform; with V[j, d] = (j == 64c + d) the forward output
    out[b, i, h, d] S (1 - p) is the keep bit of (i, 64c + d), and with dO[i, d] = (i == 64c + d) the backward's
    dV[b, j, h, d] S (1 - p) is the keep bit of (64c + d, j) as attn_bwd and attn_bwd_dkv_long's quad exchange use
    it. Both must equal fb.keep_mask at ((b Htot + h0 + h) S + i) S + j exactly; p = 0.5 also pins drop_threshold's
    rounding against the host twin."""
    B, H = 2, 2
    keep = _keep(B, H, S, p)
    rng = torch.tensor(SEED_CTR, dtype=torch.int64, device="cuda")
    eye = torch.eye(64)
    unit = S / fb._drop_scale(p)
    for c in range(S // 64):
        x = torch.zeros(B, S, 3, H, DH)
        x[:, :, 1] = _qkv("diffuse", B, H, S)[:, :, 1].float()
        x[:, 64 * c:64 * c + 64, 2] = eye[None, :, None, :]
        qkv = x.bfloat16().cuda().requires_grad_()
        out = fb.attention(qkv, None, SCALE, p, rng, SITE, H0, H + 2)
        dout = torch.zeros(B, S, H, DH)
        dout[:, 64 * c:64 * c + 64] = eye[None, :, None, :]
        out.backward(dout.bfloat16().cuda())
        fwd = (out.detach().float().cpu() * unit).round()  # [B, S(i), H, 64(d)]
        assert bool(((fwd == 0) | (fwd == 1)).all())
        assert torch.equal(fwd.bool().permute(0, 2, 1, 3), keep[..., 64 * c:64 * c + 64]), f"forward, chunk {c}"
        bwd = (qkv.grad[:, :, 2].float().cpu() * unit).round()  # [B, S(j), H, 64(d)] = P_d[64c + d, j]
        assert bool(((bwd == 0) | (bwd == 1)).all())
        assert torch.equal(bwd.bool().permute(0, 2, 3, 1), keep[:, :, 64 * c:64 * c + 64, :]), f"dV, chunk {c}"


def _direct(qkv, kb, p, dout, rng):
    """mifx_attn_fwd / mifx_attn_bwd called directly on NaN-filled outputs and workspaces."""
    B, S, _, H, _ = qkv.shape
    nan = float("nan")
    out = torch.full((B, S, H, DH), nan, device="cuda", dtype=torch.bfloat16)
    stats = torch.full((2, B, H, S), nan, device="cuda")
    dqkv = torch.full_like(qkv, nan)
    dsum = torch.full((B, H, S), nan, device="cuda")
    st = fb.stream_handle(qkv.device)
    r = fb.ptr(rng if p > 0 else None)
    fb.check(fb._attn_fns()["fwd"](fb.ptr(qkv), fb.ptr(kb), B, S, H, H0, H + 2, SCALE, p, r, SITE, fb.ptr(out),
                                   fb.ptr(stats), st), "mifx_attn_fwd")
    fb.check(fb._attn_fns()["bwd"](fb.ptr(qkv), fb.ptr(kb), fb.ptr(out), fb.ptr(dout), fb.ptr(stats), B, S, H, H0,
                                   H + 2, SCALE, p, r, SITE, fb.ptr(dqkv), fb.ptr(dsum), st), "mifx_attn_bwd")
    torch.cuda.synchronize()
    return out, stats, dqkv, dsum


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,S", [(2, 3, 64), (2, 2, 128), (2, 3, 192), (2, 3, 320), (2, 2, 448)])
def test_attention_writes_everything_and_lse_gpu(B, H, S):
    """Every element of out, the saved statistics, dqkv and (S > 128) the dsum workspace is written, the half-idle
    last 128-query block of S = 192, 320 and 448 included; and the saved statistics are the float64 logsumexp of
    the biased scores: stats[0] + ln 2 * stats[1] (row maximum and log2 of the row sum, kept apart so that a fully
    masked row, maximum -1e30, keeps its log2(S)) to 1e-5 relative."""
    c = _case("diffuse", "full", B, H, S, 0.1)
    rng = torch.tensor(SEED_CTR, dtype=torch.int64, device="cuda")
    out, stats, dqkv, dsum = _direct(c.qkv.cuda(), c.kb.cuda(), 0.1, c.dout.cuda(), rng)
    for name, t in (("out", out), ("stats", stats), ("dqkv", dqkv)) + ((("dsum", dsum),) if S > 128 else ()):
        assert not bool(torch.isnan(t).any()), f"{name} has unwritten elements"
    m, log2l = stats.double().cpu()
    live = c.lse[1]  # the normal sequence
    assert bool(((m[1] + math.log(2) * log2l[1] - live).abs() <= 1e-5 * live.abs()).all())
    assert bool((m[0] == float(torch.tensor(NEG))).all())  # the fully masked one: its parts, each on its own
    assert bool(((log2l[0] - math.log2(S)).abs() <= 1e-5 * math.log2(S)).all())
    _assert_within(f"kernels={_kernels(S)} case=direct/full/S{S}/H{H}/p0.1",
                   _split(out.float().cpu(), dqkv.float().cpu()), c.emu, c.ref)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,H,S", [(2, 2, 128), (2, 3, 320)])
def test_attention_deterministic_gpu(B, H, S, p):
    """Forward and backward twice: out and dqkv bit-identical (no atomics, no order left to the scheduler)."""
    c = _case("peaky", "hole", B, H, S, p)
    rng = torch.tensor(SEED_CTR, dtype=torch.int64, device="cuda")
    runs = [_direct(c.qkv.cuda(), c.kb.cuda(), p, c.dout.cuda(), rng) for _ in range(2)]
    for name, a, b in zip(("out", "stats", "dqkv"), *runs):
        assert torch.equal(a, b), name


_QSPLIT_CHILD = """
import os, sys, torch
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import test_attention as t
torch.save(t._qsplit_outputs(), sys.argv[2])
"""


def _qsplit_outputs():
    """S = 128 forward outputs and saved statistics for a fixed seed, without and with dropout."""
    c = _case("peaky", "hole", 2, 3, 128, 0.0)
    rng = torch.tensor(SEED_CTR, dtype=torch.int64, device="cuda")
    res = []
    for p in (0.0, 0.1):
        out, stats, _, _ = _direct(c.qkv.cuda(), c.kb.cuda(), p, c.dout.cuda(), rng)
        res += [out.cpu(), stats.cpu()]
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("qs", [2, 4])
def test_attention_qsplit_gpu(qs, tmp_path):
    """MIFX_ATTN_QSPLIT = 2 and 4 (attn_fwd<128, QS>: QS workgroups per head, read once per process, so each value
    runs in a fresh child): bit-identical to QS = 1, as each wave's arithmetic is the same."""
    if "MIFX_ATTN_QSPLIT" in os.environ:
        pytest.skip("MIFX_ATTN_QSPLIT is set for this process: no QS = 1 result to compare with")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / f"qs{qs}.pt")
    subprocess.run([sys.executable, "-c", _QSPLIT_CHILD, root, path], env={**os.environ, "MIFX_ATTN_QSPLIT": str(qs)},
                   cwd=root, check=True, timeout=300)
    for a, b in zip(_qsplit_outputs(), torch.load(path)):
        assert not bool(torch.isnan(b.float()).any())
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,S", [(2, 2, 128), (2, 3, 192)])
def test_attention_input_plumbing_gpu(B, H, S):
    """A non-contiguous qkv view and an fp32, non-contiguous dout give the results of their contiguous bf16
    equivalents, bit for bit."""
    c = _case("diffuse", "tail9", B, H, S, 0.1)
    rng = torch.tensor(SEED_CTR, dtype=torch.int64, device="cuda")
    kb = c.kb.cuda()

    def run(qkv, dout):
        qkv = qkv.requires_grad_()
        out = fb.attention(qkv, kb, SCALE, 0.1, rng, SITE, H0, H + 2)
        (g,) = torch.autograd.grad(out, qkv, dout)
        return out.detach(), g

    want = run(c.qkv.cuda(), c.dout.cuda())
    wide = torch.zeros(B, S, 3, H + 1, DH + 8, device="cuda", dtype=torch.bfloat16)
    wide[:, :, :, :H, :DH] = c.qkv.cuda()
    view = wide[:, :, :, :H, :DH].detach()
    assert not view.is_contiguous()
    dout32 = c.dout.float().cuda().transpose(1, 2).contiguous().transpose(1, 2)
    assert not dout32.is_contiguous() and dout32.dtype == torch.float32
    got = run(view, dout32)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
