"""BERT fine-tuning on packed variable-length batches: csrc/attn_varlen_train.hip, mifx/ops/attn_varlen.py,
BertForSequenceClassification.forward_packed and the packed BertTrainer.

Attention. The three kernels (attn_fwd_varlen_train, attn_bwd_dq_varlen, attn_bwd_dkv_varlen) are compared per
(sequence, head, 16-token tile; the last tile of a sequence holds its L % 16 remaining rows) with `_ref64`: attention
from its definition in float64 on the bf16-rounded inputs of that sequence alone, gradients by autograd. Yardstick and
metric are those of tests/test_attention.py:

    err_tile <= MARGIN * E_tile + FLOOR,    MARGIN = 3, FLOOR = 2^-9

for each of out, dq, dk and dv. err is the tile's L2 error relative to the tile's L2 norm in the reference; a tile
that is zero or below TINY of the tensor's largest tile OVER THE WHOLE PACK is compared against that largest tile (a
1-token sequence has a reference dq and dk of exactly zero and is its own only tile). E is the same error of
`_emulate`, float32 with the kernels' bf16 rounding points; it comes from the emulation, never from a kernel. The
parent kernels need, by that file's header, out 0.28, dq 1.61, dk 1.52 and dv 0.44 of the margin of 3.

Cases: lengths 1, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 191, 257 and 512 (1,718 tokens), H = 2, in two pack
orders: "head13" starts with the 1- and 3-token sequences (cu = 0, 1, 4, 19, 35, 52, 115, ...: the packed rows have
no alignment) in a buffer with 10 spare rows, "tail512_1" ends with 512 and then 1 in a buffer of exactly T rows
(the row after the last sequence is past the allocation); families diffuse and peaky; p = 0 and p = 0.1 with h0 = 1
of htot = H + 2.

Replaced cases. In the peaky family the lengths whose last 16-token tile holds 1 to 3 rows (3, 17, 65, 129, 130, 257)
are replaced by 8, 24, 72, 136, 137 and 264, whose last tile holds 8 or 9 rows; the diffuse family keeps every length,
so each edge (one row past a tile, a chunk, a 128-row block) is still run. Why: where one key takes nearly all of a
row, dS = P (dP - D) cancels and what is left of that row's dq and dk is one scalar, the rounding error of
D = rowsum(dO o O), i.e. of the rounded output (tests/test_attention.py's header). The kernels round the unnormalised
P and the yardstick the normalised one, so the two errors are independent, and for a tile of k rows err / E is the
ratio of two independent chi_k variables: above 3 with probability 0.20 at k = 1, 0.10 at k = 2, 0.05 at k = 3, and
0.003 at k = 8. With k <= 3 the bound says nothing about such a tile; the kernel-order emulation itself landed outside
it there (dq of the single 65th row: err 1.0e-2, E 2.7e-3, need 3.07), before any kernel was run.

`_emulate_varlen` is the kernels' own order (64-row chunks, zero-filled staging rows, the select of dead keys in the dq
pass and of dead queries in the dkv pass, per-row statistics m and log2 l); it stays within the bound on every case on
the CPU. Three wrong variants exceed it at the ceiling, margin 4:
 a. the dead query rows of the dkv pass computed instead of selected to zero. With zero-filled Q and dO staging rows
    the select is, in exact arithmetic, a no-op (P_d and dS of a dead row multiply a zero row); it matters when the
    row's statistics are not its own: the mutant stages the NEXT sequence's Q / dO rows and statistics there, as
    unpredicated loads would, and does not select;
 b. the last partial 16-query tile left out of dk and dv;
 c. the dropout mask indexed by the row inside the sequence instead of the packed row.

Margin the kernels need, measured on an MI355X (max over tiles of (err - FLOOR) / E, in brackets the plain max of
err / E over tiles with E >= FLOOR), the worst of the two pack orders:

    family   p     out           dq            dk            dv
    diffuse  0     0.28 (1.20)   0.60 (1.21)   0.66 (1.40)   0.36 (1.01)
    diffuse  0.1   0.39 (1.23)   1.23 (1.87)   0.74 (1.33)   0.32 (1.01)
    peaky    0     0.00 (0.88)   1.33 (1.90)   1.18 (1.67)   0.31 (1.00)
    peaky    0.1   0.00 (0.91)   1.04 (1.55)   1.15 (1.62)   0.41 (1.01)

so out 0.39, dq 1.33, dk 1.18 and dv 0.41 of the margin of 3, at or below what the parent's long kernels need. The
kernel-order emulation on the CPU needs the same margins to three digits in its worst cases (dq 1.326 peaky / p 0 and
1.227 diffuse / p 0.1, dk 1.178): the kernels round where it rounds.

End to end (test_packed_trainer_step_against_padded_gpu, same machine), max abs error against the fp32 CPU model run
per sequence, packed / the padded bf16 step / the bound 2 E_pad + one bf16 ulp: loss 5.1e-5 / 5.4e-5 / 4.0e-3,
classifier.weight gradient 4.8e-4 / 4.6e-4 / 1.4e-3, layers.0.qkv.weight gradient 5.6e-6 / 7.0e-6 / 1.8e-5, touched
word-embedding rows 3.4e-4 / 3.4e-4 / 9.3e-4.
"""
import functools
import json
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mifx.models.bert import BertConfig, BertForSequenceClassification, full_init_state
from mifx.ops import attn_varlen as av
from mifx.ops import bert_infer as bi
from mifx.ops import fused_bert as fb

DH = 64
SCALE = DH ** -0.5
TILE = 16
FLOOR = 2.0 ** -9
MARGIN = 3
TINY = 1e-6
H = 2
H0, SITE, SEED_CTR = 1, 3, (5, 17)
LENGTHS = {"diffuse": [1, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 191, 257, 512],
           "peaky": [1, 8, 15, 16, 24, 63, 64, 72, 127, 128, 136, 137, 191, 264, 512]}
ORDERS = ("head13", "tail512_1")


def _order(order, family):
    """(lengths in pack order, spare rows of the buffer)."""
    ls = LENGTHS[family]
    return (ls, 10) if order == "head13" else ([L for L in ls if L not in (1, 512)] + [512, 1], 0)


LOG2E = 1.4426950408889634
NAMES = ("out", "dq", "dk", "dv")


def _rng_cpu():
    return torch.tensor(SEED_CTR, dtype=torch.int64)


def _bf(t):
    return t.bfloat16().float()


def _slices(lengths):
    cu = bi.cu_seqlens(lengths)
    return [slice(cu[b], cu[b + 1]) for b in range(len(lengths))]


# ---- one sequence: x [L, 3, H, 64], keep [H, L, L] or None, dout [L, H, 64] --------------------------------------------
def _ref64(x, keep, p, dout):
    x = x.double().requires_grad_()
    q, k, v = x.unbind(1)
    pr = torch.softmax(torch.einsum("ihd,jhd->hij", q, k) * SCALE, -1)
    if p > 0:
        pr = pr * (keep.double() * fb._drop_scale(p))
    out = torch.einsum("hij,jhd->ihd", pr, v)
    out.backward(dout.double())
    return _split(out.detach(), x.grad)


def _split(out, dqkv):
    return {"out": out, "dq": dqkv[:, 0], "dk": dqkv[:, 1], "dv": dqkv[:, 2]}


def _emulate(x, keep, p, dout):
    """float32 with the kernels' rounding points (tests/test_attention.py `_emulate`, one sequence)."""
    q, k, v = x.float().unbind(1)
    pr = torch.softmax(torch.einsum("ihd,jhd->hij", q, k) * SCALE, -1)
    dsc = fb._drop_scale(p) if p > 0 else 1.0
    mf = keep.float() if p > 0 else torch.ones(())
    out = _bf(torch.einsum("hij,jhd->ihd", _bf(pr * dsc * mf), v))
    do = dout.float()
    dsum = (do * out).sum(-1).t()[..., None]  # [H, L, 1]
    dp = torch.einsum("ihd,jhd->hij", do, v) * dsc * mf
    ds = _bf(pr * (dp - dsum) * SCALE)
    pd = _bf(pr * dsc * mf)
    dq = torch.einsum("hij,jhd->ihd", ds, k)
    dk = torch.einsum("hij,ihd->jhd", ds, q)
    dv = torch.einsum("hij,ihd->jhd", pd, do)
    return _split(out, _bf(torch.stack((dq, dk, dv), 1)))


def _zfill(t, n):
    return torch.cat([t, torch.zeros(n - t.shape[0], *t.shape[1:], dtype=t.dtype)])


def _emulate_varlen(x, keep, p, dout, nxt=None, drop_last_query_tile=False):
    """The kernels' own order of operations on one sequence.

    Forward: K / V staged to l64 = ceil64(L) rows (zeros beyond L), 64-key chunks, running maximum from -3.0e38 and
    running sum, dead keys selected to -3.0e38, the unnormalised kept P rounded to bf16, out = o * (1 / (1 - p)) / l
    rounded; statistics m and log2 l per row. dq pass: the same chunks, P = exp2((s - m) log2e - log2 l) selected to 0
    for dead keys, dS rounded, D = rowsum(dO o O) from the rounded output. dkv pass: Q / dO staged to l64 rows, 64-query
    chunks, P of dead queries selected to 0, P_d and dS rounded.
    Mutants: nxt = (x, dout, m, log2 l, D) of the next sequence: the dkv pass stages its rows and statistics in the dead
    rows L .. l64 - 1 (as far as it has any) and does not select them to zero; drop_last_query_tile: the queries of the
    last partial 16-query tile left out of dk and dv."""
    L = x.shape[0]
    l64 = (L + 63) // 64 * 64
    q, k, v = (t.float() for t in x.unbind(1))
    do = dout.float()
    kz, vz = _zfill(k, l64), _zfill(v, l64)
    dsc = fb._drop_scale(p) if p > 0 else 1.0
    kp = torch.ones(H, l64, l64)  # keep[h, i, j]; dead rows / keys: never used unselected
    if p > 0:
        kp[:, :L, :L] = keep.float()
    live = torch.arange(l64) < L
    floor = torch.full((), -3.0e38)
    s = torch.where(live[None, None, :], torch.einsum("ihd,jhd->hij", q, kz) * SCALE, floor)
    m = torch.full((H, L, 1), -3.0e38)
    l = torch.zeros(H, L, 1)
    o = torch.zeros(H, L, DH)
    for c in range(0, l64, 64):
        sc = s[..., c:c + 64]
        mc = torch.maximum(m, sc.amax(-1, keepdim=True))
        alpha = torch.exp(m - mc)
        m, l, o = mc, l * alpha, o * alpha
        pe = torch.exp(sc - m)
        l = l + pe.sum(-1, keepdim=True)
        o = o + torch.einsum("hij,jhd->hid", _bf(pe * kp[:, :L, c:c + 64]), vz[c:c + 64])
    out = _bf(o * (dsc / l)).permute(1, 0, 2)
    l2 = torch.log2(l)
    dsum = (do * out).sum(-1).t()[..., None]  # [H, L, 1]
    # dq pass
    dq = torch.zeros(H, L, DH)
    for c in range(0, l64, 64):
        sc = torch.einsum("ihd,jhd->hij", q, kz[c:c + 64]) * SCALE
        pe = torch.where(live[None, None, c:c + 64], torch.exp2((sc - m) * LOG2E - l2), torch.zeros(()))
        dpv = torch.einsum("ihd,jhd->hij", do, vz[c:c + 64]) * dsc * kp[:, :L, c:c + 64]
        dq = dq + torch.einsum("hij,jhd->hid", _bf(pe * (dpv - dsum) * SCALE), kz[c:c + 64])
    # dkv pass: query rows staged to l64
    qz, doz = _zfill(q, l64), _zfill(do, l64)
    mz, lz, dz = (_zfill(t.permute(1, 0, 2), l64).permute(1, 0, 2) for t in (m, l2, dsum))
    qlive = live.clone()
    kq = kp
    if nxt is not None:
        nx, ndo, nm, nl, nd = nxt
        n = min(l64 - L, nx.shape[0])
        qz[L:L + n], doz[L:L + n] = nx[:n, 0].float(), ndo[:n].float()
        mz[:, L:L + n], lz[:, L:L + n], dz[:, L:L + n] = nm[:, :n], nl[:, :n], nd[:, :n]
        qlive[L:L + n] = True
    if drop_last_query_tile and L % 16 and L > 16:
        qlive[L // 16 * 16:] = False
    dk = torch.zeros(H, L, DH)
    dv = torch.zeros(H, L, DH)
    for c in range(0, l64, 64):
        sc = torch.einsum("ihd,jhd->hij", qz[c:c + 64], k) * SCALE
        pe = torch.where(qlive[None, c:c + 64, None], torch.exp2((sc - mz[:, c:c + 64]) * LOG2E - lz[:, c:c + 64]),
                         torch.zeros(()))
        kc = kq[:, c:c + 64, :L]
        pd = _bf(pe * dsc * kc)
        dpv = torch.einsum("ihd,jhd->hij", doz[c:c + 64], v) * dsc * kc
        ds = _bf(pe * (dpv - dz[:, c:c + 64]) * SCALE)
        dv = dv + torch.einsum("hij,ihd->hjd", pd, doz[c:c + 64])
        dk = dk + torch.einsum("hij,ihd->hjd", ds, qz[c:c + 64])
    dqkv = _bf(torch.stack((dq, dk, dv), 0)).permute(2, 0, 1, 3)  # [L, 3, H, 64]
    return _split(out, dqkv), (m, l2, dsum)


# ---- cases -----------------------------------------------------------------------------------------------------------
def _qkv(family, T, seed=0):
    """[T, 3, H, 64] bf16: the diffuse and peaky families of tests/test_attention.py."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(T, 3, H, DH, generator=g) * 0.7
    if family == "peaky":
        x[:, :2] *= 5 ** 0.5 / 0.7
    else:
        assert family == "diffuse"
    return x.bfloat16()


def _keep(rows, row0, L, p, packed_row=True):
    return av.seq_keep_mask(rows, row0 if packed_row else 0, L, range(H0, H0 + H), _rng_cpu(), SITE, p)


@functools.lru_cache(maxsize=None)
def _case(order, family, p):
    """The pack, and per sequence the float64 reference and the emulation's E; computed once, shared, not modified."""
    lengths, spare = _order(order, family)
    T = sum(lengths)
    rows = T + spare
    qkv = _zfill(_qkv(family, T), rows)
    dout = _zfill(torch.randn(T, H, DH, generator=torch.Generator().manual_seed(T + 1)).bfloat16(), rows)
    sl = _slices(lengths)
    keeps = [_keep(rows, s.start, s.stop - s.start, p) if p > 0 else None for s in sl]
    ref = [_ref64(qkv[s], kp, p, dout[s]) for s, kp in zip(sl, keeps)]
    emu = [_emulate(qkv[s], kp, p, dout[s]) for s, kp in zip(sl, keeps)]
    return types.SimpleNamespace(order=order, family=family, p=p, lengths=lengths, rows=rows, T=T, qkv=qkv, dout=dout,
                                 sl=sl, keeps=keeps, ref=ref, emu=emu)


CASES = [(o, f, p) for o in ORDERS for f in LENGTHS for p in (0.0, 0.1)]


# ---- metric and bound ------------------------------------------------------------------------------------------------
def _tile_norms(x):
    """L2 norms over (16 consecutive tokens, head dim) of [L, H, 64] -> [ceil(L / 16), H]; the last tile may be
    partial."""
    pad = (-x.shape[0]) % TILE
    x = torch.cat([x.double(), torch.zeros(pad, *x.shape[1:], dtype=torch.float64)])
    return x.reshape(-1, TILE, H, DH).pow(2).sum((1, 3)).sqrt()


def _tile_err(got, ref, top):
    n = _tile_norms(ref)
    return _tile_norms(got.double() - ref.double()) / torch.where(n >= TINY * top, n, top)


def _measure(c, got, margin=MARGIN):
    """got: per sequence a dict of out / dq / dk / dv [L, H, 64]. Per tensor: (worst excess err - (margin E + FLOOR)
    over every tile of every sequence, the margin needed, the plain max of err / E over tiles with E >= FLOOR). A
    non-finite error counts as an infinite excess."""
    res = {}
    for name in NAMES:
        top = max(float(_tile_norms(r[name]).max()) for r in c.ref)
        worst, need, plain = -math.inf, 0.0, 0.0
        for g, e_, r in zip(got, c.emu, c.ref):
            err, e = _tile_err(g[name], r[name], top), _tile_err(e_[name], r[name], top)
            if not bool(torch.isfinite(err).all()):
                worst = need = math.inf
                continue
            worst = max(worst, float((err - (margin * e + FLOOR)).max()))
            need = max(need, float(((err - FLOOR).clamp(min=0) / e.clamp(min=1e-30)).max()))
            big = e >= FLOOR
            if bool(big.any()):
                plain = max(plain, float((err[big] / e[big]).max()))
        res[name] = (worst, need, plain)
    return res


def _report(tag, res):
    for name, (worst, need, plain) in res.items():
        print(f"VARLEN_TRAIN_RATIO {tag} tensor={name} need={need:.3f} plain={plain:.3f} excess={worst:.3e}")


def _tag(c):
    return f"case={c.order}/{c.family}/p{c.p}"


# ---- CPU: the reference op ---------------------------------------------------------------------------------------------
def test_keep_index_is_the_documented_one():
    """seq_keep_mask / keep_at are fb.keep_mask at (g * rows + t) * 512 + j, and multiples of 4 stay groups of 4."""
    rows, lengths, p = 40, [3, 17, 9], 0.3
    full = fb.keep_mask((H + 2) * rows * 512, _rng_cpu(), SITE, p).view(H + 2, rows, 512)
    for s in _slices(lengths):
        L = s.stop - s.start
        assert torch.equal(_keep(rows, s.start, L, p), full[H0:H0 + H, s, :L])
    assert 0.2 < 1 - full.float().mean() < 0.4


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_reference_op_is_per_sequence_attention(p):
    """attention_varlen on CPU tensors (the reference op) equals fb.attention_reference on each sequence cut out and
    run alone (p = 0), and the same composition with the mask taken at the documented index (p > 0): values and
    gradients; rows of no sequence are zero and get zero gradient."""
    lengths, rows = [5, 1, 33, 16], 64
    T = sum(lengths)
    qkv = _zfill(_qkv("peaky", T, seed=3), rows).float()
    qkv[T:] = 7.0  # rows of no sequence: never read
    dout = torch.randn(rows, H, DH, generator=torch.Generator().manual_seed(2))
    cu = torch.tensor(bi.cu_seqlens(lengths) + [T, T], dtype=torch.int32)
    table = torch.tensor(bi.block_table(lengths), dtype=torch.int32)
    x = qkv.clone().requires_grad_()
    out = av.attention_varlen(x, cu, table, len(lengths) + 2, 64, SCALE, p, _rng_cpu(), SITE, H0, H + 2)
    out.backward(dout)
    assert out.shape == (rows, H, DH) and bool((out[T:] == 0).all()) and bool((x.grad[T:] == 0).all())
    full = fb.keep_mask((H + 2) * rows * 512, _rng_cpu(), SITE, p).view(H + 2, rows, 512) if p > 0 else None
    for s in _slices(lengths):
        L = s.stop - s.start
        y = qkv[s].clone().requires_grad_()
        if p == 0:
            want = fb.attention_reference(y[None], None, SCALE)[0]
        else:
            pr = torch.softmax(torch.einsum("ihd,jhd->hij", y[:, 0], y[:, 1]) * SCALE, -1)
            pr = torch.where(full[H0:H0 + H, s, :L], pr * fb._drop_scale(p), torch.zeros(()))
            want = torch.einsum("hij,jhd->ihd", pr, y[:, 2])
        want.backward(dout[s])
        torch.testing.assert_close(out[s], want, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(x.grad[s], y.grad, rtol=1e-5, atol=1e-6)
    r64 = av.attention_varlen_reference(qkv, cu, len(lengths), SCALE, p, _rng_cpu(), SITE, H0, H + 2,
                                        dtype=torch.float64)
    assert r64.dtype == torch.float64
    torch.testing.assert_close(r64.float(), out.detach(), rtol=1e-5, atol=1e-6)


def test_op_argument_errors():
    qkv = torch.zeros(8, 3, H, DH)
    cu, table = torch.tensor([0, 8], dtype=torch.int32), torch.tensor([[0, 0]], dtype=torch.int32)
    with pytest.raises(ValueError, match="rng"):
        av.attention_varlen(qkv, cu, table, 1, 8, SCALE, 0.1)
    with pytest.raises(ValueError, match="longest"):
        av.attention_varlen(qkv, cu, table, 1, 513, SCALE)
    with pytest.raises(ValueError, match="outside"):
        av.attention_varlen(qkv, cu, table, 1, 8, SCALE, 1.0, _rng_cpu())
    with pytest.raises(ValueError, match="rows, 3"):
        av.attention_varlen(qkv[:, :2], cu, table, 1, 8, SCALE)


# ---- CPU: the bound and its sensitivity ----------------------------------------------------------------------------------
def _emu_varlen_all(c, **mutant):
    """_emulate_varlen over the pack. mutant: next_stats / drop_last_query_tile / seq_row_mask."""
    keeps = c.keeps
    if mutant.get("seq_row_mask"):
        keeps = [_keep(c.rows, s.start, s.stop - s.start, c.p, packed_row=False) for s in c.sl]
    plain = [_emulate_varlen(c.qkv[s], kp, c.p, c.dout[s]) for s, kp in zip(c.sl, keeps)]
    if mutant.get("next_stats"):
        got = []
        for b, (s, kp) in enumerate(zip(c.sl, keeps)):
            nxt = None
            if b + 1 < len(c.sl):
                n = c.sl[b + 1]
                nxt = (c.qkv[n], c.dout[n]) + plain[b + 1][1]
            got.append(_emulate_varlen(c.qkv[s], kp, c.p, c.dout[s], nxt=nxt)[0])
        return got
    if mutant.get("drop_last_query_tile"):
        return [_emulate_varlen(c.qkv[s], kp, c.p, c.dout[s], drop_last_query_tile=True)[0]
                for s, kp in zip(c.sl, keeps)]
    return [g for g, _ in plain]


@pytest.mark.parametrize("order,family,p", CASES)
def test_emulation_in_kernel_order_within_bound(order, family, p):
    c = _case(order, family, p)
    res = _measure(c, _emu_varlen_all(c))
    _report("emulation " + _tag(c), res)
    assert all(w <= 0 for w, _, _ in res.values()), res


@pytest.mark.parametrize("family", ["diffuse", "peaky"])
def test_mutant_dead_queries_on_next_sequence(family):
    """a. dk and dv leave the bound (margin 4); out and dq, which the dkv pass does not write, do not."""
    c = _case("head13", family, 0.0)
    res = _measure(c, _emu_varlen_all(c, next_stats=True), margin=4)
    assert res["dk"][0] > 0 and res["dv"][0] > 0 and res["out"][0] <= 0 and res["dq"][0] <= 0, res


@pytest.mark.parametrize("family", ["diffuse", "peaky"])
def test_mutant_last_partial_query_tile_dropped(family):
    """b."""
    c = _case("head13", family, 0.0)
    res = _measure(c, _emu_varlen_all(c, drop_last_query_tile=True), margin=4)
    assert res["dk"][0] > 0 and res["dv"][0] > 0, res


@pytest.mark.parametrize("family", ["diffuse", "peaky"])
def test_mutant_mask_indexed_by_row_in_sequence(family):
    """c. every tensor leaves the bound (the sequence at packed row 0 alone is unchanged)."""
    c = _case("head13", family, 0.1)
    res = _measure(c, _emu_varlen_all(c, seq_row_mask=True), margin=4)
    assert all(w > 0 for w, _, _ in res.values()), res


# ---- CPU: the packed model ---------------------------------------------------------------------------------------------
def _cfg(**kw):
    d = dict(vocab_size=512, hidden=128, heads=2, intermediate=256, layers=2, max_position=512, dropout=0.0)
    d.update(kw)
    return BertConfig(**d)


def _model64():
    """float64 throughout: fused_attention=False, as the fused attention's CPU reference computes in float32."""
    m = BertForSequenceClassification(_cfg(fused_attention=False), None, seed=None)
    m.load_full(full_init_state(_cfg(), 0))
    return m.double().train()


MODEL_LENGTHS = [5, 1, 33, 16, 20, 7]


def _model_batch(lengths=MODEL_LENGTHS):
    g = np.random.default_rng(3)
    seqs = [g.integers(0, 512, size=L) for L in lengths]
    tts = [np.array([0] * (L // 2) + [1] * (L - L // 2)) for L in lengths]
    return seqs, tts, g.integers(0, 2, size=len(lengths))


def _packed_inputs(seqs, tts, labels, C, max_seqs, device="cpu"):
    from mifx.models import bert_infer as M

    p = M.pack(seqs, tts, C, max_seqs)
    p.ids[p.tokens:] = 0
    y = np.full(max_seqs, -100, np.int64)
    y[:len(seqs)] = labels
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    return (t(p.ids), t(p.tts), t(p.pos), t(p.cu), t(p.table), max_seqs, 64, t(p.first)), t(y)


def _packed_grads(m, seqs, tts, labels, C, max_seqs, mutate=None):
    m.zero_grad()
    args, y = _packed_inputs(seqs, tts, labels, C, max_seqs)
    if mutate:
        args = mutate(args)
    loss = F.cross_entropy(m.forward_packed(*args), y, ignore_index=-100)
    loss.backward()
    return float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters()}


def _per_sequence_grads(m, seqs, tts, labels):
    m.zero_grad()
    logits = torch.cat([m(torch.tensor(s)[None], torch.tensor(t)[None]) for s, t in zip(seqs, tts)])
    loss = F.cross_entropy(logits, torch.from_numpy(labels))
    loss.backward()
    return float(loss.detach()), {n: p.grad.clone() for n, p in m.named_parameters()}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def test_packed_model_equals_per_sequence_model_float64():
    """Loss and every parameter gradient of forward_packed against the unpadded model run per sequence, float64,
    dropout 0: 1e-9 relative (only the order of sums differs). Wrong position ids or CLS rows show at 1e-3 or more."""
    m = _model64()
    seqs, tts, y = _model_batch()
    T = sum(MODEL_LENGTHS)
    l0, g0 = _per_sequence_grads(m, seqs, tts, y)
    l1, g1 = _packed_grads(m, seqs, tts, y, T, len(seqs))
    assert abs(l1 - l0) <= 1e-9 * abs(l0)
    worst = max(_rel(g1[n], g0[n]) for n in g0)
    assert worst <= 1e-9, worst

    def no_restart(a):  # position ids that run on over the pack
        return a[:2] + (torch.arange(T, dtype=torch.int32),) + a[3:]

    def cls_off(a):  # CLS rows one off from the second sequence on
        return a[:7] + ((a[7] + (a[7] > 0)).to(a[7].dtype),)

    for bad in (no_restart, cls_off):
        l2, g2 = _packed_grads(m, seqs, tts, y, T, len(seqs), mutate=bad)
        assert max(abs(l2 - l0) / abs(l0), max(_rel(g2[n], g0[n]) for n in g0)) >= 1e-3, bad.__name__


def test_padding_rows_and_empty_slots_change_no_gradient_float64():
    m = _model64()
    seqs, tts, y = _model_batch()
    T = sum(MODEL_LENGTHS)
    l0, g0 = _packed_grads(m, seqs, tts, y, T, len(seqs))
    l1, g1 = _packed_grads(m, seqs, tts, y, T + 46, len(seqs) + 5)
    assert abs(l1 - l0) <= 1e-9 * abs(l0)
    assert max(_rel(g1[n], g0[n]) for n in g0) <= 1e-9


def test_packed_path_refuses_tensor_parallelism():
    from mifx.trainer.bert_trainer import BertTrainer

    m = BertForSequenceClassification(_cfg(), None, seed=None)
    m.tp = types.SimpleNamespace(size=2, rank=0)
    seqs, tts, y = _model_batch()
    args, _ = _packed_inputs(seqs, tts, y, 128, 8)
    with pytest.raises(ValueError, match="TP = 1"):
        m.forward_packed(*args)
    with pytest.raises(ValueError, match="TP = 1"):
        BertTrainer(_cfg(), 8, 64, "cpu", tp=types.SimpleNamespace(size=2, rank=0, ipc=None), packed_tokens=128)
    with pytest.raises(ValueError, match="sequence parallelism"):
        BertTrainer(_cfg(sequence_parallel=True), 8, 64, "cpu", packed_tokens=128)


def test_set_packed_batch_and_planner_validation():
    from mifx.trainer.bert_trainer import BertTrainer, plan_train_batches

    assert list(plan_train_batches([60, 60, 60, 5, 128, 1, 1, 1], 128, 3)) == [[0, 1], [2, 3], [4], [5, 6, 7]]
    with pytest.raises(ValueError, match="above the token capacity"):
        list(plan_train_batches([10, 200], 128, 4))
    with pytest.raises(ValueError, match="empty"):
        list(plan_train_batches([10, 0], 128, 4))
    with pytest.raises(ValueError, match="positive"):
        list(plan_train_batches([10], 128, 0))
    with pytest.raises(ValueError, match="max_len"):
        BertTrainer(_cfg(), 8, 64, "cpu", packed_tokens=1024, max_len=513)
    with pytest.raises(ValueError, match="packed_tokens"):
        BertTrainer(_cfg(), 8, 64, "cpu", max_seqs=4)
    tr = BertTrainer(_cfg(), 8, 64, "cpu", packed_tokens=128, max_seqs=4)
    assert tr.packed and tr.max_len == 64 and tr.packed_batch == (128, 2)
    ok = [[1, 2, 3], [4, 5]]
    for seqs, tts, y, word in [
        ([[1] * 65], None, [0], "max_len"),
        ([[1] * 40] * 4, None, [0] * 4, "packed_tokens"),
        ([[1]] * 5, None, [0] * 5, "max_seqs"),
        ([[1, 2], []], None, [0, 1], "sequence 1"),
        ([[1, 512]], None, [0], "vocabulary"),
        (ok, [[0, 0, 2], None], [0, 1], "token type"),
        (ok, None, [0], "labels"),
        (ok, None, [0, 2], "label outside"),
        ([], None, [], "at least one"),
    ]:
        with pytest.raises(ValueError, match=word):
            tr.set_packed_batch(seqs, tts, y)
    tr.set_packed_batch(ok, [[0, 1, 1], None], [1, 0])
    v = tr.pviews
    assert tr.packed_batch == (5, 2) and v.ids[:7].tolist() == [1, 2, 3, 4, 5, 0, 0]
    assert v.pos[:6].tolist() == [0, 1, 2, 0, 1, 0] and v.first.tolist() == [0, 3, 0, 0]
    assert tr.plabels.tolist() == [1, 0, -100, -100] and v.cu.tolist() == [0, 3, 5, 5, 5]
    assert math.isfinite(float(tr.step()))  # the CPU reference path trains
    with pytest.raises(ValueError, match="packed_tokens"):
        BertTrainer(_cfg(), 8, 64, "cpu").set_packed_batch(ok, None, [0, 1])


# ---- GPU: the kernels ---------------------------------------------------------------------------------------------------
def _tables(lengths, nseq_pad=0, listed=None):
    cu = bi.cu_seqlens(lengths)
    cu = cu + [cu[-1]] * nseq_pad
    tab = [e for e in bi.block_table(lengths) if listed is None or e[0] in listed]
    return (torch.tensor(cu, dtype=torch.int32, device="cuda"),
            torch.tensor(tab, dtype=torch.int32, device="cuda").reshape(-1, 2))


def _direct(qkv, dout, cu, table, nseq, lmax, p, fill=0.0):
    """The entry points called directly: out, stats and dsum prefilled with `fill`, dqkv zeroed."""
    rows = qkv.shape[0]
    out = torch.full((rows, H, DH), fill, device="cuda", dtype=torch.bfloat16)
    stats = torch.full((2, H, rows), fill, device="cuda")
    dsum = torch.full((H, rows), fill, device="cuda")
    dqkv = torch.zeros_like(qkv)
    rng = torch.tensor(SEED_CTR, dtype=torch.int64, device="cuda")
    r, st = fb.ptr(rng if p > 0 else None), fb.stream_handle(qkv.device)
    fb.check(av._fns()["fwd"](fb.ptr(qkv), fb.ptr(cu), fb.ptr(table), nseq, table.shape[0], rows, lmax, H, H0, SCALE,
                              p, r, SITE, fb.ptr(out), fb.ptr(stats), st), "fwd")
    fb.check(av._fns()["bwd"](fb.ptr(qkv), fb.ptr(cu), fb.ptr(table), nseq, table.shape[0], rows, lmax, H, H0, SCALE,
                              p, r, SITE, fb.ptr(out), fb.ptr(dout), fb.ptr(stats), fb.ptr(dqkv), fb.ptr(dsum), st),
             "bwd")
    torch.cuda.synchronize()
    return out, stats, dqkv, dsum


@pytest.mark.gpu
@pytest.mark.parametrize("order,family,p", CASES)
def test_attn_varlen_train_gpu(order, family, p):
    """Forward and backward through the autograd op against the bound, per tile of every sequence."""
    from mifx.ops import native_stats

    c = _case(order, family, p)
    cu, table = _tables(c.lengths)
    qkv = c.qkv.cuda().requires_grad_()
    rng = torch.tensor(SEED_CTR, dtype=torch.int64, device="cuda")
    native_stats.reset()
    out = av.attention_varlen(qkv, cu, table, len(c.lengths), 512, SCALE, p, rng, SITE, H0, H + 2)
    assert native_stats.snapshot()["attention_varlen"] == {"native": 1, "fallback": 0}
    out.backward(c.dout.cuda())
    o, g = out.detach().float().cpu(), qkv.grad.float().cpu()
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(g).all())
    assert bool((o[c.T:] == 0).all()) and bool((g[c.T:] == 0).all())
    res = _measure(c, [_split(o[s], g[s]) for s in c.sl])
    _report("kernels " + _tag(c), res)
    assert all(w <= 0 for w, _, _ in res.values()), res


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [float("nan"), 1e30])
@pytest.mark.parametrize("L", [17, 130])
@pytest.mark.parametrize("where", ["start", "middle", "end"])
def test_attn_varlen_train_inert_rows_gpu(where, L, poison):
    """Rows of qkv, out, dout, the statistics and dsum that belong to no sequence, and the rows of the two neighbouring
    sequences when they are left out of the table, hold NaN or 1e30: the listed sequence's out and dqkv are
    bit-identical to the clean run, every other dqkv row is still zero and every other out row untouched."""
    lengths = {"start": [L, 40, 23], "middle": [40, L, 23], "end": [40, 23, L]}[where]
    b = lengths.index(L)
    T, rows = sum(lengths), sum(lengths) + 24
    s = _slices(lengths)[b]
    qkv = _zfill(_qkv("peaky", T, seed=L), rows).cuda()
    dout = _zfill(torch.randn(T, H, DH, generator=torch.Generator().manual_seed(L)).bfloat16(), rows).cuda()
    cu, table = _tables(lengths)
    want = _direct(qkv, dout, cu, table, 3, 192, 0.1)
    mine = torch.zeros(rows, dtype=torch.bool, device="cuda")
    mine[s] = True
    q2, d2 = qkv.clone(), dout.clone()
    q2[~mine] = poison
    d2[~mine] = poison
    cu, table = _tables(lengths, listed={b})
    got = _direct(q2, d2, cu, table, 3, 192, 0.1, fill=poison)
    assert torch.equal(got[0][s], want[0][s]) and torch.equal(got[2][s], want[2][s])
    assert bool(torch.isfinite(want[2].float()).all()) and bool((want[2][T:] == 0).all())
    assert bool((got[2][~mine] == 0).all())
    rest = got[0][~mine].float()
    assert bool(torch.isnan(rest).all()) if math.isnan(poison) else bool((rest == float(torch.tensor(poison).bfloat16())).all())


@pytest.mark.gpu
def test_attn_varlen_train_deterministic_gpu():
    c = _case("tail512_1", "peaky", 0.1)
    cu, table = _tables(c.lengths)
    runs = [_direct(c.qkv.cuda(), c.dout.cuda(), cu, table, len(c.lengths), 512, 0.1) for _ in range(2)]
    for name, a, b in zip(("out", "stats", "dqkv", "dsum"), *runs):
        assert torch.equal(a, b), name


@pytest.mark.gpu
def test_attn_varlen_train_padding_entries_and_lmax_gpu():
    """A table with -1 entries between and after the live ones gives the same bits; a sequence longer than lmax is
    skipped, its rows left untouched, and its neighbours are computed as before."""
    lengths = [70, 130, 20]
    T = sum(lengths)
    sl = _slices(lengths)
    qkv = _qkv("diffuse", T, seed=9).cuda()
    dout = torch.randn(T, H, DH, generator=torch.Generator().manual_seed(9)).bfloat16().cuda()
    cu, table = _tables(lengths, nseq_pad=2)
    want = _direct(qkv, dout, cu, table, 5, 192, 0.1)
    holes = torch.full((9, 2), -1, dtype=torch.int32, device="cuda")
    holes[torch.tensor([1, 3, 4, 6], device="cuda")] = table
    got = _direct(qkv, dout, cu, holes, 5, 192, 0.1)
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2])
    short = _direct(qkv, dout, cu, table, 5, 128, 0.1, fill=3.0)
    for b in (0, 2):
        assert torch.equal(short[0][sl[b]], want[0][sl[b]]) and torch.equal(short[2][sl[b]], want[2][sl[b]])
    assert bool((short[0][sl[1]] == 3.0).all()) and bool((short[2][sl[1]] == 0).all())
    assert bool((short[1][:, :, sl[1]] == 3.0).all()) and bool((short[3][:, sl[1]] == 3.0).all())


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments_gpu():
    qkv = torch.zeros(64, 3, H, DH, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros(64, H, DH, device="cuda", dtype=torch.bfloat16)
    stats = torch.zeros(2, H, 64, device="cuda")
    cu, table = _tables([64])
    st = fb.stream_handle(qkv.device)

    def fwd(q=qkv, lmax=64, nent=1, p=0.0, rng=None):
        return av._fns()["fwd"](fb.ptr(q), fb.ptr(cu), fb.ptr(table), 1, nent, 64, lmax, H, 0, SCALE, p, fb.ptr(rng),
                                0, fb.ptr(out), fb.ptr(stats), st)

    assert fwd() == 0
    assert fwd(q=qkv.view(-1)[4:]) == -1 and fwd(lmax=0) == -1 and fwd(lmax=513) == -1
    assert fwd(nent=2 ** 30 + 1) == -1 and fwd(p=1.0) == -1 and fwd(p=-0.1) == -1 and fwd(p=0.1) == -1
    torch.cuda.synchronize()


# ---- GPU: the trainer ---------------------------------------------------------------------------------------------------
def _seqs_of(lengths, seed):
    g = np.random.default_rng(seed)
    return ([g.integers(0, 512, size=L) for L in lengths], [np.array([0] * (L // 2) + [1] * (L - L // 2)) for L in lengths],
            g.integers(0, 2, size=len(lengths)))


@pytest.mark.gpu
def test_packed_trainer_captured_equals_eager_gpu():
    """Three steps with dropout 0.1, a different batch set before each: one leaves padding rows and empty slots, one
    fills the capacity exactly, one fills every slot. hipGraph against graph=False: losses and weights bit for bit."""
    from mifx.trainer.bert_trainer import BertTrainer

    cfg = _cfg(dropout=0.1)
    kw = dict(lr=1e-3, packed_tokens=512, max_seqs=8, max_len=192)
    eager = BertTrainer(cfg, 8, 64, "cuda", graph=False, **kw)
    graphed = BertTrainer(cfg, 8, 64, "cuda", graph=True, **kw)
    batches = [_seqs_of([17, 130, 64, 1], 1), _seqs_of([128, 128, 128, 65, 63], 2),
               _seqs_of([100, 3, 50, 60, 70, 15, 16, 33], 3)]
    eager.set_packed_batch(*batches[0])
    for _ in range(3):  # the capture's warm-up steps, on the first batch
        eager.step()
    le, lg = [], []
    for b in batches:
        for tr, ls in ((eager, le), (graphed, lg)):
            tr.set_packed_batch(*b)
            ls.append(float(tr.step()))
    assert graphed.graph is not None and eager.graph is None
    assert graphed.packed_batch == (347, 8) and all(math.isfinite(v) for v in lg)
    assert le == lg, (le, lg)
    for (n, a), (_, b) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
        assert torch.equal(a, b), n
    # the pinned gradient-address table the captured step copies in on every replay is still the optimizer's own
    assert graphed.opt._captured_table.tolist() == list(graphed.opt._addr)


def _bf16_ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


@pytest.mark.gpu
def test_packed_trainer_step_against_padded_gpu():
    """One forward + backward of the packed trainer's step from equal weights on 8 sequences, dropout 0, against the
    fp32 CPU model run per sequence: the loss, and the gradients of the classifier weight, layer 0's qkv.weight and the
    touched word-embedding rows, within 2 x the error of the existing padded bf16 trainer (S = 128, attention mask)
    plus one bf16 ulp of the largest reference element."""
    from mifx.models import bert_infer as M
    from mifx.trainer.bert_trainer import BertTrainer

    cfg = _cfg()
    lengths = [17, 128, 1, 64, 100, 33, 90, 48]
    seqs, tts, y = _seqs_of(lengths, 5)
    names = ("classifier.weight", "layers.0.qkv.weight", "word.weight")
    touched = torch.from_numpy(np.unique(np.concatenate(seqs)))

    def pick(model, loss):
        g = dict(model.named_parameters())
        return [loss.detach().float().cpu().reshape(1)] + [
            (g[n].grad.float().cpu()[touched] if n == "word.weight" else g[n].grad.float().cpu()) for n in names]

    def run(tr):
        tr.opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, cache_enabled=False):
            if tr.packed:
                v = tr.pviews
                logits = tr.model.forward_packed(v.ids, v.tts, v.pos, v.cu, v.table, tr.max_seqs, tr.max_len, v.first)
                loss = F.cross_entropy(logits.float(), tr.plabels.long(), ignore_index=-100)
            else:
                logits = tr.model(*tr.data[:3])
                loss = F.cross_entropy(logits.float(), tr.data[3])
        loss.backward()
        return pick(tr.model, loss)

    packed = BertTrainer(cfg, 8, 128, "cuda", graph=False, packed_tokens=512, max_seqs=12)
    packed.set_packed_batch(seqs, tts, y)
    padded = BertTrainer(cfg, 8, 128, "cuda", graph=False)
    padded.set_batch(*(torch.from_numpy(a) for a in M._pad_arrays(seqs, tts, 128)), torch.from_numpy(y))
    ref = BertForSequenceClassification(cfg, None, seed=None)
    ref.load_state_dict({k: v.float().cpu() for k, v in packed.model.state_dict().items()}, strict=False)
    ref.train()
    logits = torch.cat([ref(torch.tensor(s)[None], torch.tensor(t)[None]) for s, t in zip(seqs, tts)])
    loss = F.cross_entropy(logits, torch.from_numpy(y))
    loss.backward()
    want, got, pad = pick(ref, loss), run(packed), run(padded)
    bad = []
    for n, w, g, e in zip(("loss",) + names, want, got, pad):
        err, e_pad = float((g - w).abs().max()), float((e - w).abs().max())
        bound = 2 * e_pad + _bf16_ulp(float(w.abs().max()))
        print(f"PACKED_TRAIN_E2E tensor={n} packed_err={err:.3e} E_pad={e_pad:.3e} bound={bound:.3e}")
        if not err <= bound:
            bad.append(n)
    assert not bad, bad


@pytest.mark.gpu
def test_component_packed_tokens_gpu(tmp_path):
    """The BertTrainer component with custom_config["packed_tokens"] on the synthetic examples runs, exports, and
    records the new keys."""
    from safetensors.torch import load_file

    from mifx.components import EvalArgs, TrainArgs
    from mifx.components.bert import BertTrainer, TextExampleGen
    from mifx.orchestration import LocalDagRunner, Pipeline

    eg = TextExampleGen(num_synthetic=240, seq_len=64, vocab_size=512, num_labels=2, seed=3)
    tr = BertTrainer(examples=eg.outputs.examples, train_args=TrainArgs(num_steps=12), eval_args=EvalArgs(num_steps=2),
                     custom_config=dict(vocab_size=512, hidden=128, layers=2, heads=2, intermediate=256, max_position=64,
                                        dropout=0.1, tp=1, batch_size=8, learning_rate=1e-3, packed_tokens=512))
    p = Pipeline(pipeline_name="packed", pipeline_root=str(tmp_path / "packed"), components=[eg, tr],
                 metadata_db_root=str(tmp_path / "md"))
    res = LocalDagRunner(device="cuda").run(p)
    assert res.succeeded
    art = res.components["BertTrainer"].outputs["output"][0]
    m = json.load(open(os.path.join(art.uri, "metrics.json")))
    pk = m["packed"]
    assert pk["packed_tokens"] == 512 and pk["max_seqs"] == 32
    assert 512 / 64 <= pk["mean_sequences_per_step"] <= 512 / 32 and 0.15 < pk["padded_padding_share"] < 0.35
    assert all(math.isfinite(v) for v in m["losses"]) and 0.0 <= m["eval"]["accuracy"] <= 1.0
    sd = load_file(os.path.join(m["export"], "variables.safetensors"))
    assert sd["word.weight"].shape == (512, 128) and all(bool(torch.isfinite(v).all()) for v in sd.values())
