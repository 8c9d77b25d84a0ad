"""Packed variable-length BERT inference (csrc/bert_infer.hip, mifx/models/bert_infer.py).

Attention. `mifx_attn_fwd_varlen` is compared per (sequence, head, 16-token tile) with `_ref64`, attention written
from its definition in float64 on the bf16-rounded inputs of one sequence alone. The bound is the rule of
tests/test_attention.py, whose long forward this kernel derives from:

    err_tile <= MARGIN * E_tile + FLOOR,    MARGIN = 3, FLOOR = 2^-9

err is the tile's L2 error relative to the tile's L2 norm in the reference (the last tile of a sequence holds its
L % 16 remaining rows), E the same error of `_emulate`, the computation in float32 with bf16 rounding of P and of the
output. E comes from the emulation, never from a kernel. `_emulate_varlen` is the kernel's own order of operations
(64-key chunks, keys at or beyond L selected to the floor -3.0e38, zero-filled V rows, the unnormalised P rounded); it
stays within the bound on the CPU, and three wrong variants do not (one padding key left unmasked with score 0; the
last partial 16-key tile dropped; for the embedding, positions that do not restart at a sequence boundary).

Margin the kernel needs, measured on an MI355X over every case of this file (max over tiles of (err - FLOOR) / E, in
brackets the plain max of err / E over tiles with E >= FLOOR): 0.34 (1.12); diffuse 0.34 (1.07) shuffled and 0.27
(1.12) with the 512- and 1-token sequences last, peaky 0.11 (0.94) and 0.00 (0.88).

End to end. The packed forward's logits against the fp32 CPU model run per sequence, unpadded, must be within
2 * E_pad + one bf16 ulp of the largest |logit|, E_pad being the same error of the existing padded bf16 eval forward
(fused kernels, S = 128, attention mask). Measured on an MI355X (24 sequences of 1 .. 128 tokens): packed 5.2e-04,
E_pad 5.9e-04, bound 1.66e-03."""
import functools
import math

import numpy as np
import pytest
import torch

from mifx.models import bert_infer as M
from mifx.models.bert import BertConfig, BertForSequenceClassification, full_init_state
from mifx.ops import bert_infer as bi

DH = 64
SCALE = DH ** -0.5
TILE = 16
FLOOR = 2.0 ** -9
MARGIN = 3
TINY = 1e-6
H = 2
LENGTHS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 320, 512]


def _cfg():
    return BertConfig(vocab_size=512, hidden=128, heads=2, intermediate=256, layers=2, max_position=512)


@functools.lru_cache(maxsize=None)
def _state():
    return full_init_state(_cfg(), 0)


def _bf(t):
    return t.bfloat16().float()


def _orders():
    """Two pack orders: shuffled, and one with the 512-token and then the 1-token sequence last."""
    g = torch.Generator().manual_seed(11)
    shuffled = [LENGTHS[i] for i in torch.randperm(len(LENGTHS), generator=g).tolist()]
    rest = [L for L in shuffled if L not in (1, 512)]
    return {"shuffled": shuffled, "tail512_1": rest + [512, 1]}


def _qkv(family, lengths, seed=0):
    """[T, 3, H, 64] bf16 with exactly T rows: the diffuse and peaky families of tests/test_attention.py."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn(sum(lengths), 3, H, DH, generator=g) * 0.7
    if family == "peaky":
        x[:, :2] *= 5 ** 0.5 / 0.7
    else:
        assert family == "diffuse"
    return x.bfloat16()


# ---- references (one sequence: x [L, 3, H, 64]) -------------------------------------------------------------------
def _ref64(x):
    q, k, v = x.double().unbind(1)
    s = torch.einsum("ihd,jhd->hij", q, k) * SCALE
    return torch.einsum("hij,jhd->ihd", torch.softmax(s, -1), v)


def _emulate(x):
    """float32, P rounded to bf16 before P V, the output rounded to bf16 (the yardstick of tests/test_attention.py)."""
    q, k, v = x.float().unbind(1)
    s = torch.einsum("ihd,jhd->hij", q, k) * SCALE
    return _bf(torch.einsum("hij,jhd->ihd", _bf(torch.softmax(s, -1)), v))


def _emulate_varlen(x, unmasked_pad_key=False, drop_last_tile=False):
    """The kernel's order: K / V staged to ceil64(L) rows (zeros beyond L), 64-key chunks with a running maximum
    from -3.0e38 and a running sum, keys >= L selected to -3.0e38, the unnormalised P rounded to bf16, the output
    rounded. Mutants: key L (a zero staging row, score 0) left unmasked; keys of the last partial 16-key tile masked."""
    L = x.shape[0]
    l64 = (L + 63) // 64 * 64
    q = x[:, 0].float()
    k = torch.zeros(l64, H, DH)
    v = torch.zeros(l64, H, DH)
    k[:L], v[:L] = x[:, 1].float(), x[:, 2].float()
    live = torch.arange(l64) < L
    if unmasked_pad_key and L < l64:
        live[L] = True
    if drop_last_tile and L % 16 and L > 16:
        live[L // 16 * 16:] = False
    s = torch.einsum("ihd,jhd->hij", q, k) * SCALE
    s = torch.where(live[None, None, :], s, torch.full((), -3.0e38))
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
        o = o + torch.einsum("hij,jhd->hid", _bf(pe), v[c:c + 64])
    return _bf(o / l).permute(1, 0, 2)


# ---- metric and bound (per sequence) ------------------------------------------------------------------------------
def _tile_norms(x):
    """L2 norms over (16 consecutive tokens, head dim) of [L, H, 64] -> [ceil(L / 16), H]; the last tile may be
    partial."""
    L = x.shape[0]
    pad = (-L) % TILE
    x = torch.cat([x.double(), torch.zeros(pad, *x.shape[1:], dtype=torch.float64)])
    return x.reshape(-1, TILE, H, DH).pow(2).sum((1, 3)).sqrt()


def _tile_err(got, ref):
    n = _tile_norms(ref)
    top = n.max()
    return _tile_norms(got.double() - ref.double()) / torch.where(n >= TINY * top, n, top)


def _seq_slices(lengths):
    cu = bi.cu_seqlens(lengths)
    return [slice(cu[b], cu[b + 1]) for b in range(len(lengths))]


def _check_pack(tag, got, qkv, lengths, margin=MARGIN):
    """Worst excess err - (margin E + FLOOR) over every tile of every sequence, and the margin needed."""
    worst, need, plain = -1.0, 0.0, 0.0
    for b, sl in enumerate(_seq_slices(lengths)):
        ref = _ref64(qkv[sl])
        err, e = _tile_err(got[sl], ref), _tile_err(_emulate(qkv[sl]), ref)
        worst = max(worst, float((err - (margin * e + FLOOR)).max()))
        need = max(need, float(((err - FLOOR).clamp(min=0) / e.clamp(min=1e-30)).max()))
        big = e >= FLOOR
        if bool(big.any()):
            plain = max(plain, float((err[big] / e[big]).max()))
    print(f"VARLEN_RATIO {tag} need={need:.3f} plain={plain:.3f} excess={worst:.3e}")
    return worst


# ---- CPU: packing ---------------------------------------------------------------------------------------------------
def test_packing_layout():
    lengths = [1, 17, 128, 130, 512]
    seqs = [list(range(7, 7 + L)) for L in lengths]
    tts = [[0] * (L // 2) + [1] * (L - L // 2) for L in lengths]
    assert M.capacity_bucket(sum(lengths), 4096) == 1024
    assert [M.capacity_bucket(t, 1024) for t in (1, 256, 257, 512, 513, 1024)] == [256, 256, 512, 512, 768, 1024]
    p = M.pack(seqs, tts, 1024, 8)
    assert (p.tokens, p.seqs, p.longest, p.capacity, p.blocks) == (788, 5, 512, 1024, 9)
    assert p.cu.tolist() == [0, 1, 18, 146, 276, 788, 788, 788, 788]
    assert p.first.tolist() == [0, 1, 18, 146, 276, 0, 0, 0]
    want_pos = np.concatenate([np.arange(L) for L in lengths])
    assert np.array_equal(p.pos[:788], want_pos) and not p.pos[788:].any()
    assert np.array_equal(p.ids[:788], np.concatenate(seqs)) and bool((p.ids[788:] == -1).all())
    assert np.array_equal(p.tts[:788], np.concatenate(tts)) and not p.tts[788:].any()
    table = [[0, 0], [1, 0], [2, 0], [3, 0], [3, 1], [4, 0], [4, 1], [4, 2], [4, 3]]
    assert p.table.shape == (1024 // 128 + 8, 2)
    assert p.table[:9].tolist() == table and bool((p.table[9:] == -1).all())
    assert p.buf.size == M.staging_size(1024, 8) == 3 * 1024 + 9 + 8 + 2 * 16
    # repacking a smaller request into the same buffer leaves nothing of the larger one behind
    q = M.pack([[5, 6, 7]], None, 1024, 8, out=p.buf)
    assert q.cu.tolist() == [0, 3] + [3] * 7 and bool((q.ids[3:] == -1).all()) and not q.tts.any()
    assert q.table[0].tolist() == [0, 0] and bool((q.table[1:] == -1).all()) and q.first.tolist() == [0] * 8
    assert M.length_class(1) == 64 and M.length_class(64) == 64 and M.length_class(65) == 128


def test_split_into_ordered_packs():
    assert M.plan_packs([300, 300, 300, 512, 10], 1024, 8) == [(0, 3), (3, 5)]
    assert M.plan_packs([512, 512, 1, 512], 1024, 8) == [(0, 2), (2, 4)]
    assert M.plan_packs([5] * 7, 1024, 3) == [(0, 3), (3, 6), (6, 7)]
    assert M.plan_packs([], 1024, 3) == []
    g = np.random.default_rng(1)
    seqs = [g.integers(0, 512, size=L).tolist() for L in (300, 40, 300, 7, 1, 512, 33)]
    whole = M.BertInference(_state(), _cfg(), "cpu", max_tokens=4096).logits(seqs)
    cut = M.BertInference(_state(), _cfg(), "cpu", max_tokens=512, max_seqs=2)
    assert len(M.plan_packs([len(s) for s in seqs], 512, 2)) == 5
    out = cut.logits(seqs)
    assert out.shape == (7, 2)
    torch.testing.assert_close(out, whole, rtol=0, atol=1e-5)


@pytest.mark.parametrize("bad,index,word", [
    ([[1, 2], [], [3]], 1, "empty"),
    ([[1], [2] * 513], 1, "length"),
    ([[1, 2], [3, 4], [5, 512]], 2, "vocabulary"),
    ([[1, -1]], 0, "vocabulary"),
])
def test_validation_errors(bad, index, word):
    inf = M.BertInference(_state(), _cfg(), "cpu")
    with pytest.raises(ValueError, match=rf"sequence {index}: .*{word}"):
        inf.logits(bad)


def test_validation_token_types_and_position_limit():
    inf = M.BertInference(_state(), _cfg(), "cpu")
    with pytest.raises(ValueError, match=r"sequence 1: token type outside"):
        inf.logits([[1, 2], [3, 4]], [[0, 1], [0, 2]])
    with pytest.raises(ValueError, match=r"sequence 0: 1 token types for 2 tokens"):
        inf.logits([[1, 2]], [[0]])
    short = BertConfig(vocab_size=512, hidden=128, heads=2, intermediate=256, layers=2, max_position=64)
    with pytest.raises(ValueError, match=r"sequence 0: length 65 above the maximum 64"):
        M.validate([np.arange(65)], None, short)


def test_cpu_forward_matches_unpadded_model():
    """Off the GPU: each sequence's logits equal that sequence run alone, unpadded (fp32 reassociation only)."""
    g = np.random.default_rng(2)
    lengths = [1, 17, 40, 128, 3]
    seqs = [g.integers(0, 512, size=L).tolist() for L in lengths]
    tts = [[0] * (L // 2) + [1] * (L - L // 2) for L in lengths]
    out = M.BertInference(_state(), _cfg(), "cpu").logits(seqs, tts)
    ref = _ref_logits(seqs, tts)
    torch.testing.assert_close(out, ref, rtol=0, atol=1e-5)


# ---- CPU: the bound is honest ---------------------------------------------------------------------------------------
HONEST = [17, 65, 130, 200]  # partial tiles and chunks; every one has padding keys in its last chunk


@pytest.mark.parametrize("family", ["diffuse", "peaky"])
def test_emulation_within_bound(family):
    qkv = _qkv(family, HONEST)
    got = torch.cat([_emulate_varlen(qkv[sl]) for sl in _seq_slices(HONEST)])
    assert _check_pack(f"emulation/{family}", got, qkv, HONEST) <= 0
    ref = bi.attn_varlen_reference(qkv.float(), bi.cu_seqlens(HONEST), SCALE)
    want = torch.cat([_ref64(qkv[sl]) for sl in _seq_slices(HONEST)])
    torch.testing.assert_close(ref.double(), want, rtol=1e-5, atol=1e-5)


def _mutant_excess(mutant, family, lengths):
    qkv = _qkv(family, lengths)
    return {L: _check_pack(f"{mutant}/{family}/L{L}", _emulate_varlen(qkv[sl], **{mutant: True}), qkv[sl], [L], margin=4)
            for L, sl in zip(lengths, _seq_slices(lengths))}


@pytest.mark.parametrize("family", ["diffuse", "peaky"])
def test_mutant_unmasked_padding_key(family):
    """a. key L (a zero staging row, score 0) left unmasked: it takes about 1 / (L + 1) of a diffuse row, so the short
    sequences of the GPU pack show it, at the ceiling margin 4. In the peaky family (scores of std 5) a score of 0
    lies far below most rows' maximum and the key gets next to no weight, as it should by the definition of
    softmax; the single-token sequence, whose only live score competes with it, shows it in either family."""
    ex = _mutant_excess("unmasked_pad_key", family, [1, 15, 17, 63, 65])
    if family == "diffuse":
        assert all(v > 0 for v in ex.values()), ex
    else:
        assert ex[1] > 0, ex


@pytest.mark.parametrize("family", ["diffuse", "peaky"])
def test_mutant_last_partial_tile_dropped(family):
    """b. the keys of the last, partial 16-key tile left out (1, 1, 2 and 8 keys of 17, 65, 130 and 200)."""
    ex = _mutant_excess("drop_last_tile", family, HONEST)
    assert all(v > 0 for v in ex.values()), ex


def _embed_case(lengths, restart=True):
    c = _cfg()
    g = torch.Generator().manual_seed(5)
    sd = _state()
    tabs = [sd[k].bfloat16() for k in ("word.weight", "pos.weight", "tok_type.weight")]
    gamma = (1 + 0.1 * torch.randn(c.hidden, generator=g)).bfloat16()
    beta = (0.1 * torch.randn(c.hidden, generator=g)).bfloat16()
    T = sum(lengths)
    ids = torch.randint(0, c.vocab_size, (T,), generator=g, dtype=torch.int32)
    tts = torch.randint(0, c.type_vocab, (T,), generator=g, dtype=torch.int32)
    pos = torch.cat([torch.arange(L, dtype=torch.int32) for L in lengths]) if restart \
        else (torch.arange(T, dtype=torch.int32) % c.max_position)
    return ids, tts, pos, tabs, gamma, beta


def _embed_ref64(ids, tts, pos, tabs, gamma, beta, eps):
    w, p, t = (x.double() for x in tabs)
    s = w[ids.long()] + p[pos.long()] + t[tts.long()]
    mu = s.mean(-1, keepdim=True)
    var = (s - mu).pow(2).mean(-1, keepdim=True)
    return (s - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def _embed_excess(got, ref, hidden):
    """One bf16 rounding of the output (relative 2^-8 per element) plus the fp32 LayerNorm's error: mean and variance
    are sums of `hidden` terms, each partial sum rounded to 2^-24, acting on an output of the tensor's scale."""
    tol = 2.0 ** -8 * ref.abs() + hidden * 2.0 ** -24 * ref.abs().max()
    return float(((got.double() - ref).abs() - tol).max())


def test_embedding_reference_and_position_mutant():
    lengths = [3, 130, 17, 64]
    c = _cfg()
    ids, tts, pos, tabs, gamma, beta = _embed_case(lengths)
    ref = _embed_ref64(ids, tts, pos, tabs, gamma, beta, c.ln_eps)
    got = bi.embed_ln_packed(ids, tts, pos, *tabs, gamma, beta, c.ln_eps)  # the CPU twin: fp32, one rounding
    assert got.dtype == torch.bfloat16 and _embed_excess(got.float(), ref, c.hidden) <= 0
    # positions running on over the sequence boundaries: only the first sequence still agrees
    bad = bi.embed_ln_packed(ids, tts, _embed_case(lengths, restart=False)[2], *tabs, gamma, beta, c.ln_eps)
    assert _embed_excess(bad.float()[:3], ref[:3], c.hidden) <= 0
    assert _embed_excess(bad.float(), ref, c.hidden) > 0
    # padding rows (id -1) are zero rows
    ids[5] = -1
    assert not bi.embed_ln_packed(ids, tts, pos, *tabs, gamma, beta, c.ln_eps)[5].any()


# ---- GPU: kernels ---------------------------------------------------------------------------------------------------
def _run_varlen_gpu(qkv, lengths, lmax=None):
    T = qkv.shape[0]
    assert T == sum(lengths)
    cu = torch.tensor(bi.cu_seqlens(lengths), dtype=torch.int32, device="cuda")
    table = torch.tensor(bi.block_table(lengths) + [(-1, -1)] * 3, dtype=torch.int32, device="cuda")
    out = torch.full((T, H, DH), float("nan"), dtype=torch.bfloat16, device="cuda")  # every live row is written
    bi.attn_fwd_varlen(qkv.cuda(), cu, table, len(lengths), lmax or max(lengths), SCALE, out=out)
    return out.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["diffuse", "peaky"])
@pytest.mark.parametrize("order", ["shuffled", "tail512_1"])
def test_attn_varlen_gpu(order, family):
    """Per (sequence, head, 16-token tile) against fp64; qkv holds exactly T rows, so in the second order the
    512-token and the 1-token sequences end at the end of the allocation. Measured need: 0.34 (see the file's docstring)."""
    lengths = _orders()[order]
    qkv = _qkv(family, lengths)
    got = _run_varlen_gpu(qkv, lengths).float()
    assert bool(torch.isfinite(got).all())
    assert _check_pack(f"kernel/{order}/{family}", got, qkv, lengths) <= 0


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [float("nan"), 1e30])
@pytest.mark.parametrize("L", [17, 130])
@pytest.mark.parametrize("where", ["start", "middle", "end"])
def test_attn_varlen_neighbours_inert_gpu(where, L, poison):
    """Every other sequence's Q, K and V overwritten with NaN / 1e30 in the same pack layout: the target's rows are
    bit-identical to the clean run (nothing is read across a sequence boundary, no garbage enters through P = 0)."""
    others = [64, 129, 1, 320]
    at = {"start": 0, "middle": 2, "end": 4}[where]
    lengths = others[:at] + [L] + others[at:]
    qkv = _qkv("diffuse", lengths, seed=L)
    sl = _seq_slices(lengths)[at]
    clean = _run_varlen_gpu(qkv, lengths)
    dirty = torch.full_like(qkv, poison)
    dirty[sl] = qkv[sl]
    got = _run_varlen_gpu(dirty, lengths)
    assert bool(torch.isfinite(clean[sl].float()).all())
    assert torch.equal(got[sl].view(torch.int16), clean[sl].view(torch.int16))


@pytest.mark.gpu
def test_attn_varlen_lds_class_and_padding_entries_gpu():
    """The same pack with the LDS sized for 512 instead of for its longest sequence gives the same bits, and a
    sequence longer than what the LDS was sized for is skipped (its rows keep what `out` held), never overrun."""
    lengths = [17, 100, 64]
    qkv = _qkv("diffuse", lengths)
    a = _run_varlen_gpu(qkv, lengths)
    b = _run_varlen_gpu(qkv, lengths, lmax=512)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    c = _run_varlen_gpu(qkv, lengths, lmax=64)
    s = _seq_slices(lengths)
    assert torch.equal(c[s[0]].view(torch.int16), a[s[0]].view(torch.int16))
    assert torch.equal(c[s[2]].view(torch.int16), a[s[2]].view(torch.int16))
    assert bool(torch.isnan(c[s[1]].float()).all())


@pytest.mark.gpu
def test_embed_ln_packed_gpu():
    """Against fp64 on the same pack: one bf16 rounding of the output plus the fp32 LayerNorm's error; capacity rows
    beyond T (id -1) come out as zeros."""
    lengths = _orders()["shuffled"]
    c = _cfg()
    ids, tts, pos, tabs, gamma, beta = _embed_case(lengths)
    ref = _embed_ref64(ids, tts, pos, tabs, gamma, beta, c.ln_eps)
    T, cap = sum(lengths), 2304
    pad = lambda t, v: torch.cat([t, torch.full((cap - T,), v, dtype=torch.int32)]).cuda()  # noqa: E731
    got = bi.embed_ln_packed(pad(ids, -1), pad(tts, 0), pad(pos, 0), *(t.cuda() for t in tabs), gamma.cuda(),
                             beta.cuda(), c.ln_eps).cpu().float()
    ex = _embed_excess(got[:T], ref, c.hidden)
    print(f"EMBED_EXCESS {ex:.3e}")
    assert ex <= 0
    assert not got[T:].any()


# ---- GPU: end to end ------------------------------------------------------------------------------------------------
def _ref_logits(seqs, tts=None):
    """The fp32 CPU model, per sequence, unpadded."""
    m = BertForSequenceClassification(_cfg(), None, seed=None)
    m.load_full(_state())
    m.eval()
    with torch.no_grad():
        return torch.cat([m(torch.tensor([s]), None if tts is None else torch.tensor([tts[i]]))
                          for i, s in enumerate(seqs)])


def _padded_bf16_logits(seqs, tts, S=128):
    """The existing padded bf16 eval forward on the GPU: fused kernels at S = 128, attention mask."""
    m = BertForSequenceClassification(_cfg(), None, seed=None)
    m.load_full(_state())
    m = m.cuda().bfloat16().eval()
    ids, tt, am = M._pad_arrays([np.asarray(s) for s in seqs], tts, S)
    with torch.no_grad():
        return m(*(torch.from_numpy(a).cuda() for a in (ids, tt, am))).float().cpu()


def _bf16_ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 7) if x > 0 else 0.0


E2E_LENGTHS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 100, 33, 2, 90, 48, 7, 120, 31, 77, 5, 111, 64, 19, 128, 50]


def _e2e_case():
    g = np.random.default_rng(3)
    seqs = [g.integers(0, 512, size=L).tolist() for L in E2E_LENGTHS]
    tts = [[0] * (L // 2) + [1] * (L - L // 2) for L in E2E_LENGTHS]
    return seqs, tts


@pytest.mark.gpu
def test_packed_logits_end_to_end_gpu():
    """Packed bf16 logits within 2 E_pad + one bf16 ulp of the largest |logit| of the fp32 reference, and the same
    class wherever the reference's top-two margin exceeds that bound. Measured: packed 5.2e-04, E_pad 5.9e-04."""
    seqs, tts = _e2e_case()
    ref = _ref_logits(seqs, tts)
    e_pad = float((_padded_bf16_logits(seqs, tts) - ref).abs().max())
    inf = M.BertInference(_state(), _cfg(), "cuda", max_tokens=2048, max_seqs=32)
    assert inf.packed
    got = inf.logits(seqs, tts).cpu()
    err = (got - ref).abs()
    bound = 2 * e_pad + _bf16_ulp(float(ref.abs().max()))
    print(f"E2E packed_err={float(err.max()):.3e} E_pad={e_pad:.3e} bound={bound:.3e}")
    assert got.shape == (len(seqs), 2) and float(err.max()) <= bound
    top = ref.sort(-1, descending=True).values
    sure = (top[:, 0] - top[:, 1]) > bound
    assert torch.equal(got.argmax(-1)[sure], ref.argmax(-1)[sure])
    # a request cut into several packs computes the same function (other positions in the pack: within the bound)
    cut = M.BertInference(_state(), _cfg(), "cuda", max_tokens=512, max_seqs=4).logits(seqs, tts).cpu()
    assert float((cut - ref).abs().max()) <= bound


@pytest.mark.gpu
def test_graph_replay_matches_eager_gpu():
    seqs, tts = _e2e_case()
    inf = M.BertInference(_state(), _cfg(), "cuda", max_tokens=2048, max_seqs=32)
    eager = inf.logits(seqs, tts)
    run = inf.graphed()
    first = run(seqs, tts)
    again = run(seqs, tts)
    assert torch.equal(first, eager) and torch.equal(again, eager)
    assert list(inf._graphs) == [(M.capacity_bucket(sum(E2E_LENGTHS), 2048), 128)] == [(1536, 128)]


@pytest.mark.gpu
def test_graph_replay_after_larger_batch_gpu():
    """2 short sequences replayed after 8 long ones through the same graph (capacity 256, length class 64): bit
    identical to a fresh instance that only ever saw the short batch -- no stale table, id or cu entries."""
    g = np.random.default_rng(4)
    long8 = [g.integers(0, 512, size=31).tolist() for _ in range(8)]
    short2 = [g.integers(0, 512, size=5).tolist() for _ in range(2)]
    inf = M.BertInference(_state(), _cfg(), "cuda", max_tokens=1024, max_seqs=16)
    run = inf.graphed()
    run(long8)
    got = run(short2)
    assert list(inf._graphs) == [(256, 64)]
    fresh = M.BertInference(_state(), _cfg(), "cuda", max_tokens=1024, max_seqs=16).graphed()(short2)
    assert torch.equal(got, fresh)
    assert torch.equal(got, M.BertInference(_state(), _cfg(), "cuda", max_tokens=1024, max_seqs=16).logits(short2))


@pytest.mark.gpu
def test_padded_ab_path_gpu(monkeypatch):
    """MIFX_BERT_INFER_PACKED=0 on the GPU: the training model's padded eval forward, eager and graphed, within the
    same end-to-end bound."""
    seqs, tts = _e2e_case()
    ref = _ref_logits(seqs, tts)
    bound = 2 * float((_padded_bf16_logits(seqs, tts) - ref).abs().max()) + _bf16_ulp(float(ref.abs().max()))
    monkeypatch.setenv("MIFX_BERT_INFER_PACKED", "0")
    inf = M.BertInference(_state(), _cfg(), "cuda", max_tokens=2048, max_seqs=32)
    assert not inf.packed
    eager = inf.logits(seqs, tts)
    assert float((eager.cpu() - ref).abs().max()) <= bound
    run = inf.graphed()
    assert torch.equal(run(seqs, tts), eager) and torch.equal(run(seqs, tts), eager)
