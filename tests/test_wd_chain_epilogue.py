"""The chained Wide&Deep kernel (csrc/wd_chain.hip) sums the loss and the dlogit over a wave with VALU lane swaps and
DPP adds instead of ds_bpermute; the training step of its one-iteration builds (T = 64, T = 256) reduces right behind
the loss phase, adds to the wide histogram in front of the forward barrier and runs its epilogue without a barrier.

CPU: the instruction sequence of wave_sum2, emulated lane by lane on a 64-lane float32 register file (the swap
emulations of tests/test_wd_chain_regmask.py), must give the bits of the xor butterfly 32 .. 1 in every lane.
(The loss-phase lane moves stay __shfl: their VALU form was measured slower and is not in the kernel, so there is
no sequence of theirs to emulate; profiles/wd_epilogue.md.)

GPU: the scalar part of the slab row (slab_loss per workgroup, the wide gradient with its bias column, the mean loss)
at every build's edge batches, on synthetic records, on records whose nine ids are the same in every example (the
most same-address LDS atomics) and on records with ids at or beyond the bucket count (clamped to 0), against the
fp64-accumulated emulation of the bf16 data path with the tolerances of tests/test_wd_chain_regmask.py; two runs
byte-equal."""
import functools

import numpy as np
import pytest
import torch

import test_wd_chain_live_tiles as tl
import test_wd_chain_regmask as rm
from mifx.models import wide_deep as wdm

gpu = pytest.mark.gpu
F = np.float32


# ------------------------------------------------------------------------------ CPU: the sequences, lane by lane
def _swap16(d, s):
    return tuple(np.array(x, dtype=F) for x in rm._permlane16_swap(list(d), list(s)))


def _swap32(d, s):
    return tuple(np.array(x, dtype=F) for x in rm._permlane32_swap(list(d), list(s)))


def _row_ror(v, n):
    """DPP row_ror:n -- inside every row of 16 lanes, lane i reads lane (i - n) mod 16"""
    return np.array([v[(l & ~15) + ((l & 15) - n) % 16] for l in range(64)], dtype=F)


def _quad_perm(v, perm):
    """DPP quad_perm:[p0,p1,p2,p3] -- lane 4 q + i reads lane 4 q + p_i"""
    return np.array([v[(l & ~3) + perm[l & 3]] for l in range(64)], dtype=F)


def _add_dpp(v, moved):  # v_add_f32_dpp: src0 is the DPP-selected lane's value, src1 the lane's own
    with np.errstate(all="ignore"):
        return (moved + v).astype(F)


def _wave_sum2(a, b):
    """csrc/wd_chain.hip wave_sum2: sum of a in lanes 0-31, of b in lanes 32-63"""
    with np.errstate(all="ignore"):
        p0, p1 = _swap32(a, b)
        c = (p0 + p1).astype(F)
        q0, q1 = _swap16(c, c)
        c = (q0 + q1).astype(F)
    c = _add_dpp(c, _row_ror(c, 8))
    c = _add_dpp(c, _row_ror(c, 4))
    c = _add_dpp(c, _quad_perm(c, (2, 3, 0, 1)))
    return _add_dpp(c, _quad_perm(c, (1, 0, 3, 2)))


def _butterfly(v):
    """for (o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o)"""
    v = np.array(v, dtype=F)
    idx = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[idx ^ o]).astype(F)
    return v


def _vectors():
    g = np.random.default_rng(1234)
    out = []
    for _ in range(8):
        out.append(g.standard_normal(64).astype(F))
        out.append((g.standard_normal(64) * 10.0 ** g.integers(-20, 20, 64)).astype(F))
    big = g.standard_normal(32).astype(F) * F(1e30)
    out.append(np.concatenate([big, -big])[g.permutation(64)] + g.standard_normal(64).astype(F))  # heavy cancellation
    out.append(np.concatenate([big, -big]) * F(1e-8) + F(1.0))
    tiny = np.frombuffer(g.integers(1, 1 << 23, 64, dtype=np.uint32).tobytes(), dtype=F).copy()  # denormals
    out.append(tiny)
    out.append(np.where(g.random(64) < 0.5, tiny, -tiny).astype(F))
    out.append(np.where(g.random(64) < 0.5, F(0.0), F(-0.0)).astype(F))
    out.append(np.full(64, F(-0.0)))
    inf = g.standard_normal(64).astype(F)
    inf[5] = np.inf
    out.append(inf.copy())
    inf[40] = -np.inf  # the sum is NaN in every lane
    out.append(inf.copy())
    one = np.zeros(64, dtype=F)
    one[37] = F(3.5)
    out.append(one)
    return out


def _same_bits(got, want):
    """bit-equal, a NaN matching any NaN (the kernel is built without NaN semantics; x + y and y + x may keep
    different payloads)"""
    got, want = np.asarray(got, dtype=F), np.asarray(want, dtype=F)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


def test_dpp_emulation_semantics():
    v = np.arange(64, dtype=F)
    assert _row_ror(v, 8)[:16].tolist() == [8, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6, 7]
    assert _row_ror(v, 4)[16:24].tolist() == [28, 29, 30, 31, 16, 17, 18, 19]
    assert _quad_perm(v, (2, 3, 0, 1))[:8].tolist() == [2, 3, 0, 1, 6, 7, 4, 5]
    assert _quad_perm(v, (1, 0, 3, 2))[60:].tolist() == [61, 60, 63, 62]


def test_wave_sum_equals_xor_butterfly():
    vs = _vectors()
    for i, a in enumerate(vs):
        for b in (vs[(i + 1) % len(vs)], vs[(i + 7) % len(vs)], a):
            got = _wave_sum2(a, b)
            assert _same_bits(got[:32], _butterfly(a)[:32]), i
            assert _same_bits(got[32:], _butterfly(b)[32:]), i
            # (what the kernel stores: lane 0's and lane 32's value; the butterfly leaves one value in all lanes
            # unless it is a NaN)
            assert _same_bits(got[:1], _butterfly(a)[:1]) and _same_bits(got[32:33], _butterfly(b)[:1])


# ---------------------------------------------------------------------------------------------- GPU
SHAPES = [(64, 1), (64, 17), (64, 40), (64, 64), (128, 129), (256, 1), (256, 255), (256, 256), (256, 257)]
KINDS = ["synthetic", "same_ids", "big_ids"]


@functools.lru_cache(maxsize=None)
def _records(kind):
    rec = tl._records()
    if kind == "synthetic":
        return rec
    dense, ids, label = wdm.records_to_tensors(rec)
    ids = ids.numpy().copy()
    nb = np.array([n for _, n in wdm.WideDeepConfig().wide])
    if kind == "same_ids":  # every example adds to the same nine histogram cells
        ids[:] = ids[0]
        assert (ids[0] < nb).all()
    else:  # ids at, just beyond and far beyond the bucket count, on every feature in turn: all clamp to id 0
        i = np.arange(len(ids))
        for f in range(9):
            ids[i % 9 == f, f] = nb[f] + np.array([0, 1, 65535 - nb[f]])[(i[i % 9 == f] // 9) % 3]
        assert (ids >= nb).any(1).all() and ids.max() == 65535
    out = wdm.tensors_to_records(dense.numpy(), ids, label.numpy())
    return torch.from_numpy(out.view(np.uint8).reshape(-1, 32).copy())


def _trainer(batch, tile):
    if tile == 256 and batch <= 128:
        # the trainer picks T = 256 only for batches that T = 128 cannot hold in one workgroup; the builds share the
        # weight image, the tile map and the slab, so the 8-wave one-workgroup trainer can launch the T = 256 library
        # (as tests/test_wd_chain_regmask.py does)
        from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

        tr = FusedWideDeepTrainer(tl._model(), batch=batch, device=torch.device("cuda"), large_tile=False,
                                  small_tile=False)
        assert (tr.tile, tr.waves, tr.grid) == (128, 8, 1)
        tr.tile = 256
        return tr
    return tl._trainer(batch, tile)


@functools.lru_cache(maxsize=None)
def _reference(kind, batch, tile):
    """(summed loss per workgroup, summed loss, canonical gradient by name)"""
    rec = _records(kind)
    m = tl._model()
    vec = wdm.pack_canonical(m)
    _, loss, canon = tl._emulate(vec, rec[:batch])
    per_wg = [tl._emulate(vec, rec[b * tile:min((b + 1) * tile, batch)])[1] for b in range((batch + tile - 1) // tile)]
    return per_wg, loss, tl._named(canon, m)


@gpu
@pytest.mark.parametrize("tile,batch", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_scalar_part_of_the_slab_row(kind, tile, batch):
    per_wg, loss_ref, ref = _reference(kind, batch, tile)
    runs = []
    for _ in range(2):
        tr = _trainer(batch, tile)
        assert (tr.tile, tr.grid) == (tile, (batch + tile - 1) // tile)
        tr.set_data(_records(kind).cuda())
        g = tr.gradients_once()
        torch.cuda.synchronize()
        runs.append((g.copy(), tr.slab_loss.cpu().numpy().copy(), tr.last_loss() / batch))
    g, slab_loss, mean_loss = runs[0]
    tag = f"{kind} T {tile} batch {batch}"
    assert slab_loss.shape == (len(per_wg),)
    for b, lb in enumerate(per_wg):  # workgroup b's own examples
        print(f"[epilogue] {tag} slab_loss[{b}] {slab_loss[b]:.6g} ref {lb:.6g}")
        assert abs(slab_loss[b] - lb) <= 1e-3 * abs(lb) + 1e-3
    assert abs(mean_loss - loss_ref / batch) <= 1e-3 * abs(loss_ref / batch) + 1e-3 / batch
    got = tl._named(g[tr.gidx_np].astype(np.float64), tr.model)
    for name in ("wide", "wide_bias"):
        err = np.abs(got[name] - ref[name]).max()
        tol = 2e-3 * np.abs(ref[name]).max() + 1e-5
        print(f"[epilogue] {tag} {name}: max err {err:.3g} tol {tol:.3g}")
        assert err <= tol
    if kind == "big_ids":  # the clamped ids all landed on id 0 of their feature: cells past a feature's buckets do
        # not exist, and nothing but the examples' cells and the bias is non-zero
        cfg = wdm.WideDeepConfig()
        _, ids, _ = wdm.records_to_tensors(_records(kind)[:batch])
        nbt = torch.tensor([n for _, n in cfg.wide])
        cells = (torch.where(ids < nbt, ids, torch.zeros_like(ids)) + torch.tensor(cfg.wide_offsets)).numpy()
        untouched = np.ones(got["wide"].size, dtype=bool)
        untouched[np.unique(cells)] = False
        assert (got["wide"].reshape(-1)[untouched] == 0).all()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]
