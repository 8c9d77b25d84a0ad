"""The chained Wide&Deep kernel (csrc/wd_chain.hip) takes the ReLU masks of its backward from the activation fragments
the wave still holds in registers (two lane swaps per register pair) instead of reading them back from the staged
rows.

CPU: an index-level emulation of the two swaps on a 64-lane register file against the 8-byte read of the staged
activation row, the staged layout taken from stage()'s store expression. GPU: structured ReLU masks (dead / live units
at the word, lane-group and tile level, and per example) against the fp64-accumulated emulation of the bf16 data path
(helpers and margins of tests/test_wd_chain_live_tiles.py), with exact zeros where a unit is dead; and the scalar
part of the slab row that the kernel's epilogue writes (the loss, the wide block with its bias column)."""
import functools

import numpy as np
import pytest
import torch

import test_wd_chain_live_tiles as tl
from mifx.models import wide_deep as wdm

gpu = pytest.mark.gpu
NAMES = tl.NAMES
BIAS = 2.0  # |bias| of a switched unit
DEAD_MARGIN = 0.05  # a unit counts as dead where its largest pre-activation is below -DEAD_MARGIN
LIVE_K = {64: (3, 4), 96: (5,), 128: (7,)}  # K of the mask's layer -> live C-order k tiles (layers 5 and 4, 3, 2)


# ------------------------------------------------------------------------------------- CPU: the swaps, lane by lane
def _permlane16_swap(vdst, src):
    """v_permlane16_swap on 64-lane registers (lists): rows (16 lanes) 1 and 3 of vdst trade places with rows 0
    and 2 of src -> (new vdst, new src)"""
    d, s = list(vdst), list(src)
    for row in (1, 3):
        for i in range(16):
            d[16 * row + i], s[16 * (row - 1) + i] = src[16 * (row - 1) + i], vdst[16 * row + i]
    return d, s


def _permlane32_swap(vdst, src):
    """v_permlane32_swap: lanes 32-63 of vdst trade places with lanes 0-31 of src -> (new vdst, new src)"""
    return list(vdst[:32]) + list(src[:32]), list(vdst[32:]) + list(src[32:])


def test_swap_emulation_semantics():
    a, b = [("a", i) for i in range(64)], [("b", i) for i in range(64)]
    d, s = _permlane16_swap(a, b)
    assert d == a[:16] + b[:16] + a[32:48] + b[32:48] and s == a[16:32] + b[16:32] + a[48:] + b[48:]
    d, s = _permlane32_swap(a, b)
    assert d == a[:32] + b[:32] and s == a[32:] + b[32:]


@pytest.mark.parametrize("K", [64, 96, 128])
def test_register_mask_equals_staged_read(K):
    """Lane 16 h + r holds example r's activation fragment of k-step s as four 32-bit words: bf16 elements 2 i, 2 i + 1
    of the 16 bytes stage() stores at staged column 32 s + 8 h. The old mask read of lane (r, h) for gradient tile kt
    was the 8 bytes at staged columns 16 kt + 4 h .. + 3 of example r's row. An element is named (example, column)."""
    lanes = [(l & 15, l >> 4) for l in range(64)]  # lane -> (r, h)
    staged = {}  # (example, staged column) -> the (lane, k-step, element) that stage() stored there
    for lane, (r, h) in enumerate(lanes):
        for s in range(K // 32):
            for j in range(8):
                col = 32 * s + 8 * h + j  # stage(): *(v8bf*)(SA + row * (K + PAD) + 32 * s + 8 * h) = a[tb][s]
                assert (r, col) not in staged
                staged[(r, col)] = (lane, s, j)
    assert len(staged) == 16 * K
    # the register file: reg[s][i][lane] = word i of a[s], named by the staged elements it holds
    reg = [[[((r, 32 * s + 8 * h + 2 * i), (r, 32 * s + 8 * h + 2 * i + 1)) for (r, h) in lanes] for i in range(4)]
           for s in range(K // 32)]
    for ktl in LIVE_K[K]:
        seen = 0
        for s in range(K // 32):
            if 2 * s >= ktl:
                continue
            for j in range(2):  # mask word j: both swaps on words (j, j + 2) of the k-step's fragment
                p0, p1 = _permlane16_swap(reg[s][j], reg[s][j + 2])
                q = _permlane32_swap(p0, p1)
                for b in range(2):
                    kt = 2 * s + b
                    if kt >= ktl:
                        continue  # the odd tile of a half-live last k-step is not used
                    for lane, (r, h) in enumerate(lanes):
                        c0 = 16 * kt + 4 * h + 2 * j  # word j of the uint2 read at SA[row][16 kt + 4 h]
                        assert q[b][lane] == ((r, c0), (r, c0 + 1)), (K, ktl, kt, j, lane)
                        assert staged[(r, c0)][1] == s
                        seen += 1
        assert seen == 64 * 2 * ktl  # every live mask word of every lane


# ---------------------------------------------------------------------------------------------- GPU
def _model(kind):
    """tl._model() with the hidden units of layers 1-4 switched by their bias (weights and inputs are O(1), the biases
    +-BIAS) or, for "input", layer 1 switched per example by the sign of dense input 0."""
    m = tl._model()
    with torch.no_grad():
        if kind == "input":
            w = m.dnn[0].weight
            w.zero_()
            w[:, 0] = torch.where(torch.arange(w.shape[0]) % 2 == 0, 1.0, -1.0) * torch.linspace(0.5, 1.5, w.shape[0])
            m.dnn[0].bias.zero_()
            return m
        for lin in list(m.dnn)[:4]:
            f = torch.arange(lin.bias.shape[0])
            on = {"p2": f % 2 == 0, "p8": (f // 4) % 2 == 0, "p32": (f // 16) % 2 == 0,
                  "dead": torch.zeros_like(f, dtype=torch.bool), "alive": torch.ones_like(f, dtype=torch.bool)}[kind]
            # small weights, so that a layer's pre-activation is its bias up to a fraction of it
            lin.weight.mul_(0.25)
            lin.bias.copy_(torch.where(on, BIAS, -BIAS))
    return m


def _on_pattern(kind, n):
    f = np.arange(n)
    return {"p2": f % 2 == 0, "p8": (f // 4) % 2 == 0, "p32": (f // 16) % 2 == 0, "dead": f < 0, "alive": f >= 0}[kind]


def _trainer(kind, batch, tile):
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    if tile == 256 and batch > 128:
        kw = {"large_tile": True, "max_grid": (batch + 255) // 256}
    else:
        kw = {"large_tile": False, "small_tile": tile == 64}
    tr = FusedWideDeepTrainer(_model(kind), batch=batch, device=torch.device("cuda"), **kw)
    if tile == 256 and batch <= 128:
        # the trainer picks T = 256 only for batches that T = 128 cannot hold in one workgroup; the builds share the
        # weight image, the tile map and the slab, so the 8-wave one-workgroup trainer can launch the T = 256 library
        assert (tr.tile, tr.waves, tr.grid) == (128, 8, 1)
        tr.tile = 256
    assert (tr.tile, tr.grid) == (tile, (batch + tile - 1) // tile)
    tr.set_data(tl._records().cuda())
    return tr


@functools.lru_cache(maxsize=None)
def _reference(kind, batch):
    """(summed loss, canonical gradient by name, per layer 1-4: the units that fire on no example)"""
    rec = tl._records()[:batch]
    m = _model(kind)
    vec = wdm.pack_canonical(m)
    _, loss, canon = tl._emulate(vec, rec)
    dense, _, _ = wdm.records_to_tensors(rec)
    a = dense.double()
    dead = []
    for lin in list(m.dnn)[:4]:  # fp64 forward on the bf16 weights: which units never fire
        z = tl._bf(a) @ tl._bf(lin.weight.double()).T + tl._bf(lin.bias.double())
        a = torch.relu(z)
        # (by a margin far above the fp32 accumulation error: a unit that misses firing by less is not judged)
        dead.append((z.max(0).values < -DEAD_MARGIN).numpy())
    return loss, tl._named(canon, m), dead


def _run(kind, batch, tile):
    tr = _trainer(kind, batch, tile)
    g = tr.gradients_once()
    torch.cuda.synchronize()
    return tr, tl._named(g[tr.gidx_np].astype(np.float64), tr.model)


def _check_against_reference(got, ref, tag):
    for name in NAMES:
        err = np.abs(got[name] - ref[name]).max()
        tol = 2e-3 * np.abs(ref[name]).max() + 1e-5  # the margin of tests/test_wd_chain_live_tiles.py
        print(f"[regmask] {tag} {name}: max err {err:.3g} tol {tol:.3g} (max |ref| {np.abs(ref[name]).max():.3g})")
        assert err <= tol, f"{tag} {name}: max err {err:.3g} > {tol:.3g}"


def _check_dead_exact(got, dead, tag):
    """every incoming weight (and the bias) of a unit that fires on no example has an exactly zero gradient"""
    for li, d in enumerate(dead):
        gw = got[f"dnn.{li}.weight"].reshape(len(d), -1)
        gb = got[f"dnn.{li}.bias"].reshape(-1)
        print(f"[regmask] {tag} layer {li + 1}: {int(d.sum())} dead units of {len(d)}")
        assert (gw[d] == 0).all() and (gb[d] == 0).all(), f"{tag}: non-zero gradient into a dead unit of layer {li + 1}"


SHAPES = [(64, 17), (128, 33), (256, 33), (256, 257)]


@gpu
@pytest.mark.parametrize("tile,batch", SHAPES)
@pytest.mark.parametrize("kind", ["p2", "p8", "p32"])
def test_bias_switched_masks(kind, tile, batch):
    """Units dead / alive with period 2 (neighbouring bf16 halves of one mask word), 4 on / 4 off (neighbouring lane
    groups) and 16 on / 16 off (neighbouring tiles) over the feature index, on layers 1-4 at once."""
    loss_ref, ref, dead = _reference(kind, batch)
    for d in dead:  # the reference fires exactly the designed pattern
        assert np.array_equal(~d, _on_pattern(kind, len(d)))
    tr, got = _run(kind, batch, tile)
    tag = f"{kind} T {tile} batch {batch}"
    _check_dead_exact(got, dead, tag)
    _check_against_reference(got, ref, tag)
    assert abs(tr.slab_loss.sum().item() - loss_ref) <= 1e-3 * abs(loss_ref) + 1e-3


@gpu
@pytest.mark.parametrize("tile,batch", SHAPES)
def test_input_switched_masks(tile, batch):
    """Layer 1's even units fire where dense input 0 is positive, the odd ones where it is negative: the mask differs
    from example to example, and between the two 16-example column blocks of a wave."""
    loss_ref, ref, dead = _reference("input", batch)
    x0 = wdm.records_to_tensors(tl._records()[:batch])[0][:, 0].numpy()
    if batch > 16:
        assert (x0 > 0).any() and (x0 < 0).any() and not np.array_equal(x0[:16] > 0, x0[16:32] > 0)
    tr, got = _run("input", batch, tile)
    tag = f"input T {tile} batch {batch}"
    _check_dead_exact(got, dead, tag)
    _check_against_reference(got, ref, tag)
    assert abs(tr.slab_loss.sum().item() - loss_ref) <= 1e-3 * abs(loss_ref) + 1e-3


@gpu
def test_all_units_dead():
    loss_ref, ref, dead = _reference("dead", 256)
    assert all(d.all() for d in dead)
    tr, got = _run("dead", 256, 256)
    for name in ("dnn.0.weight", "dnn.1.weight", "dnn.2.weight", "dnn.3.weight", "head.weight", "dnn.0.bias",
                 "dnn.1.bias", "dnn.2.bias", "dnn.3.bias"):
        assert (got[name] == 0).all(), name
    _check_against_reference(got, ref, "dead T 256 batch 256")  # head.bias and the wide part still learn


@gpu
def test_all_units_alive():
    loss_ref, ref, dead = _reference("alive", 256)
    assert not any(d.any() for d in dead)
    tr, got = _run("alive", 256, 256)
    _check_against_reference(got, ref, "alive T 256 batch 256")
    assert abs(tr.slab_loss.sum().item() - loss_ref) <= 1e-3 * abs(loss_ref) + 1e-3


# ---------------------------------------------------------------------------------------------- GPU: the epilogue
@gpu
@pytest.mark.parametrize("tile,batch", [(64, 1), (64, 64), (256, 256), (256, 257)])
def test_scalar_part_of_the_slab_row(tile, batch):
    """slab_loss per workgroup, the wide gradient with its bias column (every workgroup's wave sums) and the mean loss
    against the emulation; a second run on the same input is byte-equal."""
    rec = tl._records()
    m = tl._model()
    vec = wdm.pack_canonical(m)
    _, loss_ref, canon = tl._emulate(vec, rec[:batch])
    ref = tl._named(canon, m)
    runs = []
    for _ in range(2):
        tr = tl._trainer(batch, tile)
        tr.set_data(rec.cuda())
        g = tr.gradients_once()
        torch.cuda.synchronize()
        runs.append((g.copy(), tr.slab_loss.cpu().numpy().copy(), tr.last_loss() / batch))
    g, slab_loss, mean_loss = runs[0]
    assert slab_loss.shape == ((batch + tile - 1) // tile,)
    for b in range(len(slab_loss)):  # workgroup b's own examples
        lb = tl._emulate(vec, rec[b * tile:min((b + 1) * tile, batch)])[1]
        print(f"[regmask] T {tile} batch {batch} slab_loss[{b}] {slab_loss[b]:.6g} ref {lb:.6g}")
        assert abs(slab_loss[b] - lb) <= 1e-3 * abs(lb) + 1e-3
    assert abs(mean_loss - loss_ref / batch) <= 1e-3 * abs(loss_ref / batch) + 1e-3 / batch
    got = tl._named(g[tr.gidx_np].astype(np.float64), tr.model)
    for name in ("wide", "wide_bias"):
        err = np.abs(got[name] - ref[name]).max()
        tol = 2e-3 * np.abs(ref[name]).max() + 1e-5
        print(f"[regmask] T {tile} batch {batch} {name}: max err {err:.3g} tol {tol:.3g}")
        assert err <= tol
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]
