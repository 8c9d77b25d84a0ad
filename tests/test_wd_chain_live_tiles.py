"""The chained Wide&Deep kernel (csrc/wd_chain.hip, T = 64 / 128 / 256 builds) computes only its live 16x16 tiles: the
dW row axis is staged in natural tiles, so padding fills whole trailing tiles, which the forward, the activation
gradient, the mask reads, the dW phases and the gradient slab all skip at compile time.

CPU: the host maps (chain_dw_rows, chain_maps, chain_live_tiles) against an index-level emulation of the kernel's
stage() store. GPU: every build against the fp64-accumulated emulation of the bf16 data path and fp32 autograd
(helpers and bounds of tests/test_wd_chain256_onepass.py), with non-zero biases so that the constant-1 rows matter --
layer 3's sits alone in forward n tile 3, which holds no trainable row."""
import functools

import numpy as np
import pytest
import torch

from mifx.data.synthetic import synthetic_records
from mifx.models import wide_deep as wdm

NAMES = ["dnn.0.weight", "dnn.0.bias", "dnn.1.weight", "dnn.1.bias", "dnn.2.weight", "dnn.2.bias", "dnn.3.weight",
         "dnn.3.bias", "head.weight", "head.bias", "wide", "wide_bias"]
LIVE_DW = [(7, 1), (5, 7), (3, 5), (3, 4), (1, 3)]  # natural n tiles x C-order k tiles per layer


# ---------------------------------------------------------------------------------------------- CPU: the host maps
def test_chain_maps_live_tiles_and_stride():
    tmap, stride, gidx, mask, wmap = wdm.chain_maps()
    assert int((tmap >= 0).sum()) == 72
    assert stride == 72 * 256 + wdm.WIDE_PAD == 20608
    assert sorted(tmap[tmap >= 0]) == list(range(72))  # the live tiles fill the slab without holes
    for li, ((K, N), (dn, kt)) in enumerate(zip(wdm.LAYER_KN, LIVE_DW)):
        live = tmap[wdm.TILE_BASE[li]:wdm.TILE_BASE[li] + (N // 16) * (K // 16)].reshape(N // 16, K // 16) >= 0
        want = (np.arange(N // 16)[:, None] < dn) & (np.arange(K // 16)[None, :] < kt)
        assert np.array_equal(live, want), f"layer {li + 1}"
    assert [(dn, kt) for _, dn, kt in wdm.chain_live_tiles()] == LIVE_DW
    assert [fn for fn, _, _ in wdm.chain_live_tiles()] == [7, 5, 4, 3, 1]  # rows incl. the constant-1 row


def test_gidx_injective_on_trainable_entries():
    tmap, stride, gidx, mask, wmap = wdm.chain_maps()
    live = np.nonzero(mask)[0]
    assert len(live) == 3 * 100 + 100 + 100 * 70 + 70 + 70 * 48 + 48 + 48 * 34 + 34 + 34 + 1 + wdm.NWIDE
    slots = gidx[live]
    assert len(np.unique(slots)) == len(live)
    assert slots.min() >= 0 and slots.max() < stride
    dnn = slots[live < wdm.WTOT]
    assert dnn.max() < stride - wdm.WIDE_PAD  # DNN entries in the tile block, the wide ones behind it


@pytest.mark.parametrize("li", [0, 1, 2, 3])
def test_dw_row_map_equals_kernel_store(li):
    """stage(): lane group h holds, for dZ tile kt (a C-order tile of the layer above's k axis), the four C positions
    16 kt + 4 h + e, and stores the pair of tiles (2m, 2m+1) as one 16-byte fragment at staged column
    32 m + 8 (2 (h & 1) + (h >> 1)): element e of tile kt lands 4 (kt & 1) + e elements into it."""
    N = wdm.LAYER_KN[li][1]
    feat_at_c = wdm.chain_perm(N)  # C position -> natural feature
    staged = np.full(N, -1)
    for kt in range(N // 16):
        for h in range(4):
            for e in range(4):
                col = 32 * (kt >> 1) + 8 * (2 * (h & 1) + (h >> 1)) + 4 * (kt & 1) + e
                assert staged[col] == -1
                staged[col] = feat_at_c[16 * kt + 4 * h + e]
    assert np.array_equal(staged, wdm.chain_dw_rows(li))
    # natural tiles: staged 16-column tile j holds exactly the features 16 j .. 16 j + 15, inner order 0-3 8-11 4-7 12-15
    assert np.array_equal(staged.reshape(-1, 16) % 16, np.tile([0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15],
                                                               (N // 16, 1)))
    assert np.array_equal(staged.reshape(-1, 16) // 16, np.arange(N // 16)[:, None].repeat(16, 1))


def test_layer5_rows_natural():
    assert np.array_equal(wdm.chain_dw_rows(4), np.arange(16))


# ---------------------------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


def _model():
    m = wdm.WideDeepModel(seed=1)
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        m.wide.copy_(torch.randn(m.wide.shape, generator=g) * 0.3)
        m.wide_bias.fill_(-0.2)
        for lin in m.dnn:
            lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    return m


def _bf(x):
    """fp64 -> nearest bf16 value, kept as fp64"""
    return x.float().to(torch.bfloat16).double()


def _emulate(vec, rec):
    """The kernel's data path with fp64 accumulation: bf16 weights, activations and activation gradients, the
    bf16-rounded dlogit in the dense backward, the unrounded one in the wide part. -> (logits, summed loss,
    canonical gradient), fp64."""
    vec = torch.as_tensor(np.asarray(vec), dtype=torch.float64)
    dense, ids, label = wdm.records_to_tensors(rec.cpu())
    label = label.double()
    B = len(label)
    a = torch.zeros(B, wdm.LAYER_KN[0][0], dtype=torch.float64)
    a[:, :3] = dense.double()
    a[:, 3] = 1.0
    acts, wts = [_bf(a)], []
    for li, (K, N) in enumerate(wdm.LAYER_KN):
        wt = _bf(vec[wdm.LAYER_OFF[li]:wdm.LAYER_OFF[li] + K * N].reshape(N, K))
        wts.append(wt)
        z = acts[-1][:, :K] @ wt.T
        if li < 4:
            acts.append(_bf(torch.relu(z)))
        else:
            deep = z[:, 0]
    cfg = wdm.WideDeepConfig()
    nb = torch.tensor([n for _, n in cfg.wide])
    idc = torch.where(ids < nb, ids, torch.zeros_like(ids)) + torch.tensor(cfg.wide_offsets)
    wvec = vec[wdm.WTOT:]
    x = deep + wvec[idc].sum(1) + wvec[cfg.wide_rows]
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, label, reduction="sum")
    dl = torch.sigmoid(x) - label
    dz = torch.zeros(B, 16, dtype=torch.float64)
    dz[:, 0] = _bf(dl)
    grads = {}
    for li in range(4, -1, -1):
        grads[li] = dz.T @ acts[li]  # dW^T [N][K]
        if li > 0:
            dz = _bf((dz @ wts[li]) * (acts[li] > 0).double())
    gw = torch.zeros(wdm.NWIDE, dtype=torch.float64)
    gw.index_add_(0, idc.reshape(-1), dl[:, None].expand(-1, 9).reshape(-1))
    gw[cfg.wide_rows] = dl.sum()
    canon = torch.cat([grads[li].reshape(-1) for li in range(5)] + [gw])
    return x.numpy(), float(loss), canon.numpy()


def _named(canon, model):
    """canonical-order vector -> torch-shaped tensors by parameter name"""
    return wdm.canonical_grad_to_torch(canon, model, np.arange(len(canon)))


def _trainer(batch, tile, **kw):
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    if tile == 256:  # T = 256 is chosen when ceil(batch / 128) > max_grid >= ceil(batch / 256)
        kw = {"large_tile": True, "max_grid": (batch + 255) // 256, **kw}
    else:
        kw = {"large_tile": False, "small_tile": tile == 64, **kw}
    tr = FusedWideDeepTrainer(_model(), batch=batch, device=torch.device("cuda"), **kw)
    assert (tr.tile, tr.grid) == (tile, (batch + tile - 1) // tile)
    return tr


@functools.lru_cache(maxsize=None)
def _records(n=4096):
    return synthetic_records(n, seed=7)


@functools.lru_cache(maxsize=None)
def _reference(batch):
    """(emulated logits, loss, canonical gradient; fp32 autograd gradients by name) on the first `batch` records"""
    rec = _records()[:batch]
    m = _model()
    vec = wdm.pack_canonical(m)
    x, loss, canon = _emulate(vec, rec)
    dense, ids, label = wdm.records_to_tensors(rec)
    m.zero_grad()
    m.loss(dense, ids, label, reduction="sum").backward()
    auto = {n: p.grad.detach().numpy().copy() for n, p in m.named_parameters()}
    return x, loss, canon, auto


@gpu
@pytest.mark.parametrize("tile,batch", [(64, 40), (64, 64), (128, 129), (256, 256), (256, 257)])
def test_gradient_matches_bf16_path_reference(tile, batch):
    """Every build, one workgroup partly and exactly full, and a second workgroup with one live row. A forward that
    skipped layer 3's constant-1 tile would lose dnn.3's bias from the logits and dnn.3.bias / the layers below from
    the gradient."""
    tr = _trainer(batch, tile)
    tr.set_data(_records().cuda())
    g = tr.gradients_once()
    torch.cuda.synchronize()
    _, loss_ref, canon_ref, auto = _reference(batch)
    assert np.array_equal(tr.param.cpu().numpy(), wdm.pack_canonical(_model()))
    got = _named(g[tr.gidx_np].astype(np.float64), tr.model)
    ref = _named(canon_ref, tr.model)
    assert sorted(got) == sorted(NAMES) == sorted(auto)
    # 1) the data path: only the accumulation order differs from the emulation
    for name in NAMES:  # per tensor: head.* is layer 5, dnn.0.* layer 1, wide / wide_bias the LDS histogram
        err = np.abs(got[name] - ref[name]).max()
        tol = 2e-3 * np.abs(ref[name]).max() + 1e-5
        print(f"[live-tiles] T {tile} batch {batch} {name}: max err {err:.3g} tol {tol:.3g}")
        assert err <= tol, f"{name}: max err {err:.3g} > {tol:.3g}"
    assert abs(tr.slab_loss.sum().item() - loss_ref) <= 1e-3 * abs(loss_ref) + 1e-3
    # 2) fp32 autograd: the bf16 data path's error at batches below 1000
    for name in NAMES:
        r = auto[name]
        rel = np.linalg.norm(got[name].reshape(r.shape) - r) / (np.linalg.norm(r) + 1e-8)
        print(f"[live-tiles] T {tile} batch {batch} {name}: rel Frobenius vs fp32 {rel:.4f}")
        assert rel < 0.125, f"{name}: relative Frobenius err {rel:.4f}"


@gpu
@pytest.mark.parametrize("tile", [64, 128, 256])
def test_forward_only_logits(tile):
    """The eval instantiation (train = 0) of each build skips the same forward tiles."""
    from mifx.ops import wd_chain as wdc

    batch = 300
    tr = _trainer(256 if tile == 256 else 40 if tile == 64 else 129, tile)
    rec = _records()[:batch].cuda().contiguous()
    out = torch.full((batch,), float("nan"), device="cuda")
    wdc.fused(rec, batch, batch, 0, None, tr.wt, tr.wide_weights, None, None, out, 1.0, (batch + tile - 1) // tile,
              False, None, 4 if tile == 64 else 8, None, tile=tile)
    torch.cuda.synchronize()
    x_ref = _reference(batch)[0]
    err = np.abs(out.cpu().numpy() - x_ref).max()
    tol = 2e-3 * np.abs(x_ref).max() + 1e-5
    print(f"[live-tiles] T {tile} forward-only: max err {err:.3g} tol {tol:.3g}")
    assert err <= tol


@gpu
@pytest.mark.parametrize("tile,batch", [(64, 40), (128, 129), (256, 257)])
def test_dead_slots_stay_dead(tile, batch):
    """The slab has no room for a dead tile (72 live tiles x 256 columns + the wide block, test above), so a dead tile
    is NEVER WRITTEN: every tile column of every slab row belongs to a live tile and is written by the one wave that
    owns it -- checked by poisoning the slab with NaN first. Inside the live tiles, the columns that hold no trainable
    entry (the trainer's inv == -1) are of two kinds: padding rows / padding k columns, whose gradient is EXACTLY ZERO
    in every slab row and in the reduced gradient, and the constant-1 rows of layers 1, 2 and 4 (layer 3's lies in a
    dead tile), which carry the gradient of a weight nobody trains: finite, equal to the emulation's value, and never
    read by the optimizer (wsc == -1)."""
    tr = _trainer(batch, tile)
    tr.set_data(_records().cuda())
    tr.slab.fill_(float("nan"))
    g = tr.gradients_once()
    torch.cuda.synchronize()
    ntile_cols = tr.stride - wdm.WIDE_PAD
    slab = tr.slab.cpu().numpy()
    assert np.isfinite(slab).all() and np.isfinite(g).all()  # every column of every row was written
    inv = tr.inv.cpu().numpy()
    assert (tr.wsc.cpu().numpy()[inv < 0] == -1).all()
    # canonical entries of the constant-1 rows (row R_l of layers 1-4, columns 0..K-1) that have a slab slot
    tmap, _, gidx, mask, _ = wdm.chain_maps()
    const_slots = []
    for li, ((K, N), (_, nr)) in enumerate(zip(wdm.LAYER_KN[:4], wdm._real_dims(tr.model.cfg)[:4])):
        ktile = np.argsort(wdm.chain_perm(K)) // 16  # natural column -> C-order k tile
        live = tmap[wdm.TILE_BASE[li] + (nr // 16) * (K // 16) + ktile] >= 0  # (gidx is 0 where the tile is dead)
        can = wdm.LAYER_OFF[li] + nr * K + np.arange(K)[live]
        if live.any():  # the row's n tile is live
            const_slots.append((can, gidx[can]))
        else:
            assert li == 2  # layer 3: row 48 is alone in n tile 3
    can = np.concatenate([c for c, _ in const_slots])
    cs = np.concatenate([s for _, s in const_slots])
    assert (inv[cs] < 0).all() and len(np.unique(cs)) == len(cs)
    dead = np.nonzero(inv[:ntile_cols] < 0)[0]
    pad = np.setdiff1d(dead, cs)
    assert len(pad) > 0 and (slab[:, pad] == 0).all() and (g[pad] == 0).all()
    ref = _reference(batch)[2][can]
    err = np.abs(g[cs] - ref).max()
    tol = 2e-3 * np.abs(ref).max() + 1e-5
    print(f"[live-tiles] T {tile} constant-row slots: max err {err:.3g} tol {tol:.3g}")
    assert err <= tol
    # the wide block's padding columns are zero too
    wpad = np.nonzero(inv[ntile_cols:] < 0)[0] + ntile_cols
    assert (g[wpad] == 0).all()


@gpu
def test_deterministic_at_257():
    out = []
    for _ in range(2):
        tr = _trainer(257, 256)
        tr.set_data(_records().cuda())
        out.append((tr.gradients_once().copy(), tr.slab_loss.cpu().numpy().copy()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])


@gpu
def test_builds_agree_at_256():
    """T = 128 (two workgroups, the 8-wave ownership at TBN = 1) against T = 256 (one workgroup), the bound of
    tests/test_wd_chain256_onepass.py for this comparison."""
    recs = _records().cuda()
    res = {}
    for tile in (128, 256):
        tr = _trainer(256, tile)
        tr.set_data(recs)
        res[tile] = (tr.gradients_once().copy(), tr.slab_loss.sum().item())
    torch.cuda.synchronize()
    (g128, loss128), (g256, loss256) = res[128], res[256]
    scale = np.abs(g128).max()
    np.testing.assert_allclose(g256, g128, rtol=0, atol=2e-5 * scale)
    assert abs(loss256 - loss128) <= 1e-3 * abs(loss128)


@gpu
def test_trainer_steps_and_checkpoint_round_trip():
    """Three optimizer steps (Adagrad on the DNN, FTRL on the wide part: the defaults) at batch 300 on the T = 256
    build against the T = 128 build, then state_dict() -> fresh trainer -> load_state_dict() continues bit-identically:
    the slab-column-order master weights and optimizer state survive the new slab layout."""
    recs = _records().cuda()
    trs = {}
    for tile in (128, 256):
        tr = _trainer(300, tile)
        assert (tr.dnn_opt.kind, tr.wide_opt.kind) == ("adagrad", "ftrl")
        tr.set_data(recs)
        for _ in range(3):
            tr.step()
        trs[tile] = tr
    torch.cuda.synchronize()
    assert trs[128].steps_done == trs[256].steps_done == 3
    for name in ("param", "s0", "s1"):
        a, b = getattr(trs[256], name).cpu().numpy(), getattr(trs[128], name).cpu().numpy()
        scale = np.abs(b).max()
        print(f"[live-tiles] 3 steps {name}: max diff {np.abs(a - b).max():.3g} bound {2e-5 * scale:.3g}")
        np.testing.assert_allclose(a, b, rtol=0, atol=2e-5 * scale)
    assert torch.equal(trs[256].wt, trs[256]._weight_image())
    sd = trs[256].state_dict()
    fresh = _trainer(300, 256)
    fresh.load_state_dict(sd)
    fresh.set_data(recs)
    assert fresh.steps_done == 3
    for tr in (trs[256], fresh):
        for _ in range(2):
            tr.step()
    torch.cuda.synchronize()
    assert fresh.steps_done == trs[256].steps_done == 5
    for name in ("param", "s0", "s1"):
        assert torch.equal(getattr(fresh, name), getattr(trs[256], name)), name
    assert torch.equal(fresh.wt, trs[256].wt)
