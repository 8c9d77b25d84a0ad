"""The T = 256 build of the chained Wide&Deep kernel (csrc/wd_chain256.hip) at its edges: every layer's dW operands
staged once, over the LDS of weight layers the backward has passed (rotated image placement). One workgroup partly and
exactly full (129, 256 examples), a second workgroup with 1 and 44 live rows (257, 300). References: an
fp64-accumulated emulation of the kernel's bf16 data path, fp32 autograd, and the T = 128 build."""
import functools

import numpy as np
import pytest
import torch

from mifx.data.synthetic import synthetic_records
from mifx.models import wide_deep as wdm

pytestmark = pytest.mark.gpu

NAMES = ["dnn.0.weight", "dnn.0.bias", "dnn.1.weight", "dnn.1.bias", "dnn.2.weight", "dnn.2.bias", "dnn.3.weight",
         "dnn.3.bias", "head.weight", "head.bias", "wide", "wide_bias"]


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


def _trainer(batch, large=True, **kw):
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    # T = 256 is chosen when ceil(batch / 128) > max_grid >= ceil(batch / 256)
    tr = FusedWideDeepTrainer(_model(), batch=batch, device=torch.device("cuda"), large_tile=large,
                              **({"max_grid": (batch + 255) // 256} if large else {}), **kw)
    assert (tr.tile, tr.grid) == ((256, (batch + 255) // 256) if large else (128, min((batch + 127) // 128, 256)))
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


@pytest.mark.parametrize("batch", [129, 256, 257, 300])
def test_gradient_matches_bf16_path_reference(batch):
    tr = _trainer(batch)
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
        print(f"[t256-onepass] batch {batch} {name}: max err {err:.3g} tol {tol:.3g}")
        assert err <= tol, f"{name}: max err {err:.3g} > {tol:.3g}"
    assert abs(tr.slab_loss.sum().item() - loss_ref) <= 1e-3 * abs(loss_ref) + 1e-3
    # 2) fp32 autograd: the bf16 data path's error at batches below 1000
    for name in NAMES:
        r = auto[name]
        rel = np.linalg.norm(got[name].reshape(r.shape) - r) / (np.linalg.norm(r) + 1e-8)
        print(f"[t256-onepass] batch {batch} {name}: rel Frobenius vs fp32 {rel:.4f}")
        assert rel < 0.125, f"{name}: relative Frobenius err {rel:.4f}"


def test_deterministic_and_image_consistent():
    """A stage that overwrites weights still being read, or a prologue that places W1 wrongly, shows as run-to-run
    differences or as a weight image that is not the image of the master weights."""
    out = []
    for _ in range(2):
        tr = _trainer(300)
        tr.set_data(_records().cuda())
        tr.capture(steps_per_graph=5)
        tr.run(10)
        torch.cuda.synchronize()
        assert torch.equal(tr.wt, tr._weight_image())
        assert torch.isfinite(tr.param).all()
        out.append((tr.param.clone(), tr.s0.clone(), tr.s1.clone(), tr.steps_done))
    assert out[0][3] == out[1][3] >= 10
    for a, b in zip(out[0][:3], out[1][:3]):
        assert torch.equal(a, b)


def test_forward_only_t256():
    """The eval instantiation (train = 0) of the T = 256 build reads the same rotated placement."""
    from mifx.ops import wd_chain as wdc

    batch = 300
    tr = _trainer(batch)
    rec = _records()[:batch].cuda().contiguous()
    out = torch.full((batch,), float("nan"), device="cuda")
    wdc.fused(rec, batch, batch, 0, None, tr.wt, tr.wide_weights, None, None, out, 1.0, 2, False, None, 8, None,
              tile=256)
    torch.cuda.synchronize()
    x_ref = _reference(batch)[0]
    err = np.abs(out.cpu().numpy() - x_ref).max()
    tol = 2e-3 * np.abs(x_ref).max() + 1e-5
    print(f"[t256-onepass] forward-only: max err {err:.3g} tol {tol:.3g}")
    assert err <= tol


def test_padding_rows_contribute_nothing():
    """Batch 257: the second workgroup has one live row and 255 clamped ones."""
    batch = 257
    recs = _records()
    tr = _trainer(batch)
    tr.set_data(recs.cuda())
    g256 = tr.gradients_once()
    loss256 = tr.slab_loss.sum().item()
    # the same 257 records followed by other records: the clamped rows never read past the batch
    other = torch.cat([recs[:batch], recs[2048:2048 + 512]]).cuda()
    tr.set_data(other)
    np.testing.assert_array_equal(tr.gradients_once(), g256)
    t128 = _trainer(batch, large=False)
    t128.set_data(recs.cuda())
    g128 = t128.gradients_once()
    loss128 = t128.slab_loss.sum().item()
    torch.cuda.synchronize()
    scale = np.abs(g128).max()
    np.testing.assert_allclose(g256, g128, rtol=0, atol=2e-5 * scale)
    assert abs(loss256 - loss128) <= 1e-3 * abs(loss128)
