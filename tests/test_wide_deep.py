"""Wide&Deep: canonical-layout packing (CPU) and fused gfx950 kernel vs fp32 PyTorch (GPU)."""
import numpy as np
import pytest
import torch

from mifx.data.synthetic import synthetic_records
from mifx.models import wide_deep as wdm
from mifx.trainer.fused_wide_deep import OptSpec
from mifx.trainer.torch_wide_deep import TorchWideDeepTrainer

# the "*_reg" cases of the variant tests: FTRL's L1 shrinkage, its 2 * l2 term and its general lr_power (powf) branch
_REG_OPTS = {"dnn_opt": OptSpec("adagrad", lr=0.05),
             "wide_opt": OptSpec("ftrl", lr=0.2, l1=0.5, l2=0.1, lr_power=-0.75)}


def _canonical_forward(vec, dense, ids):
    """numpy emulation of the kernel's padded forward (fp32), biases via constant-1 column."""
    a = np.zeros((len(dense), wdm.LAYER_KN[0][0]), np.float32)
    a[:, :3] = dense
    a[:, 3] = 1.0
    for li, (K, N) in enumerate(wdm.LAYER_KN):
        wt = vec[wdm.LAYER_OFF[li]:wdm.LAYER_OFF[li] + K * N].reshape(N, K)
        z = a[:, :K] @ wt.T
        if li < len(wdm.LAYER_KN) - 1:
            a = np.maximum(z, 0)
        else:
            deep = z[:, 0]
    cfg = wdm.WideDeepConfig()
    nb = np.array([n for _, n in cfg.wide])
    off = np.array(cfg.wide_offsets)
    idc = np.where(ids < nb, ids, 0) + off
    wide = vec[wdm.WTOT:][idc].sum(1) + vec[wdm.WTOT + cfg.wide_rows]
    return deep + wide


def test_hidden_units_match_reference():
    assert wdm.dnn_hidden_units() == [100, 70, 48, 34]
    assert wdm.WideDeepConfig().wide_rows == 2127


def test_pack_roundtrip_and_forward():
    m = wdm.WideDeepModel(seed=3)
    with torch.no_grad():
        m.wide.normal_()
        m.wide_bias.fill_(0.3)
        for lin in m.dnn:
            lin.bias.normal_()
    vec = wdm.pack_canonical(m)
    rec = synthetic_records(300, seed=5)
    dense, ids, _ = wdm.records_to_tensors(rec)
    ref = m(dense, ids).detach().numpy()
    got = _canonical_forward(vec, dense.numpy(), ids.numpy())
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4)
    m2 = wdm.unpack_canonical(vec, wdm.WideDeepModel(seed=9))
    np.testing.assert_allclose(m2(dense, ids).detach().numpy(), ref, rtol=1e-5, atol=1e-5)


def test_index_maps_are_bijective_on_slab():
    gidx, mask = wdm.canonical_index_maps()
    tmap, stride = wdm.compact_tile_map()
    live = gidx[mask.astype(bool)]
    assert len(np.unique(live)) == len(live)  # every trainable entry has its own compact slot
    assert live.max() < stride <= wdm.STRIDE and stride % 4 == 0
    assert (tmap >= 0).sum() == 72 and sorted(tmap[tmap >= 0]) == list(range(72))
    # every trainable entry's tile is live; dead tiles hold padding only
    for li, ((K, N), m) in enumerate(zip(wdm.LAYER_KN, wdm._trainable_masks(wdm.WideDeepConfig()))):
        for nt in range(N // 16):
            for kt in range(K // 16):
                t = wdm.TILE_BASE[li] + nt * (K // 16) + kt
                assert (tmap[t] >= 0) == bool(m[16 * nt:16 * nt + 16, 16 * kt:16 * kt + 16].any())
    # trainable = real weights + biases: 3*100+100 + 100*70+70 + 70*48+48 + 48*34+34 + 34+1 + 2128
    assert mask.sum() == 400 + 7070 + 3408 + 1666 + 35 + 2128


def test_records_roundtrip():
    rec = synthetic_records(100, seed=1)
    d, i, l = wdm.records_to_tensors(rec)
    back = wdm.tensors_to_records(d.numpy(), i.numpy(), l.numpy())
    assert back.tobytes() == rec.numpy().tobytes()
    assert set(np.unique(l.numpy())) <= {0.0, 1.0}


def test_torch_trainer_learns():
    torch.manual_seed(0)
    tr = TorchWideDeepTrainer(wdm.WideDeepModel(seed=0), batch=256)
    tr.set_data(synthetic_records(8192, seed=2))
    losses = []
    for _ in range(60):
        tr.step()
        losses.append(tr.last_loss() / 256)
    assert np.mean(losses[-10:]) < np.mean(losses[:10]) - 0.02


# ------------------------------------------------------------------------------------ GPU
def _torch_grads(model, rec, reduction="sum"):
    dense, ids, label = wdm.records_to_tensors(rec.cpu())
    model.zero_grad()
    loss = model.loss(dense, ids, label, reduction=reduction)
    loss.backward()
    g = {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()}
    return float(loss.detach()), g


def _bf(x):
    return x.to(torch.bfloat16).float()


def _emulated_grads(vec, rec):
    """fp32 emulation of the kernel's bf16 data path on the canonical padded layout
    (bf16 weights/activations/activation-grads, fp32 accumulation)."""
    vec = torch.as_tensor(vec, dtype=torch.float32)
    dense, ids, label = wdm.records_to_tensors(rec.cpu())
    B = len(label)
    a = torch.zeros(B, wdm.LAYER_KN[0][0])
    a[:, :3] = dense
    a[:, 3] = 1.0
    acts = [_bf(a)]
    wts = []
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
    dz = torch.zeros(B, 16)
    dz[:, 0] = dl
    dz = _bf(dz)
    grads = {}
    for li in range(4, -1, -1):
        grads[li] = dz.T @ acts[li]          # dWt [N][K]
        if li > 0:
            da = dz @ wts[li]                # [B][K]
            dz = _bf(da * (acts[li] > 0).float())
    gw = torch.zeros(wdm.NWIDE)
    gw.index_add_(0, idc.reshape(-1), dl[:, None].expand(-1, 9).reshape(-1))
    gw[cfg.wide_rows] = dl.sum()
    canon = torch.cat([grads[li].reshape(-1) for li in range(5)] + [gw])
    return float(loss), canon.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["chain", "chain4", "chain128", "tile"])
@pytest.mark.parametrize("batch", [40, 64, 1000, 8192])
def test_fused_gradients_match_torch(batch, kernel):
    torch.manual_seed(batch)
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    m = wdm.WideDeepModel(seed=1)
    with torch.no_grad():
        m.wide.normal_(0, 0.3)
        m.wide_bias.fill_(-0.2)
        for lin in m.dnn:
            lin.bias.normal_(0, 0.1)
    rec = synthetic_records(batch, seed=7)
    kw = {"kernel": "chain", "waves": 4} if kernel == "chain4" else {"kernel": kernel}
    if kernel == "chain128":  # small batches on the T = 128 build (the default trains them on T = 64)
        if batch > 64:
            pytest.skip("same launch as 'chain' above 64 examples")
        kw = {"kernel": "chain", "small_tile": False}
    tr = FusedWideDeepTrainer(m, batch=batch, device=dev, **kw)
    if kernel == "chain" and batch <= 64:
        assert tr.tile == 64 and tr.waves == 4
    if kernel == "chain128":
        assert tr.tile == 128
    tr.set_data(rec.to(dev))
    g_tn = tr.gradients_once()
    torch.cuda.synchronize()
    _, mask = wdm.canonical_index_maps()
    gidx = tr.gidx_np
    got = g_tn[gidx]
    loss_em, em = _emulated_grads(tr.param.cpu(), rec)
    # 1) exact data-path check against the bf16 emulation (only accumulation order differs)
    msk = mask.astype(bool)
    err = np.abs(got - em)[msk]
    tol = 2e-3 * np.abs(em[msk]).max() + 1e-5
    bad = np.argsort(-err)[:5]
    assert err.max() <= tol, f"max err {err.max():.3g} > {tol:.3g}; worst canon idx {np.flatnonzero(msk)[bad]}"
    assert abs(tr.slab_loss.sum().item() - loss_em) <= 1e-3 * abs(loss_em) + 1e-3
    # 2) against the fp32 PyTorch model: relative Frobenius error per tensor. The bf16 data path
    #    (inputs, activations, activation-grads rounded to 8 mantissa bits) costs a few % on the
    #    first layer at tiny batches (cancellation over 40 examples), <3 % at >= 1000.
    named = wdm.canonical_grad_to_torch(g_tn, m, gidx)
    mref = wdm.unpack_canonical(tr.param.cpu(), wdm.WideDeepModel(seed=1))
    _, ref = _torch_grads(mref, rec)
    #    Bounds from the measured errors (round 5, every kernel: B 40 <= 0.103, 64 <= 0.096, 1000 <= 0.050,
    #    8192 <= 0.0057) with ~20 % margin; and, since a Frobenius bound alone would pass a systematic scaling of the
    #    gradient of that size, the projection <g, r> / <r, r> of each gradient on the reference must be 1 to within
    #    a few noise standard deviations (rounding noise is unbiased; a 10 % bias gives 0.9).
    lim = 0.125 if batch < 1000 else (0.06 if batch < 8192 else 0.008)
    plim = 0.05 if batch < 1000 else 0.02
    rels, projs = {}, {}
    for name, r in ref.items():
        gk = named[name].reshape(r.shape)
        rel = np.linalg.norm(gk - r) / (np.linalg.norm(r) + 1e-8)
        proj = float(np.sum(gk * r) / (np.sum(r * r) + 1e-30))
        rels[name], projs[name] = float(rel), proj
        assert rel < lim, f"{name}: relative Frobenius err {rel:.4f}"
        assert abs(proj - 1.0) < plim, f"{name}: gradient projection on the fp32 reference {proj:.4f}"
    print(f"[wd-grad-rel] batch {batch} kernel {kernel} " + " ".join(f"{k}={v:.4f}/{projs[k]:.4f}"
                                                                     for k, v in rels.items()))


@pytest.mark.gpu
def test_fused_step_matches_torch_trainer():
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    rec = synthetic_records(4096, seed=11)
    ft = FusedWideDeepTrainer(wdm.WideDeepModel(seed=4), batch=512, device=dev)
    ft.set_data(rec.to(dev))
    tt = TorchWideDeepTrainer(wdm.WideDeepModel(seed=4), batch=512)
    tt.set_data(rec)
    for _ in range(5):
        ft.step()
        tt.step()
    torch.cuda.synchronize()
    assert ft.steps_done == 5
    fm = ft.sync_to_model()
    dense, ids, label = wdm.records_to_tensors(rec[:2048])
    a = fm(dense, ids).detach()
    b = tt.model(dense, ids).detach()
    assert torch.corrcoef(torch.stack([a, b]))[0, 1] > 0.99
    assert (a - b).abs().mean() < 0.05


@pytest.mark.gpu
def test_fused_training_converges_and_graph_replay():
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=0), batch=4096, device=dev, loss_reduction="mean",
                              dnn_opt=OptSpec("adam", lr=3e-3), wide_opt=OptSpec("adam", lr=3e-2))
    tr.set_data(synthetic_records(1 << 18, device=dev, seed=3))
    tr.step()
    first = tr.last_loss() / 4096
    tr.capture()
    for _ in range(200):
        tr.step()
    torch.cuda.synchronize()
    last = tr.last_loss() / 4096
    assert tr.steps_done >= 200
    assert last < first - 0.03, (first, last)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["chain", "tile"])
def test_fused_predict_matches_torch(kernel):
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    m = wdm.WideDeepModel(seed=2)
    with torch.no_grad():
        m.wide.normal_(0, 0.5)
    tr = FusedWideDeepTrainer(m, batch=64, device=dev, kernel=kernel)
    rec = synthetic_records(5000, seed=8)
    got = tr.predict_logits(rec.to(dev)).cpu()
    mref = wdm.unpack_canonical(tr.param.cpu(), wdm.WideDeepModel(seed=2))
    dense, ids, _ = wdm.records_to_tensors(rec)
    ref = mref(dense, ids).detach()
    assert (got - ref).abs().max() < 0.05 * (ref.abs().max() + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["chain", "tile"])
def test_fused_training_is_run_to_run_deterministic(kernel):
    """Two trainers from the same init on the same data must produce bit-identical parameters:
    slab reduction is fixed-order; checks that the in-LDS wide-gradient accumulation is too."""
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    rec = synthetic_records(1 << 16, device=dev, seed=5)
    params = []
    for _ in range(2):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=1), batch=8192, device=dev, kernel=kernel)
        tr.set_data(rec)
        for _ in range(10):
            tr.step()
        torch.cuda.synchronize()
        params.append(tr.param.clone())
    diff = (params[0] - params[1]).abs().max().item()
    assert torch.equal(params[0], params[1]), f"max |diff| {diff}"


def test_stage_dims_cover_every_nonzero_weight():
    """The fused kernel stages only the live rows/granules of the bf16 weight image into LDS and
    zero-fills the rest: every non-zero entry of the packed image must lie inside the staged part."""
    m = wdm.WideDeepModel(seed=3)
    with torch.no_grad():
        for lin in list(m.dnn) + [m.head]:
            lin.bias.normal_()
    vec = wdm.pack_canonical(m)
    sd = wdm.stage_dims(m.cfg)
    rows, gpr = sd[:5], sd[5:]
    for li, (K, N) in enumerate(wdm.LAYER_KN):
        img = vec[wdm.LAYER_OFF[li]:wdm.LAYER_OFF[li] + K * N].reshape(N, K)
        n, k = np.nonzero(img)
        assert n.max() < rows[li] and k.max() < 8 * gpr[li], li
        staged = np.zeros_like(img)
        staged[:rows[li], :8 * gpr[li]] = img[:rows[li], :8 * gpr[li]]
        assert np.array_equal(staged, img)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["adagrad_ftrl", "adam", "sgd"])
@pytest.mark.parametrize("batch", [40, 16384])
def test_fused_reduce_opt_matches_two_launch_path(kind, batch):
    """wd_reduce_opt (full slab sum + optimizer in one launch) against wd_reduce -> wd_optimizer: the same
    update up to summation order. Compared after ONE step (over several steps the trajectories drift
    apart legitimately: a last-bit change of an fp32 master weight can flip its bf16 image). Adam checks
    the step counter: every optimizer workgroup keeps its own step slot; all must agree."""
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    opts = {"adagrad_ftrl": (None, None), "adam": (OptSpec("adam", lr=3e-3), OptSpec("adam", lr=1e-2)),
            "sgd": (OptSpec("sgd", lr=1e-4), OptSpec("sgd", lr=1e-4))}[kind]
    rec = synthetic_records(batch * 8, device=dev, seed=21)
    out, losses = [], []
    for fused_update in (False, True):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=6), batch=batch, device=dev, dnn_opt=opts[0],
                                  wide_opt=opts[1], fused_update=fused_update, kernel="tile")
        tr.set_data(rec)
        tr.step()
        torch.cuda.synchronize()
        out.append((tr.param.clone(), tr.s0.clone(), tr.s1.clone(), tr.wt.clone()))
        tr.capture(warmup=1)
        for _ in range(6):
            tr.step()
        torch.cuda.synchronize()
        assert tr.steps_done == 8 and bool((tr.step_ctr[:117] == 8).all())  # slots of the launched workgroups
        losses.append(tr.last_loss())
    for a, b, name in zip(out[0], out[1], ("param", "s0", "s1")):
        scale = a.abs().max().item() + 1e-6
        tol = (1e-3 if kind == "adam" else 2e-5) * scale  # Adam: m/sqrt(v) of a near-zero g is order noise
        assert (a - b).abs().max().item() <= tol, name
    # the bf16 weight image must be the rounding of the fp32 master
    assert torch.equal(out[1][0][: wdm.WTOT].to(torch.bfloat16).view(torch.int16), out[1][3])
    assert abs(losses[0] - losses[1]) <= 2e-2 * abs(losses[0]), losses


@pytest.mark.gpu
def test_reduce_full_matches_fp64_sum():
    from mifx.ops import wide_deep as wdk

    g = torch.Generator(device="cpu").manual_seed(3)
    for groups, stride in ((1, 20608), (7, 20608), (256, 20608), (300, 4096)):
        slab = torch.randn(groups, stride, generator=g).mul_(100).cuda()
        out = torch.empty(stride, device="cuda")
        wdk.reduce_full(slab, groups, out)
        ref = slab.double().sum(0)
        err = (out.double() - ref).abs().max().item()
        assert err <= 1e-6 * slab.abs().sum(0).max().item(), (groups, stride, err)


@pytest.mark.gpu
def test_xcd_local_reduce_matches_fp64_sum():
    """XCD-local two-level slab reduction (wd_reduce_xcd + wd_xcd_opt_sc): whatever XCD labels the rows carry --
    the real placement, labels no level-1 workgroup can match (XCD 13: the level-2 fallback sums them from the
    slab), or a random mix -- the result is the full column sum."""
    from mifx.ops import wide_deep as wdk

    g = torch.Generator(device="cpu").manual_seed(5)
    stride = 20608
    xr = wdk.XcdReduce(stride, "cuda")
    for groups in (256, 37, 1):
        slab = torch.randn(groups, stride, generator=g).mul_(10).cuda()
        ref = slab.double().sum(0)
        tol = 1e-6 * slab.abs().sum(0).max().item()
        for labels in (torch.arange(groups) % 8, torch.full((groups,), 13), torch.randint(0, 16, (groups,),
                                                                                            generator=g)):
            xr.xcd_of[:groups] = labels.to(torch.int32).cuda()
            out = torch.empty(stride, device="cuda")
            xr.sum_into(slab, groups, out)
            err = (out.double() - ref).abs().max().item()
            assert err <= tol, (groups, labels[:4].tolist(), err)


@pytest.mark.gpu
def test_chain_trainer_xcd_reduce_matches_plain_reduce():
    """The chained trainer's default single-GPU step (XCD-local reduction) against the plain slab reduction."""
    from mifx.data.synthetic import synthetic_records
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    recs = synthetic_records(1 << 16, device="cuda", seed=9)
    out = []
    for xcd in (True, False):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=3), batch=16384, device="cuda", in_kernel_tail=False)
        assert tr._xcd is not None  # grid 128
        if not xcd:
            tr._xcd = None
        tr.set_data(recs)
        for _ in range(4):
            tr.step()
        torch.cuda.synchronize()
        out.append(tr.param.clone())
    np.testing.assert_allclose(out[0].cpu().numpy(), out[1].cpu().numpy(), rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
def test_chain_trainer_recorded_xcd_reduce_matches_default(monkeypatch):
    """MIFX_WD_RES=0 selects the placement-recorded XCD reduction (XcdReduce: wd_reduce_xcd + wd_xcd_opt_sc<1> on
    the xcd_of the chained kernel records) instead of the residue-class default; both train the same."""
    from mifx.data.synthetic import synthetic_records
    from mifx.ops import wide_deep as wdk
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    recs = synthetic_records(1 << 16, device="cuda", seed=9)
    out = []
    for res, cls in (("0", wdk.XcdReduce), (None, wdk.ResReduce)):
        if res is None:
            monkeypatch.delenv("MIFX_WD_RES", raising=False)
        else:
            monkeypatch.setenv("MIFX_WD_RES", res)
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=3), batch=16384, device="cuda", in_kernel_tail=False)
        assert type(tr._xcd) is cls
        tr.set_data(recs)
        for _ in range(4):
            tr.step()
        torch.cuda.synchronize()
        assert tr.steps_done == 4
        out.append(tr.param.clone())
    np.testing.assert_allclose(out[0].cpu().numpy(), out[1].cpu().numpy(), rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [40, 16384])
def test_chain_kernel_step_matches_tile_kernel(batch):
    """The register-chained kernel against the LDS-tile kernel: same data, same init, one fused step each
    (gradient-slab sum + Adagrad/FTRL). Both are bf16 data paths with different accumulation orders, so the
    updates agree to a tolerance; the chained kernel's re-emitted C-ordered bf16 image must equal the image
    built from its own fp32 master weights."""
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    rec = synthetic_records(batch * 4, device=dev, seed=31)
    out = []
    for kernel in ("tile", "chain"):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=9), batch=batch, device=dev, kernel=kernel)
        tr.set_data(rec)
        tr.step()
        torch.cuda.synchronize()
        out.append((tr.param.clone(), tr.last_loss()))
        if kernel == "chain":
            img = torch.from_numpy(wdm.chain_image(tr.param.cpu())).to(dev).to(torch.bfloat16).view(torch.int16)
            assert torch.equal(img, tr.wt)
    (pa, la), (pb, lb) = out
    assert abs(la - lb) <= 1e-2 * abs(la) + 1e-3, (la, lb)
    d = (pa - pb).abs()
    assert d.max().item() <= 5e-3 * (pa.abs().max().item() + 1e-3), d.max().item()


def test_chain_maps_cover_trainable_parameters():
    """chain_maps: every trainable canonical parameter has its own slab slot inside a live tile, and the
    image map is a bijection onto the weight image's non-pad positions."""
    tmap, stride, gidx, mask, wmap = wdm.chain_maps()
    live = mask.astype(bool)
    assert len(np.unique(gidx[live])) == live.sum()
    assert (gidx[live] < stride).all()
    assert len(np.unique(wmap)) == wdm.WTOT and wmap.max() < wdm.CHAIN_LWEND
    m = wdm.WideDeepModel(seed=3)
    vec = wdm.pack_canonical(m)
    img = wdm.chain_image(vec)
    np.testing.assert_array_equal(img[wmap], vec[:wdm.WTOT])
    assert np.count_nonzero(img) == np.count_nonzero(vec[:wdm.WTOT])


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 40, 64])
def test_small_tile_training_matches_t128(batch):
    """The T = 64 build (csrc/wd_chain64.hip, 4 waves x 16 examples) against the T = 128 build on the same small
    batches: the dense dW tiles accumulate the same 32-example k-steps in the same order (bit-identical), the wide
    fixed-point histogram uses a finer scale at T = 64 (2^k / (iterations x T)), so whole training runs agree to
    rounding. Also run-to-run bit-identical, through multi-step graphs."""
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    rec = synthetic_records(4096, device=dev, seed=21)
    grads, params = {}, {}
    for small in (True, False, True):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=5), batch=batch, device=dev, small_tile=small)
        assert tr.tile == (64 if small else 128)
        tr.set_data(rec)
        g = tr.gradients_once()
        tr.capture(steps_per_graph=10)
        tr.run(200)
        torch.cuda.synchronize()
        if small in grads:
            np.testing.assert_array_equal(g, grads[small])
            assert torch.equal(tr.param, params[small])
        grads[small], params[small] = g, tr.param.clone()
    dense = tr.stride - wdm.WIDE_PAD  # the wide histogram is the last WIDE_PAD slab columns
    np.testing.assert_array_equal(grads[True][:dense], grads[False][:dense])
    np.testing.assert_allclose(grads[True][dense:], grads[False][dense:], rtol=0, atol=1e-5)
    assert torch.allclose(params[True], params[False], rtol=1e-3, atol=1e-4)


@pytest.mark.gpu
def test_multi_step_graph_matches_single_step_replays():
    """run(n) with a 7-step graph (2 multi-step replays + 3 one-step replays) must give exactly the parameters
    of 17 one-step replays: the data offset and optimizer step advance through the device-side step counter."""
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    rec = synthetic_records(1 << 16, device=dev, seed=12)
    out = []
    for spg in (1, 7):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=3), batch=2048, device=dev)
        tr.set_data(rec)
        tr.capture(steps_per_graph=spg)
        tr.run(17)
        torch.cuda.synchronize()
        assert tr.steps_done == 17 + 2  # + the capture's warmup steps
        out.append(tr.param.clone())
    assert torch.equal(out[0], out[1])


@pytest.mark.gpu
@pytest.mark.parametrize("batch,opt", [(65536, "adagrad_ftrl"), (16384, "adam"), (8192, "sgd"),
                                       (8192, "adagrad_ftrl_reg")])
def test_in_kernel_tail_step_matches_three_launch_step(batch, opt):
    """The one-launch step (slab reduction + optimizer inside the fused kernel after two grid barriers) against the
    three-launch step (fused, XCD-local reduce, reduce + optimizer) over 12 steps with multi-step hipGraph replays:
    same math, another fp32 association of the slab sum -> allclose; no barrier may time out. adagrad_ftrl_reg: FTRL
    with l1, l2 and the general lr_power branch (the three-launch side is anchored to an fp64 reference in
    tests/test_wd_optimizer.py)."""
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    recs = synthetic_records(1 << 18, device="cuda", seed=13)
    lr = 1e-3 if opt == "adam" else 1e-6  # (sum-reduced loss over the batch: plain SGD needs a tiny step)
    kw = {} if opt == "adagrad_ftrl" else _REG_OPTS if opt == "adagrad_ftrl_reg" else \
        {"dnn_opt": OptSpec(opt, lr=lr), "wide_opt": OptSpec(opt, lr=lr)}
    out = []
    for tail in (True, False):
        # (the three-launch side on the same T = 128 build: large_tile=False)
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=3), batch=batch, device="cuda", in_kernel_tail=tail,
                                  large_tile=False, **kw)
        assert (tr._ktail is not None) == tail
        tr.set_data(recs)
        tr.capture(steps_per_graph=5)
        tr.run(12)
        torch.cuda.synchronize()
        assert tr.steps_done == 14  # 2 capture warmup steps + 12
        if tail:
            assert int(tr._ktail.err.item()) == 0
        out.append((tr.param.clone(), tr.s0.clone(), tr.s1.clone(), tr.last_loss()))
    for a, b in zip(out[0][:3], out[1][:3]):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-4, atol=2e-6)
    assert np.isfinite(out[0][3]) and out[0][3] == pytest.approx(out[1][3], rel=1e-3)


@pytest.mark.gpu
def test_in_kernel_tail_is_run_to_run_deterministic_and_image_consistent():
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    recs = synthetic_records(1 << 18, device="cuda", seed=17)
    res = []
    for _ in range(2):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=4), batch=65536, device="cuda", in_kernel_tail=True)
        assert tr._ktail is not None
        tr.set_data(recs)
        for _ in range(6):
            tr.step()
        torch.cuda.synchronize()
        res.append(tr.param.clone())
        # the bf16 weight image the kernel re-emitted == the image built from its own fp32 master weights
        assert torch.equal(tr.wt, tr._weight_image())
    assert torch.equal(res[0], res[1])


@pytest.mark.gpu
@pytest.mark.parametrize("batch,opt", [(40, "adagrad_ftrl"), (128, "adagrad_ftrl"), (1, "adagrad_ftrl"),
                                       (40, "adam"), (77, "sgd"), (40, "ftrl"), (1, "adagrad_ftrl_reg")])
def test_persistent_small_batch_matches_slab_path(batch, opt):
    """The persistent single-workgroup kernel (n whole steps in one launch, weight image resident in LDS, optimizer
    in the workgroup) against the grid-1 slab path (fused kernel + reduce/optimizer kernel per step): the same fp32
    gradient and update, so parameters, optimizer state, the bf16 image and the loss must be BIT-identical. The data
    (300 records) wraps around several times over the 23 steps; run(n) split 1 + 20 + 2 checks the step counter
    carries the data offset and Adam's bias-correction step across launches."""
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    recs = synthetic_records(300, device="cuda", seed=21)
    lr = 1e-3 if opt == "adam" else 1e-4 if opt == "sgd" else None
    kw = {} if opt == "adagrad_ftrl" else _REG_OPTS if opt == "adagrad_ftrl_reg" else \
        {"dnn_opt": OptSpec(opt, lr=lr) if lr else OptSpec(opt, lr=0.05),
         "wide_opt": OptSpec(opt, lr=lr) if lr else OptSpec(opt, lr=0.2)}
    out = []
    for persistent in (True, False):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=5), batch=batch, device="cuda", persistent=persistent,
                                  small_tile=False, **kw)  # the T = 128 slab path it is bit-identical to
        assert tr._persist == persistent
        tr.set_data(recs)
        tr.step()
        tr.run(20)
        tr.run(2)
        torch.cuda.synchronize()
        assert tr.steps_done == 23
        out.append((tr.param.clone(), tr.s0.clone(), tr.s1.clone(), tr.wt.clone(), tr.last_loss()))
        if persistent:  # the image the kernel left behind == the image of its own fp32 master weights
            assert torch.equal(tr.wt, tr._weight_image())
    if opt == "adam":  # Adam's powf bias corrections: the two kernels' translation units are compiled with
        # different fp flags and may round powf differently in the last ulp -> tight allclose (a step off by one
        # would be ~1e-4 relative after 23 steps)
        for a, b in zip(out[0][:3], out[1][:3]):
            np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-6, atol=1e-8)
        assert out[0][4] == pytest.approx(out[1][4], rel=1e-6)
        return
    for a, b in zip(out[0][:4], out[1][:4]):
        assert torch.equal(a, b)
    assert np.isfinite(out[0][4]) and out[0][4] == out[1][4]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [4096, 65536])
def test_large_tile_matches_t128(batch):
    """The T = 256 build (csrc/wd_chain256.hip: 8 waves x 32 examples, one iteration per workgroup, layers 1-3
    staged in two 128-row passes) against the T = 128 build running two iterations per workgroup on the same
    batch: the same gradient up to the fp32 order of the per-workgroup sums (the examples land in other
    workgroups), the fp32 autograd gradient within the bf16 data path's error, and run-to-run bit-identical."""
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    rec = synthetic_records(batch * 3, device=dev, seed=33)
    G = batch // 256
    grads, params = {}, {}
    for large in (True, False, True):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=5), batch=batch, device=dev, max_grid=G, large_tile=large)
        assert (tr.tile, tr.grid) == ((256, G) if large else (128, G))
        tr.set_data(rec)
        g = tr.gradients_once()
        tr.capture(steps_per_graph=5)
        tr.run(10)
        torch.cuda.synchronize()
        if large in grads:
            np.testing.assert_array_equal(g, grads[large])
            assert torch.equal(tr.param, params[large])
        grads[large], params[large] = g, tr.param.clone()
    scale = np.abs(grads[False]).max()
    np.testing.assert_allclose(grads[True], grads[False], rtol=0, atol=2e-5 * scale)
    assert torch.allclose(params[True], params[False], rtol=2e-3, atol=2e-4)
    # the fp32 model's gradient on the first batch (the T = 256 step's own check)
    named = wdm.canonical_grad_to_torch(grads[True], wdm.WideDeepModel(seed=5), tr.gidx_np)
    _, ref = _torch_grads(wdm.WideDeepModel(seed=5), rec[:batch].cpu())
    for name, r in ref.items():
        rel = np.linalg.norm(named[name].reshape(r.shape) - r) / (np.linalg.norm(r) + 1e-8)
        assert rel < 0.06, f"{name}: relative Frobenius err {rel:.4f}"


@pytest.mark.gpu
@pytest.mark.parametrize("batch,opt", [pytest.param(40, "adagrad_ftrl", id="40"),
                                       pytest.param(100, "adagrad_ftrl", id="100"),
                                       pytest.param(40, "adagrad_ftrl_reg", id="40-adagrad_ftrl_reg")])
def test_one_launch_step_bit_identical(batch, opt):
    """The one-launch step (csrc/wd_chain.hip help_update: the optimizer in extra workgroups of the fused launch,
    waiting for workgroup 0's gradient row) trains bit-identically to the fused kernel + wd_opt1_sc two-kernel step:
    eager steps, captured multi-step graphs, and a checkpoint rewind in between (which resets the published-step
    flag). Batch 40: the T = 64 build; 100: the 8-wave T = 128 build. adagrad_ftrl_reg: FTRL with l1, l2 and
    lr_power = -0.75."""
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    dev = torch.device("cuda")
    rec = synthetic_records(batch * 5 + 77, device=dev, seed=43)
    kw = _REG_OPTS if opt == "adagrad_ftrl_reg" else {}
    out = {}
    for one in (False, True):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=8), batch=batch, device=dev, one_launch=one,
                                  shuffle_seed=0x5EED, **kw)
        assert (tr._one is not None) == one
        tr.set_data(rec)
        for _ in range(3):
            tr.step()
        tr.capture(steps_per_graph=4)  # (its warm-up steps are real steps)
        ck = tr.state_dict()
        tr.run(8)
        mid = tr.param.clone()
        tr.load_state_dict(ck)  # rewind and train the same 8 steps again
        tr.run(8)
        torch.cuda.synchronize()
        assert torch.equal(tr.param, mid)
        out[one] = (tr.param.clone(), tr.s0.clone(), tr.steps_done, tr.last_loss())
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    assert out[True][2] == out[False][2] and out[True][3] == out[False][3]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", [16384, 65536])
def test_res_reduce_fused_matches_two_launch(batch):
    """The one-launch residue-class tail (last-arriving residue workgroup applies the optimizer) against the
    two-launch default: bit-identical parameters, optimizer state and weight image after several steps, the graph
    replays included, and the per-chunk tickets back at zero."""
    from mifx.ops import wide_deep as wdk
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    recs = synthetic_records(1 << 17, device="cuda", seed=21)
    out = []
    for fused in (False, True):
        tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=5), batch=batch, device="cuda")
        assert isinstance(tr._xcd, wdk.ResReduce)
        tr._xcd.fused = fused
        tr.set_data(recs)
        for _ in range(3):
            tr.step()
        tr.run(12)
        torch.cuda.synchronize()
        out.append((tr.param_sc.clone(), tr.s0_sc.clone(), tr.s1_sc.clone(), tr.wt.clone()))
        if fused:
            assert int(tr._xcd.ticket.abs().sum()) == 0
    for a, b in zip(*out):
        assert torch.equal(a, b)
