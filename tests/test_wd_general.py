"""Wide&Deep on any DNN tower: the tower-independent checkpoint layout (CPU) and the general fused gfx950 kernel
(csrc/wd_general.hip; GPU) against a CPU emulation of its bf16 data path, fp32 autograd, the chained kernel and an
fp64 optimizer reference."""
import numpy as np
import pytest
import torch

import test_wd_optimizer as two
from mifx.data.synthetic import synthetic_records
from mifx.models import wide_deep as wdm
from mifx.trainer.estimator import RunConfig, WideDeepEstimator
from mifx.trainer.fused_wide_deep import OptSpec
from mifx.trainer.torch_wide_deep import TorchWideDeepTrainer

TOWERS = {"h2": [2], "h64_32": [64, 32], "ref": [100, 70, 50, 25], "five": [100, 70, 48, 34, 20],
          "wide_narrow_wide": [256, 17, 256], "six33": [33] * 6}
BATCHES = [1, 40, 64, 65, 1000]


def _model(hidden, seed=1, perturb=True):
    m = wdm.WideDeepModel(wdm.WideDeepConfig(hidden_units=list(hidden)), seed=seed)
    if perturb:
        g = torch.Generator().manual_seed(seed + 100)
        with torch.no_grad():
            m.wide.copy_(torch.randn(m.wide.shape, generator=g) * 0.3)
            m.wide_bias.fill_(-0.2)
            for lin in list(m.dnn) + [m.head]:
                lin.bias.copy_(torch.randn(lin.bias.shape, generator=g) * 0.1)
    return m


def _same_model(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


# ------------------------------------------------------------------------------------------------ CPU: layouts
@pytest.mark.parametrize("hidden", [[64, 32], [128, 64, 32, 16], [100, 70, 48, 34, 20], [2]])
def test_pack_flat_roundtrip_and_general_maps(hidden):
    m = _model(hidden, seed=3)
    vec = wdm.pack_flat(m)
    assert vec.dtype == np.float32 and vec.size == wdm.flat_size(m.cfg)
    dims = [3] + list(hidden) + [1]
    assert vec.size == sum(dims[i + 1] * (dims[i] + 1) for i in range(len(dims) - 1)) + 2128
    # layer blocks are [n_out][n_in + 1] with the bias in the last column; wide weights and wide bias follow
    first = vec[:hidden[0] * 4].reshape(hidden[0], 4)
    np.testing.assert_array_equal(first[:, :3], m.dnn[0].weight.detach().numpy())
    np.testing.assert_array_equal(first[:, 3], m.dnn[0].bias.detach().numpy())
    np.testing.assert_array_equal(vec[-2128:-1], m.wide.detach().numpy())
    assert vec[-1] == np.float32(-0.2)
    m2 = wdm.unpack_flat(vec, _model(hidden, seed=9, perturb=False))
    assert _same_model(m, m2)
    np.testing.assert_array_equal(wdm.pack_flat(m2), vec)
    with pytest.raises(ValueError):
        wdm.unpack_flat(vec[:-1], m2)
    # the towers outside the canonical padding checkpoint in the flat layout
    assert not wdm.uses_canonical_layout(m.cfg)
    np.testing.assert_array_equal(wdm.pack_state(m), vec)

    # general kernel maps: parameter -> slab column -> both bf16 images
    lay = wdm.general_layout(m.cfg)
    assert lay.stride == lay.wtot + wdm.WIDE_PAD and lay.stride % 4 == 0
    assert lay.pidx.size == vec.size and len(np.unique(lay.pidx)) == vec.size  # every trainable entry exactly once
    trainable = np.zeros(lay.stride, bool)
    trainable[lay.pidx] = True
    np.testing.assert_array_equal(lay.kind != -1, trainable)  # ... and nothing else: no padding, no constant 1
    assert not trainable[lay.ones].any() and len(lay.ones) == len(hidden)
    nd = vec.size - 2128
    assert (lay.kind[lay.pidx[:nd]] >= 0).all() and (lay.kind[lay.pidx[nd:]] == -2).all()
    assert (lay.pidx[nd:] == lay.wtot + np.arange(2128)).all()
    # image maps: W^T entry (n, k) of layer l sits at its slab column; the transposed image holds it at (k, n)
    kn = lay.kind[lay.pidx[:nd]]
    assert len(np.unique(kn)) == nd and kn.max() < lay.wtot
    for li, (K, N, off) in enumerate(zip(lay.K, lay.N, lay.off)):
        assert K % 32 == 0 and N % 16 == 0 and K >= dims[li] + 1 and N >= dims[li + 1] + (li < len(hidden))
        cols = np.arange(off, off + K * N)
        live = cols[lay.kind[cols] >= 0]
        n, k = (live - off) // K, (live - off) % K
        assert n.max() == dims[li + 1] - 1 and k.max() == dims[li]
        np.testing.assert_array_equal(lay.kind[live], off + k * N + n)
    # the descriptor the kernel reads
    d = lay.desc
    assert d[0] == len(hidden) + 1 and d[1] == max(lay.K) + wdm.GEN_PAD and d[2] == lay.wtot


def test_default_tower_state_dict_is_canonical():
    """Towers inside the canonical padding keep today's vectors byte for byte."""
    m = _model(wdm.dnn_hidden_units(), seed=2)
    assert wdm.uses_canonical_layout(m.cfg)
    tr = TorchWideDeepTrainer(m, batch=32)
    tr.set_data(synthetic_records(256, seed=1))
    tr.run(3)
    sd = tr.state_dict()
    assert sd["param"].numel() == wdm.WTOT + wdm.NWIDE
    assert sd["param"].numpy().tobytes() == wdm.pack_canonical(tr.model).tobytes()
    assert wdm.pack_state(tr.model).tobytes() == wdm.pack_canonical(tr.model).tobytes()
    assert sd["s0"].numel() == sd["s1"].numel() == wdm.WTOT + wdm.NWIDE


def test_torch_trainer_checkpoints_any_tower():
    """[64, 32] on the CPU: 5 steps, state_dict, a fresh trainer, 5 more == 10 uninterrupted steps, bit for bit."""
    rec = synthetic_records(640, seed=4)
    kw = dict(batch=48, shuffle_seed=7, feed_stride=64, feed_offset=8)
    full = TorchWideDeepTrainer(_model([64, 32], seed=5, perturb=False), **kw)
    full.set_data(rec)
    full.run(10)
    a = TorchWideDeepTrainer(_model([64, 32], seed=5, perturb=False), **kw)
    a.set_data(rec)
    a.run(5)
    sd = a.state_dict()
    assert sd["param"].numel() == wdm.flat_size(a.model.cfg) == sd["s0"].numel() == sd["s1"].numel()
    b = TorchWideDeepTrainer(_model([64, 32], seed=77, perturb=False), **kw)
    b.load_state_dict(sd)
    b.set_data(rec)
    assert b.steps_done == 5
    b.run(5)
    assert _same_model(full.model, b.model)
    fs, bs = full.state_dict(), b.state_dict()
    for k in ("param", "s0", "s1", "step"):
        assert torch.equal(fs[k], bs[k]), k


def _resume_case(tmp_path, device, hidden):
    recs = synthetic_records(64 * 30, seed=3)
    inp = lambda: recs.to(device)  # noqa: E731

    def est(d, every):
        return WideDeepEstimator(RunConfig(model_dir=str(tmp_path / d), save_checkpoints_steps=every,
                                           keep_checkpoint_max=1, device=device), hidden_units=hidden, batch_size=64,
                                 steps_per_graph=7)

    full = est("full", 100).train(inp, 40)
    est("part", 15).train(inp, 30)
    b = est("part", 15)  # constructed again on the same model_dir: resumes from ckpt-30
    assert b.global_step == 30
    b.train(inp, 40)
    assert _same_model(full.model, b.model)
    fs, bs = full._trainer.state_dict(), b._trainer.state_dict()
    for k in ("param", "s0", "s1"):
        assert torch.equal(fs[k].cpu(), bs[k].cpu()), k
    return full, b, recs


def test_estimator_cpu_resume_any_tower(tmp_path):
    _resume_case(tmp_path, "cpu", [64, 32])


def test_limits_raise_value_errors(monkeypatch):
    from mifx.trainer.dispatch import check_world
    from mifx.trainer.general_wide_deep import GeneralWideDeepTrainer

    with pytest.raises(ValueError, match="1 to 6 hidden layers"):
        wdm.general_layout(wdm.WideDeepConfig(hidden_units=[8] * 7))
    with pytest.raises(ValueError, match=r"width in \[2, 256\]"):
        wdm.general_layout(wdm.WideDeepConfig(hidden_units=[64, 257]))
    with pytest.raises(ValueError, match=r"width in \[2, 256\]"):
        wdm.general_layout(wdm.WideDeepConfig(hidden_units=[1]))
    with pytest.raises(ValueError, match="1 to 6 hidden layers"):
        GeneralWideDeepTrainer(_model([8] * 7), batch=8, device="cpu")
    with pytest.raises(ValueError, match="single-GPU"):
        check_world(wdm.WideDeepConfig(hidden_units=[64, 32]), 2)
    check_world(wdm.WideDeepConfig(), 2)  # the taxi tower trains data-parallel on the chained kernel
    check_world(wdm.WideDeepConfig(hidden_units=[64, 32]), 2, "cpu")  # and every tower on the CPU trainer
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="single-GPU"):
        GeneralWideDeepTrainer(_model([64, 32]), batch=8, device="cpu", process_group=object())


def test_taxi_module_reads_tower_knobs():
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(__file__), "..", "examples", "taxi", "taxi_module.py")
    spec = importlib.util.spec_from_file_location("taxi_module_under_test", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from mifx.trainer.estimator import HParams

    def hidden(custom):
        hp = HParams(custom_config=custom, device="cpu", serving_model_dir=None, warm_start_from=None,
                     transform_output=None, train_files=[], eval_files=[], train_steps=1, eval_steps=1)
        schema = type("S", (), {"feature": []})()
        return mod.trainer_fn(hp, schema)["estimator"].cfg.hidden_units

    assert hidden({}) == [100, 70, 48, 34]
    assert hidden({"first_dnn_layer_size": 64, "num_dnn_layers": 2, "dnn_decay_factor": 0.5}) == [64, 32]


def test_taxi_tower_study_job_and_trial(capsys):
    """The StudyJob searches the three tower knobs; the trial trains that tower and prints what the study parses."""
    import importlib.util
    import os
    import random

    from mifx.hpo.study import StudySpec, parse_metrics

    root = os.path.join(os.path.dirname(__file__), "..")
    spec = StudySpec.from_yaml(os.path.join(root, "examples", "hpo", "taxi-tower-search-job.yaml"))
    assert spec.objective == "auc" and spec.metrics == ["loss"] and spec.optimization == "maximize"
    assert [p.name for p in spec.parameters] == ["--first-dnn-layer-size", "--num-dnn-layers", "--dnn-decay-factor"]
    assert "examples/hpo/taxi_tower_trial.py" in spec.command
    rng = random.Random(1)
    for _ in range(20):  # every point of the search space is a tower the general kernel accepts
        first, layers, decay = (p.sample(rng) for p in spec.parameters)
        wdm.check_general_compatible(wdm.WideDeepConfig(hidden_units=wdm.dnn_hidden_units(first, layers, decay)))
    ms = importlib.util.spec_from_file_location("taxi_tower_trial_under_test",
                                                os.path.join(root, "examples", "hpo", "taxi_tower_trial.py"))
    mod = importlib.util.module_from_spec(ms)
    ms.loader.exec_module(mod)
    mod.main(["--first-dnn-layer-size=24", "--num-dnn-layers=2", "--dnn-decay-factor=0.5", "--steps=20",
              "--records=600", "--device=cpu"])
    out = capsys.readouterr().out
    assert "hidden_units=[24, 12]" in out
    got = parse_metrics(out, [spec.objective] + spec.metrics)
    assert set(got) == {"auc", "loss"} and 0.0 <= got["auc"] <= 1.0 and np.isfinite(got["loss"])


# ------------------------------------------------------------------------------------------------ emulation
def _bf(x):
    return x.to(torch.bfloat16).float()


def _emulated_grads(model, rec, reverse=False):
    """fp32 emulation of the general kernel's data path on the padded layout of general_layout (bf16 weights,
    activations rounded after ReLU, dZ rounded after the ReLU mask, fp32 accumulation), generalising
    tests/test_wide_deep.py::_emulated_grads. reverse: the same sums in another order (examples reversed in the
    dW / wide sums, K reversed in the forward and dA products). Returns (loss, gradient in flat order)."""
    cfg = model.cfg
    lay = wdm.general_layout(cfg)
    sc = np.zeros(lay.stride, np.float32)
    sc[lay.pidx] = wdm.pack_flat(model)
    sc[lay.ones] = 1.0
    vec = torch.from_numpy(sc)
    dense, ids, label = wdm.records_to_tensors(rec.cpu())
    B = len(label)

    def mm(a, b):  # a [m, k] @ b [k, n], optionally with the k axis reversed
        return a.flip(1) @ b.flip(0) if reverse else a @ b

    a = torch.zeros(B, lay.K[0])
    a[:, :3] = dense
    a[:, 3] = 1.0
    acts, wts = [_bf(a)], []
    nl = len(lay.K)
    for li, (K, N, off) in enumerate(zip(lay.K, lay.N, lay.off)):
        wt = _bf(vec[off:off + K * N].reshape(N, K))
        wts.append(wt)
        z = mm(acts[-1], wt.T)
        if li < nl - 1:
            acts.append(_bf(torch.relu(z)))
        else:
            deep = z[:, 0]
    nb = torch.tensor([n for _, n in cfg.wide])
    idc = torch.where(ids < nb, ids, torch.zeros_like(ids)) + torch.tensor(cfg.wide_offsets)
    wvec = vec[lay.wtot:]
    x = deep + wvec[idc].sum(1) + wvec[cfg.wide_rows]
    loss = torch.nn.functional.binary_cross_entropy_with_logits(x, label, reduction="sum")
    dl = torch.sigmoid(x) - label
    dz = torch.zeros(B, lay.N[-1])
    dz[:, 0] = dl
    dz = _bf(dz)
    grads = {}
    for li in range(nl - 1, -1, -1):
        grads[li] = (dz.flip(0).T @ acts[li].flip(0)) if reverse else dz.T @ acts[li]  # dWt [N][K]
        if li > 0:
            dz = _bf(mm(dz, wts[li]) * (acts[li] > 0).float())
    gw = torch.zeros(wdm.WIDE_PAD)
    order = torch.arange(B - 1, -1, -1) if reverse else torch.arange(B)
    gw.index_add_(0, idc[order].reshape(-1), dl[order][:, None].expand(-1, 9).reshape(-1))
    gw[cfg.wide_rows] = dl[order].sum()
    slab = torch.cat([grads[li].reshape(-1) for li in range(nl)] + [gw]).numpy()
    return float(loss), slab[lay.pidx]


_EM = {}


def _case(name, batch):
    """(model, records, loss, emulated gradient, elementwise bound), computed once per (tower, batch)."""
    key = (name, batch)
    if key not in _EM:
        m = _model(TOWERS[name], seed=1)
        rec = synthetic_records(batch, seed=7)
        loss, em = _emulated_grads(m, rec)
        tol = 2e-3 * np.abs(em).max() + 1e-5  # the project's bound (tests/test_wide_deep.py)
        if not wdm.uses_canonical_layout(m.cfg):
            # a tower outside the old padding: 3 x the largest difference between two emulations that differ only in
            # accumulation order, where that is more (the margin convention of tests/test_attention.py)
            _, em_r = _emulated_grads(m, rec, reverse=True)
            tol = max(tol, 3.0 * float(np.abs(em - em_r).max()))
        _EM[key] = (m, rec, loss, em, tol)
    return _EM[key]


def _torch_grads(model, rec):
    dense, ids, label = wdm.records_to_tensors(rec.cpu())
    model.zero_grad()
    loss = model.loss(dense, ids, label, reduction="sum")
    loss.backward()
    return {n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()}


def _general(model, batch, **kw):
    from mifx.trainer.dispatch import make_wide_deep_trainer
    from mifx.trainer.general_wide_deep import GeneralWideDeepTrainer

    tr = make_wide_deep_trainer(model, "cuda", batch=batch, kernel="general", **kw)
    assert isinstance(tr, GeneralWideDeepTrainer)
    return tr


def _check_gradients(name, batch, grid=None):
    import copy

    m, rec, loss_em, em, tol = _case(name, batch)
    tr = _general(copy.deepcopy(m), batch, **({"grid": grid} if grid else {}))
    if grid:
        assert tr.grid == grid and (batch + 63) // 64 >= 3 * grid  # several tiles per workgroup
    tr.set_data(rec.cuda())
    got = tr.gradients_once()[tr.gidx_np]
    torch.cuda.synchronize()
    assert tr.steps_done == 0  # gradients_once does not update
    err = np.abs(got - em)
    loss = tr.last_loss()
    print(f"[wdg-grad] {name} B={batch} grid={tr.grid} max err {err.max():.3g} tol {tol:.3g} "
          f"max|em| {np.abs(em).max():.3g} loss {loss:.6g} / {loss_em:.6g}")
    assert err.max() <= tol, f"max err {err.max():.3g} > {tol:.3g}; worst flat idx {np.argsort(-err)[:5]}"
    assert abs(loss - loss_em) <= 1e-3 * abs(loss_em)
    # fp32 autograd: asserted for the reference's own default tower at the batch sizes of
    # test_fused_gradients_match_torch (its limits), printed otherwise
    named = wdm.flat_grad_to_torch(got, m)
    ref = _torch_grads(copy.deepcopy(m), rec)
    lim = 0.125 if batch < 1000 else 0.06
    plim = 0.05 if batch < 1000 else 0.02
    out = []
    for k, r in ref.items():
        gk = named[k].reshape(r.shape)
        rel = float(np.linalg.norm(gk - r) / (np.linalg.norm(r) + 1e-8))
        proj = float(np.sum(gk * r) / (np.sum(r * r) + 1e-30))
        out.append(f"{k}={rel:.4f}/{proj:.4f}")
        if name == "ref" and batch in (40, 64, 1000):
            assert rel < lim, f"{k}: relative Frobenius err {rel:.4f}"
            assert abs(proj - 1.0) < plim, f"{k}: gradient projection on the fp32 reference {proj:.4f}"
    print(f"[wdg-grad-rel] {name} B={batch} " + " ".join(out))


# ------------------------------------------------------------------------------------------------ GPU: gradients
@pytest.mark.gpu
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("name", list(TOWERS))
def test_general_gradients_match_emulation(name, batch):
    _check_gradients(name, batch)


@pytest.mark.gpu
def test_general_gradients_two_workgroups_many_tiles():
    """The slab accumulation path: 2 workgroups, 8 tiles each."""
    _check_gradients("ref", 1000, grid=2)
    _check_gradients("wide_narrow_wide", 1000, grid=2)


@pytest.mark.gpu
def test_general_forced_on_default_tower_matches_chained():
    from mifx.trainer.dispatch import make_wide_deep_trainer
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    batch = 1000
    rec = synthetic_records(batch * 3, device="cuda", seed=33)
    hidden = wdm.dnn_hidden_units()
    ch = make_wide_deep_trainer(_model(hidden, seed=5), "cuda", batch=batch)
    assert isinstance(ch, FusedWideDeepTrainer) and ch.kernel == "chain"  # dispatch: the default tower is unchanged
    ge = _general(_model(hidden, seed=5), batch)
    ch.set_data(rec)
    ge.set_data(rec)
    m = _model(hidden, seed=5)
    _, em = _emulated_grads(m, rec[:batch])
    tol = 2e-3 * np.abs(em).max() + 1e-5
    g_ch = wdm.canonical_grad_to_torch(ch.gradients_once(), m, ch.gidx_np)
    g_ge = wdm.flat_grad_to_torch(ge.gradients_once()[ge.gidx_np], m)
    for k in g_ch:
        d = float(np.abs(g_ch[k].reshape(-1) - g_ge[k].reshape(-1)).max())
        print(f"[wdg-vs-chain] {k} max diff {d:.3g} tol {tol:.3g}")
        assert d <= tol, k
    ch.run(20)
    ge.run(20)
    torch.cuda.synchronize()
    assert ch.steps_done == ge.steps_done == 20
    pc, pg = ch.param.cpu(), ge.param.cpu()  # both canonical: the default tower keeps today's checkpoint layout
    assert pc.shape == pg.shape
    live = torch.from_numpy(ch.mask.cpu().numpy().astype(bool))
    assert torch.allclose(pg[live], pc[live], rtol=2e-3, atol=2e-4), float((pg[live] - pc[live]).abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["h2", "ref", "wide_narrow_wide", "six33"])
def test_general_predict_matches_torch(name):
    m = _model(TOWERS[name], seed=2)
    tr = _general(m, 64)
    for n in (1, 5000):
        rec = synthetic_records(n, seed=8)
        got = tr.predict_logits(rec.cuda()).cpu()
        dense, ids, _ = wdm.records_to_tensors(rec)
        ref = m(dense, ids).detach()
        assert got.shape == ref.shape
        assert (got - ref).abs().max() < 0.05 * (ref.abs().max() + 1), (name, n)


# ------------------------------------------------------------------------------------------------ GPU: reduce + opt
_OPT_CONFIGS = dict(two.CONFIGS)
_OPT_CONFIGS["adam_step999"] = (OptSpec("adam", lr=3e-3), OptSpec("adam", lr=1e-2), 998)  # first step is 999


def _exact_slab(G, sums, rng):
    """float32 [G, stride] with entries k * 2**-8 whose column sums are exactly `sums` (k * 2**-8) in any order."""
    slab = (rng.integers(-64, 65, size=(G, sums.size)).astype(np.float64) * 2.0 ** -8)
    slab[G - 1] = sums - slab[:G - 1].sum(0)
    out = slab.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), slab) and np.array_equal(out.astype(np.float64).sum(0), sums)
    assert np.array_equal(out.sum(0, dtype=np.float32).astype(np.float64), sums)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(_OPT_CONFIGS))
def test_general_reduce_opt_matches_fp64_reference(name):
    """wdg_reduce_opt on the [64, 32] tower's layout: 3 steps against the fp64 reference of
    tests/test_wd_optimizer.py (its tolerance rule: 8 x the fp32 numpy error + 2 ulp); slab entries k * 2**-8 with the
    same exact column sums for every row count, so 1, 2, 9 and 256 rows must give bit-identical results; sentinels on
    every padding entry of param / s0 / s1 and on every image entry no parameter owns."""
    from mifx.ops import wd_general as wdg

    dnn_spec, wide_spec, step0 = _OPT_CONFIGS[name]
    specs = (dnn_spec, wide_spec)
    lay = wdm.general_layout(wdm.WideDeepConfig(hidden_units=[64, 32]))
    stride, wtot = lay.stride, lay.wtot
    rng = np.random.default_rng([stride, 5])
    sums = rng.integers(-512, 513, size=stride).astype(np.float64) * 2.0 ** -8
    live, dnn = lay.kind != -1, lay.kind >= 0
    case = two.Case(live, dnn, [sums * mlt for mlt in two.STEP_MULT], specs, np.random.default_rng([stride, 3]))
    ref = two.reference(case, specs, step0)
    two.assert_l1_split(case, specs, ref, name)
    dev = torch.device("cuda")
    slots = wdg.constants()["SLOTS"]
    img_owned = np.zeros(2 * wtot, bool)
    img_owned[np.flatnonzero(dnn)] = True
    img_owned[wtot + lay.kind[dnn]] = True
    results = {}
    for G in (1, 2, 9, 256):
        base = _exact_slab(G, sums, np.random.default_rng([G, 11]))
        p, s0, s1 = (torch.from_numpy(v.copy()).to(dev) for v in case.init)
        img = torch.full((2 * wtot,), two.WT_SENTINEL, dtype=torch.int16, device=dev)
        ctr = torch.full((slots,), step0, dtype=torch.int64, device=dev)
        kind = torch.from_numpy(lay.kind).to(dev)
        for i, mlt in enumerate(two.STEP_MULT):
            slab = torch.from_numpy(base * np.float32(mlt)).to(dev)
            wdg.reduce_apply(slab, G, kind, p, s0, s1, img, ctr, dnn_spec.encode(), wide_spec.encode())
            torch.cuda.synchronize()
            got = [v.cpu().numpy() for v in (p, s0, s1)]
            for k, tname in enumerate(("param", "s0", "s1")):
                err = float(np.abs(got[k][live].astype(np.float64) - ref[i].val[k][live]).max())
                print(f"[wdg-opt] {name} G={G} step {i} {tname}: err {err:.3g} bound {ref[i].bound[k]:.3g}")
                assert err <= ref[i].bound[k], (name, G, i, tname, err, ref[i].bound[k])
                assert np.array_equal(got[k][~live], np.full((~live).sum(), two.SENTINEL[k])), (name, G, i, tname)
            im = img.cpu().numpy().view(np.uint16)
            want = torch.from_numpy(got[0]).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            assert np.array_equal(im[:wtot][dnn[:wtot]], want[:wtot][dnn[:wtot]])
            assert np.array_equal(im[wtot + lay.kind[dnn]], want[dnn])
            assert (im[~img_owned] == two.WT_SENTINEL).all()
            # a reduced row count must not change the plain sum either
            out = torch.empty(stride, device=dev)
            wdg.reduce_sum(slab, G, out)
            assert np.array_equal(out.cpu().numpy().astype(np.float64), sums * mlt)
        assert int(ctr[0].item()) == step0 + len(two.STEP_MULT)
        used = (stride // 4 + 255) // 256
        assert (ctr[:used] == step0 + len(two.STEP_MULT)).all()
        results[G] = got
    for G in (2, 9, 256):
        for a, b in zip(results[1], results[G]):
            assert a.tobytes() == b.tobytes(), (name, G)


# ------------------------------------------------------------------------------------------------ GPU: trainer
@pytest.mark.gpu
def test_general_training_is_deterministic():
    rec = synthetic_records(5000, device="cuda", seed=5)
    states = []
    for _ in range(2):
        tr = _general(_model(TOWERS["ref"], seed=1, perturb=False), 1000, shuffle_seed=11)
        tr.set_data(rec)
        tr.run(20)
        torch.cuda.synchronize()
        states.append(tr.state_dict())
    for k in ("param", "s0", "s1", "step"):
        assert torch.equal(states[0][k], states[1][k]), k
    assert int(states[0]["step"][0]) == 20


@pytest.mark.gpu
def test_general_graph_replay_bit_identical():
    """A 5-step graph == 5 single replays == 5 eager steps; steps_done counts them."""
    rec = synthetic_records(2000, device="cuda", seed=6)
    out = {}
    for mode in ("eager", "single", "multi"):
        tr = _general(_model(TOWERS["h64_32"], seed=3, perturb=False), 200, shuffle_seed=5)
        tr.set_data(rec)
        if mode != "eager":
            tr.capture(warmup=0, steps_per_graph=5 if mode == "multi" else 1)
            assert (tr.graph_multi is not None) == (mode == "multi")
        tr.run(5)
        torch.cuda.synchronize()
        assert tr.steps_done == 5
        tr.run(7)  # multi: one 5-step replay + 2 single replays
        torch.cuda.synchronize()
        assert tr.steps_done == 12
        out[mode] = tr.state_dict()
    for mode in ("single", "multi"):
        for k in ("param", "s0", "s1", "step"):
            assert torch.equal(out["eager"][k], out[mode][k]), (mode, k)


@pytest.mark.gpu
def test_general_feed_parity_with_torch_trainer():
    """30 steps beside the CPU trainer on the same shuffled, strided, offset record stream."""
    rec = synthetic_records(4096, seed=11)
    kw = dict(batch=256, shuffle_seed=0x1234567, feed_stride=300, feed_offset=17)
    gt = _general(_model(TOWERS["ref"], seed=4, perturb=False), **kw)
    gt.set_data(rec.cuda())
    tt = TorchWideDeepTrainer(_model(TOWERS["ref"], seed=4, perturb=False), **kw)
    tt.set_data(rec)
    losses = []
    for _ in range(30):
        gt.step()
        tt.step()
        losses.append(gt.last_loss() / 256)
    torch.cuda.synchronize()
    assert gt.steps_done == 30
    a, b = gt.state_dict()["param"], tt.state_dict()["param"]
    d = float((a - b).abs().mean())
    print(f"[wdg-feed] mean |dparam| {d:.4g} loss {np.mean(losses[:5]):.4f} -> {np.mean(losses[-5:]):.4f}")
    assert d < 0.05
    assert np.mean(losses[-5:]) < np.mean(losses[:5])


@pytest.mark.gpu
def test_general_estimator_resume_and_serving(tmp_path):
    """WideDeepEstimator on the GPU with the reference's default tower: checkpoint + resume bit-identical to the
    uninterrupted run, finite metrics; export -> saved_model.load -> wd_logits equals the estimator's logits."""
    from mifx.serving import saved_model
    from mifx.trainer.general_wide_deep import GeneralWideDeepTrainer

    full, b, recs = _resume_case(tmp_path, "cuda", TOWERS["ref"])
    assert isinstance(b._trainer, GeneralWideDeepTrainer)
    m = b.evaluate(lambda: recs[:500].cuda())
    assert all(np.isfinite(m[k]) for k in ("loss", "average_loss", "accuracy", "auc")), m
    want = b.predict_logits(recs[:333].cuda())
    path = b.export_saved_model(str(tmp_path / "export"))
    loaded = saved_model.load(path, device="cuda")
    assert loaded.device.type == "cuda"
    cols = {}
    dense, ids, _ = wdm.records_to_tensors(recs[:333])
    for j, k in enumerate(b.cfg.dense_features):
        cols[k] = dense[:, j].numpy()
    for j, (k, _) in enumerate(b.cfg.wide):
        cols[k] = ids[:, j].numpy()
    got = loaded.wd_logits(cols)
    assert isinstance(loaded._fused, GeneralWideDeepTrainer)
    np.testing.assert_array_equal(got, want)
