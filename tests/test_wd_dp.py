"""Differentially private Wide&Deep training: per-example clipping inside the general fused gfx950 kernel
(csrc/wd_general.hip, DP mode) and the noise of its reduce / optimizer pass, against a CPU emulation of the kernel's
bf16 data path, brute-force per-example gradients in fp64, fp32 autograd, the host noise stream and the CPU DP
trainer; dispatch, estimator, accounting and the taxi module knobs."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import test_wd_general as twg
from mifx.data.shuffle import record_indices
from mifx.data.synthetic import synthetic_records
from mifx.models import wide_deep as wdm
from mifx.ops.dp import gaussian_noise_reference
from mifx.ops.wd_general import DP_SHRINK
from mifx.privacy import DPSpec
from mifx.privacy.rdp import compute_dp_sgd_privacy
from mifx.trainer.estimator import RunConfig, WideDeepEstimator
from mifx.trainer.fused_wide_deep import OptSpec
from mifx.trainer.torch_wide_deep import TorchWideDeepTrainer

S = float(DP_SHRINK)
TOWERS = {k: twg.TOWERS[k] for k in ("h2", "ref", "wide_narrow_wide", "six33")}
TOWERS["taxi"] = wdm.dnn_hidden_units()  # the default tower, forced onto the general kernel
# (batch, grid): 65 = a partial second tile, 400 on 2 workgroups = 3 and 4 tiles each
CASES = [(1, None), (40, None), (65, None), (400, 2)]
SGD = dict(dnn_opt=OptSpec("sgd", lr=0.1), wide_opt=OptSpec("sgd", lr=0.1))


# ------------------------------------------------------------------------------------------------ emulation
def _dp_emulation(model, rec, clip=None, reverse=False, detail=False):
    """The DP mode of the general kernel on the data path of test_wd_general._emulated_grads (padded layout, bf16
    weights / activations / dZ, fp32 accumulation, UNSCALED dl): per-example norms by the factorisation
    n_i^2 = sum_l (sum_{n < out_l} dZ_l[i,n]^2) (sum_k A_l[i,k]^2) + 10 dl_i^2, c_i = min(1, s C / n_i) (clip=None:
    c_i = 1), the clipped sum sum_i bf16(c_i dZ_l[i])^T A_l[i] plus the wide part with c_i dl_i. reverse: the same
    sums in another order. Returns (loss, norms [B], c [B], clipped gradient sum in flat order) and with detail the
    per-layer (dZ_l, A_l), dl and the wide columns."""
    cfg = model.cfg
    lay = wdm.general_layout(cfg)
    sc = np.zeros(lay.stride, np.float32)
    sc[lay.pidx] = wdm.pack_flat(model)
    sc[lay.ones] = 1.0
    vec = torch.from_numpy(sc)
    dense, ids, label = wdm.records_to_tensors(rec.cpu())
    B = len(label)
    outs = list(cfg.hidden_units) + [1]  # trainable outputs per layer: column out_l is the constant-1 producer

    def mm(a, b):
        return a.flip(1) @ b.flip(0) if reverse else a @ b

    def rowsum(a):
        return a.flip(1).sum(1) if reverse else a.sum(1)

    a = torch.zeros(B, lay.K[0])
    a[:, :3] = dense
    a[:, 3] = 1.0
    acts, wts = [twg._bf(a)], []
    nl = len(lay.K)
    for li, (K, N, off) in enumerate(zip(lay.K, lay.N, lay.off)):
        wt = twg._bf(vec[off:off + K * N].reshape(N, K))
        wts.append(wt)
        z = mm(acts[-1], wt.T)
        if li < nl - 1:
            acts.append(twg._bf(torch.relu(z)))
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
    dz = twg._bf(dz)
    dzs = {}
    n2 = 10.0 * dl * dl
    for li in range(nl - 1, -1, -1):
        dzs[li] = dz
        n2 = n2 + rowsum(dz[:, :outs[li]] ** 2) * rowsum(acts[li] ** 2)
        if li > 0:
            dz = twg._bf(mm(dz, wts[li]) * (acts[li] > 0).float())
    norms = torch.sqrt(n2)
    if clip is None:
        c = torch.ones(B)
    else:
        thr = torch.tensor(np.float32(S) * np.float32(clip))
        c = torch.where(norms > thr, thr / norms, torch.ones(B))
    grads = {}
    for li in range(nl):
        dzc = twg._bf(c[:, None] * dzs[li])
        grads[li] = (dzc.flip(0).T @ acts[li].flip(0)) if reverse else dzc.T @ acts[li]
    gw = torch.zeros(wdm.WIDE_PAD)
    order = torch.arange(B - 1, -1, -1) if reverse else torch.arange(B)
    dlc = c * dl
    gw.index_add_(0, idc[order].reshape(-1), dlc[order][:, None].expand(-1, 9).reshape(-1))
    gw[cfg.wide_rows] = dlc[order].sum()
    slab = torch.cat([grads[li].reshape(-1) for li in range(nl)] + [gw]).numpy()
    out = (float(loss), norms.numpy(), c.numpy(), slab[lay.pidx])
    if detail:
        out += ({"dz": dzs, "acts": acts, "dl": dl, "idc": idc, "lay": lay},)
    return out


def _brute_force_norms(model, rec):
    """fp64 norms of the per-example gradients formed entry by entry (outer products of the emulation's bf16 dZ_l
    and A_l rows, the wide one-hot columns and the bias), restricted to the trainable entries kind != -1."""
    _, _, _, _, d = _dp_emulation(model, rec, detail=True)
    lay = d["lay"]
    live = lay.kind != -1
    out = []
    for i in range(len(d["dl"])):
        parts = [torch.outer(d["dz"][li][i].double(), d["acts"][li][i].double()).reshape(-1)
                 for li in range(len(lay.K))]
        gw = torch.zeros(wdm.WIDE_PAD, dtype=torch.float64)
        gw[d["idc"][i]] = d["dl"][i].double()
        gw[model.cfg.wide_rows] = d["dl"][i].double()
        row = torch.cat(parts + [gw]).numpy()
        out.append(np.linalg.norm(row[live]))
    return np.asarray(out)


_DPC = {}


def _dp_case(name, batch):
    """Per (tower, batch), computed once: model, records, the unclipped emulation (norms forward / reverse), C at
    the median emulated norm, the clipped emulation forward / reverse."""
    key = (name, batch)
    if key not in _DPC:
        m = twg._model(TOWERS[name], seed=1)
        rec = synthetic_records(batch, seed=7)
        loss, n_f, _, _ = _dp_emulation(m, rec)
        _, n_r, _, _ = _dp_emulation(m, rec, reverse=True)
        clip = float(np.median(n_f))
        _, _, c_f, g_f = _dp_emulation(m, rec, clip=clip)
        _, _, _, g_r = _dp_emulation(m, rec, clip=clip, reverse=True)
        _DPC[key] = dict(model=m, rec=rec, loss=loss, n_f=n_f, n_r=n_r, clip=clip, c_f=c_f, g_f=g_f, g_r=g_r)
    return _DPC[key]


def _autograd_norms(model, rec):
    """fp32 autograd per-example gradient norms (torch.func.vmap on WideDeepModel, through the CPU DP trainer)."""
    tt = TorchWideDeepTrainer(copy.deepcopy(model), batch=rec.shape[0], dp=DPSpec(1e30, 0.0))
    tt.set_data(rec)
    tt._dp_gradient(torch.arange(rec.shape[0]), noise=False)
    return tt.last_norms().numpy()


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", ["h2", "h64_32"])
def test_factorised_norm_equals_brute_force(name):
    """n_i of the emulation == the norm of the per-example gradient over the trainable entries, 1e-6 relative.
    Counting the constant-1 producer column of dZ_l breaks this."""
    m = twg._model(twg.TOWERS[name], seed=1)
    rec = synthetic_records(7, seed=7)
    _, n, _, _ = _dp_emulation(m, rec)
    ref = _brute_force_norms(m, rec)
    rel = np.abs(n.astype(np.float64) - ref) / ref
    print(f"[wd-dp-factor] {name} max rel {rel.max():.3g}")
    assert rel.max() <= 1e-6
    # the unclipped emulation is the non-DP emulation
    _, _, _, g = _dp_emulation(m, rec)
    _, g0 = twg._emulated_grads(m, rec)
    np.testing.assert_array_equal(g, g0)


@pytest.mark.parametrize("name", list(TOWERS))
def test_emulation_clips_about_half_at_median(name):
    """C at the median emulated norm clips between 25 % and 75 % of a batch (one example: itself)."""
    for batch, _ in CASES:
        c = _dp_case(name, batch)
        frac = float((c["c_f"] < 1.0).mean())
        assert frac == 1.0 if batch == 1 else 0.25 <= frac <= 0.75, (name, batch, frac)


def _cpu_trainer(dp=None, hidden=(64, 32), batch=32, **kw):
    tr = TorchWideDeepTrainer(twg._model(list(hidden), seed=2), batch=batch, dp=dp, **SGD, **kw)
    tr.set_data(synthetic_records(256, seed=1))
    return tr


def test_torch_dp_trainer_noop_clip_small_clip_and_noise():
    plain, noop = _cpu_trainer(), _cpu_trainer(DPSpec(1e30, 0.0))
    plain.step()
    noop.step()
    for (k, a), b in zip(plain.model.state_dict().items(), noop.model.state_dict().values()):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), k  # fp32 batch sum against an fp64 sum of fp32 rows
    assert abs(plain.last_loss() - noop.last_loss()) <= 1e-5 * abs(plain.last_loss())
    n = noop.last_norms()
    assert n.shape == (32,) and (n > 0).all()
    clip = float(n.min()) / 4
    small = _cpu_trainer(DPSpec(clip, 0.0))
    small.step()
    assert torch.equal(small.last_norms(), n)
    assert (small._contrib_norms <= clip).all() and (small._contrib_norms >= 0.99 * clip).all()
    spec = DPSpec(float(n.median()), 0.7, seed=0x1234ABCD5)
    quiet, noisy = _cpu_trainer(DPSpec(spec.l2_norm_clip, 0.0)), _cpu_trainer(spec)
    lay = wdm.general_layout(noisy.model.cfg)
    for step in range(2):  # the stream is keyed by the step
        quiet.load_state_dict(noisy.state_dict())
        quiet.step()
        noisy.step()
        want = spec.stddev * gaussian_noise_reference(lay.stride, spec.seed, step)[lay.pidx]
        got = (noisy.last_grad_flat - quiet.last_grad_flat).numpy()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6)
    # and drives the update: SGD moves every parameter by -lr x that gradient
    d = wdm.pack_flat(noisy.model) - wdm.pack_flat(quiet.model)
    np.testing.assert_allclose(d, -0.1 * want, rtol=1e-3, atol=1e-6)


def test_dispatch_and_limits():
    from mifx.trainer.dispatch import check_world, make_wide_deep_trainer, select_kernel

    cfg = wdm.WideDeepConfig()
    assert select_kernel(cfg, None) == "chain" and select_kernel(cfg, None, dp=True) == "general"
    assert select_kernel(wdm.WideDeepConfig(hidden_units=[64, 32]), None, dp=True) == "general"
    assert select_kernel(cfg, "general", dp=True) == "general"
    for forced in ("chain", "tile"):
        with pytest.raises(ValueError, match="DP"):
            select_kernel(cfg, forced, dp=True)
    check_world(cfg, 2)  # the taxi tower trains data-parallel without DP
    with pytest.raises(ValueError, match="DP") as e:
        check_world(cfg, 2, dp=True)
    assert "hidden_units" not in str(e.value)
    with pytest.raises(ValueError, match="DP"):
        check_world(wdm.WideDeepConfig(hidden_units=[64, 32]), 2, "cpu", dp=True)
    check_world(cfg, 1, dp=True)
    with pytest.raises(ValueError, match="per example"):
        TorchWideDeepTrainer(twg._model([64, 32]), batch=32, dp=DPSpec(1.0, 1.0, num_microbatches=8))
    TorchWideDeepTrainer(twg._model([64, 32]), batch=32, dp=DPSpec(1.0, 1.0, num_microbatches=32))
    with pytest.raises(ValueError, match="l2_norm_clip"):
        DPSpec(0.0, 1.0)
    tr = make_wide_deep_trainer(twg._model([64, 32]), "cpu", batch=16, dp=DPSpec(1.0, 1.0))
    assert isinstance(tr, TorchWideDeepTrainer) and tr.dp_spec is not None
    from mifx.trainer.general_wide_deep import GeneralWideDeepTrainer

    with pytest.raises(ValueError, match="per example"):
        GeneralWideDeepTrainer(twg._model([64, 32]), batch=32, device="cpu", dp=DPSpec(1.0, 1.0, num_microbatches=4))


def test_privacy_spent_and_privacy_json(tmp_path):
    recs = synthetic_records(64 * 30, seed=3)
    est = WideDeepEstimator(RunConfig(model_dir=str(tmp_path / "m"), device="cpu", tf_random_seed=5),
                            hidden_units=[64, 32], batch_size=64, dp=DPSpec(1.5, 1.1))
    assert est.dp.seed == est.noise_seed() != 0  # seed 0: derived from tf_random_seed
    est.train(lambda: recs, 20)
    got = est.privacy_spent(len(recs), delta=1e-5)
    eps, _ = compute_dp_sgd_privacy(len(recs), 64, 1.1, 20 * 64 / len(recs), 1e-5)
    assert got == {"epsilon": eps, "delta": 1e-5, "noise_multiplier": 1.1, "l2_norm_clip": 1.5, "steps": 20,
                   "sampling_rate": 64 / len(recs)}
    assert np.isfinite(eps) and eps > 0
    path = est.export_saved_model(str(tmp_path / "export"))
    with open(os.path.join(path, "privacy.json")) as f:
        assert json.load(f) == got
    plain = WideDeepEstimator(RunConfig(model_dir=str(tmp_path / "p"), device="cpu"), hidden_units=[64, 32],
                              batch_size=64)
    plain.train(lambda: recs, 2)
    assert not os.path.exists(os.path.join(plain.export_saved_model(str(tmp_path / "ep")), "privacy.json"))
    with pytest.raises(RuntimeError):
        plain.privacy_spent(len(recs))


def test_taxi_module_reads_dp_knobs():
    import importlib.util

    path = os.path.join(os.path.dirname(__file__), "..", "examples", "taxi", "taxi_module.py")
    spec = importlib.util.spec_from_file_location("taxi_module_dp_under_test", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from mifx.trainer.estimator import HParams

    def est(custom):
        hp = HParams(custom_config=custom, device="cpu", serving_model_dir=None, warm_start_from=None,
                     transform_output=None, train_files=[], eval_files=[], train_steps=1, eval_steps=1)
        return mod.trainer_fn(hp, type("S", (), {"feature": []})())["estimator"]

    assert est({}).dp is None
    e = est({"dp_l2_norm_clip": 0.75, "dp_noise_multiplier": 1.3, "dp_delta": 1e-6})
    assert (e.dp.l2_norm_clip, e.dp.noise_multiplier, e.dp_delta) == (0.75, 1.3, 1e-6)
    assert est({"dp_l2_norm_clip": 1.0, "dp_noise_multiplier": 0.5}).dp_delta == 1e-5
    with pytest.raises(ValueError, match="both"):
        est({"dp_l2_norm_clip": 1.0})


def test_trainer_component_refuses_dp_with_several_gpus(tmp_path, monkeypatch):
    """num_gpus > 1 together with the DP knobs fails in the component, before any rank is launched."""
    from mifx.components.trainer import TrainerExecutor
    from mifx.trainer import distributed

    def no_launch(*a, **k):
        raise AssertionError("ranks were launched")

    monkeypatch.setattr(distributed, "launch", no_launch)
    art = lambda uri, **kw: type("A", (), dict(uri=str(uri), custom_properties={}, **kw))()  # noqa: E731
    inputs = {"transformed_examples": [art(tmp_path / "ex", split="train")], "schema": [art(tmp_path / "schema")]}
    props = {"module_file": "taxi_module.py", "train_args": {"num_steps": 1}, "eval_args": {"num_steps": 1},
             "custom_config": {"num_gpus": 2, "dp_l2_norm_clip": 1.0, "dp_noise_multiplier": 1.1}}
    with pytest.raises(ValueError, match="DP training is single-GPU"):
        TrainerExecutor().Do(inputs, {"output": [art(tmp_path / "out")]}, props)


# ------------------------------------------------------------------------------------------------ GPU
def _gpu(model, batch, dp, grid=None, **kw):
    tr = twg._general(copy.deepcopy(model), batch, dp=dp, **({"grid": grid} if grid else {}), **kw)
    if grid:
        assert tr.grid == grid and (batch + 63) // 64 >= 3 * grid  # several tiles per workgroup
    return tr


@pytest.mark.gpu
@pytest.mark.parametrize("batch,grid", CASES)
@pytest.mark.parametrize("name", list(TOWERS))
def test_dp_norms_match_emulation(name, batch, grid):
    """last_norms() against the emulation's n_i: 3 x the largest forward / reverse emulation difference, floor 1e-5
    of the largest norm (the margin convention of test_wd_general._case); against fp32 autograd printed, asserted
    for tower `ref` within the 0.125 of test_wd_general._check_gradients."""
    c = _dp_case(name, batch)
    tr = _gpu(c["model"], batch, DPSpec(c["clip"], 0.0), grid)
    tr.set_data(c["rec"].cuda())
    tr.gradients_once()
    got = tr.last_norms().cpu().numpy()
    assert got.shape == (batch,)
    err = float(np.abs(got - c["n_f"]).max())
    tol = max(3.0 * float(np.abs(c["n_f"] - c["n_r"]).max()), 1e-5 * float(c["n_f"].max()))
    ref = _autograd_norms(c["model"], c["rec"])
    rel = float((np.abs(got - ref) / ref).max())
    print(f"[wd-dp-norms] {name} B={batch} grid={tr.grid} max err {err:.3g} tol {tol:.3g} max n {c['n_f'].max():.3g} "
          f"worst rel to fp32 autograd {rel:.4f}")
    assert err <= tol
    if name == "ref":
        assert rel < 0.125


@pytest.mark.gpu
@pytest.mark.parametrize("batch,grid", CASES)
@pytest.mark.parametrize("name", list(TOWERS))
def test_dp_clipped_sum_matches_emulation(name, batch, grid):
    """C at the median emulated norm: about half the examples clip (a batch of one: the one example, which a
    fraction between 25 % and 75 % cannot describe). The clipped sum against the DP emulation, the unclipped loss."""
    c = _dp_case(name, batch)
    tr = _gpu(c["model"], batch, DPSpec(c["clip"], 0.0), grid)
    tr.set_data(c["rec"].cuda())
    got = tr.gradients_once()[tr.gidx_np]
    frac = float((tr.last_norms().cpu().numpy() > np.float32(S) * np.float32(c["clip"])).mean())
    em = c["g_f"]
    tol = max(2e-3 * float(np.abs(em).max()) + 1e-5, 3.0 * float(np.abs(em - c["g_r"]).max()))
    err = float(np.abs(got - em).max())
    loss = tr.last_loss()
    print(f"[wd-dp-sum] {name} B={batch} grid={tr.grid} clipped {frac:.2f} max err {err:.3g} tol {tol:.3g} "
          f"max|em| {np.abs(em).max():.3g} loss {loss:.6g} / {c['loss']:.6g}")
    assert frac == 1.0 if batch == 1 else 0.25 <= frac <= 0.75
    assert err <= tol
    assert abs(loss - c["loss"]) <= 1e-3 * abs(c["loss"])
    assert tr.steps_done == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TOWERS))
def test_dp_sensitivity_of_one_example(name):
    """B = 1, one workgroup, 32 records, every one clipped (C = a quarter of the smallest norm), no noise: the fp64
    norm of what the example contributes to the trainable columns is <= C (1 + 1e-5) -- fp32 accumulation and the
    fixed-point wide histogram; the bf16 rounding is inside the shrink s -- and >= 0.97 C. A kernel that rescales dl
    and reruns the chain fails this."""
    m = twg._model(TOWERS[name], seed=1)
    rec = synthetic_records(32, seed=19)
    _, n_em, _, _ = _dp_emulation(m, rec)
    clip = float(n_em.min()) / 4
    tr = _gpu(m, 1, DPSpec(clip, 0.0), shuffle_seed=0)
    assert tr.grid == 1
    tr.set_data(rec.cuda())
    live = tr.layout.kind != -1
    worst_hi, worst_lo = 0.0, np.inf
    for k in range(32):
        assert list(record_indices(k, 1, 32)) == [k]
        tr.set_step(k)
        g = tr.gradients_once().astype(np.float64)
        assert abs(float(tr.last_norms()[0]) - n_em[k]) <= 0.02 * n_em[k]  # record k it is
        nrm = float(np.linalg.norm(g[live]))
        worst_hi, worst_lo = max(worst_hi, nrm / clip), min(worst_lo, nrm / clip)
    print(f"[wd-dp-sens] {name} C {clip:.4g} realised norm / C in [{worst_lo:.6f}, {worst_hi:.6f}]")
    assert worst_hi <= 1.0 + 1e-5
    assert worst_lo >= 0.97


@pytest.mark.gpu
@pytest.mark.parametrize("batch,grid", [(40, None), (400, 2)])
@pytest.mark.parametrize("name", list(TOWERS))
def test_dp_noop_clip_is_bit_identical_to_plain(name, batch, grid):
    c = _dp_case(name, batch)
    plain = twg._general(copy.deepcopy(c["model"]), batch, **({"grid": grid} if grid else {}))
    priv = _gpu(c["model"], batch, DPSpec(1e30, 0.0), grid)
    for tr in (plain, priv):
        tr.set_data(c["rec"].cuda())
    a, b = plain.gradients_once(), priv.gradients_once()
    assert a.tobytes() == b.tobytes()
    assert plain.last_loss() == priv.last_loss()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TOWERS))
def test_dp_noise_matches_host_stream(name):
    c = _dp_case(name, 40)
    spec = DPSpec(c["clip"], 1.3, seed=0xABCDEF12345)
    tr = _gpu(c["model"], 40, spec)
    tr.set_data(synthetic_records(400, seed=7).cuda())
    live = tr.layout.kind != -1
    seen = []
    for step in (0, 3):
        tr.set_step(step)
        noisy, clean = tr.gradients_once(noise=True), tr.gradients_once(noise=False)
        d = noisy - clean
        want = spec.stddev * gaussian_noise_reference(tr.stride, spec.seed, step)
        np.testing.assert_allclose(d[live], want[live], rtol=1e-4, atol=2e-5 * spec.stddev)
        assert (d[~live] == 0).all()
        assert tr.steps_done == step
        seen.append(d)
    assert np.abs(seen[0] - seen[1])[live].max() > 0.1 * spec.stddev
    tr.set_step(0)
    tr.run(3)
    torch.cuda.synchronize()
    ones = torch.from_numpy(tr.layout.ones).cuda()
    assert tr.steps_done == 3 and (tr.param_sc[ones] == 1.0).all()
    pad = tr.param_sc[torch.from_numpy(~live).cuda()]  # padding stays 0, the constant-1 producers 1
    assert ((pad == 0.0) | (pad == 1.0)).all()


@pytest.mark.gpu
def test_dp_graph_replay_and_seed_determinism():
    """test_general_graph_replay_bit_identical with DP and noise: eager == single-step graph == 5-step graph after 12
    steps, last_norms() too; the same seed reproduces the run, another seed does not."""
    rec = synthetic_records(2000, device="cuda", seed=6)
    out = {}
    for mode, seed in (("eager", 11), ("single", 11), ("multi", 11), ("again", 11), ("other", 12)):
        tr = twg._general(twg._model(twg.TOWERS["h64_32"], seed=3, perturb=False), 200, shuffle_seed=5,
                          dp=DPSpec(1.0, 0.8, seed=seed))
        tr.set_data(rec)
        if mode in ("single", "multi"):
            tr.capture(warmup=0, steps_per_graph=5 if mode == "multi" else 1)
            assert (tr.graph_multi is not None) == (mode == "multi")
        tr.run(5)
        torch.cuda.synchronize()
        assert tr.steps_done == 5
        tr.run(7)
        torch.cuda.synchronize()
        assert tr.steps_done == 12
        out[mode] = dict(tr.state_dict(), norms=tr.last_norms().cpu())
    frac = float((out["eager"]["norms"] > S).float().mean())
    assert 0.05 < frac  # the clip is active
    for mode in ("single", "multi", "again"):
        for k in ("param", "s0", "s1", "step", "norms"):
            assert torch.equal(out["eager"][k], out[mode][k]), (mode, k)
    assert not torch.equal(out["eager"]["param"], out["other"]["param"])


@pytest.mark.gpu
@pytest.mark.parametrize("noise_multiplier", [0.0, 0.5])
def test_dp_feed_parity_with_torch_dp_trainer(noise_multiplier):
    """test_general_feed_parity_with_torch_trainer with DP on both sides (C at the median norm of the first batch):
    30 steps, mean |dparam| < 0.05, without noise and with noise_multiplier 0.5 (both trainers add the same noise)."""
    rec = synthetic_records(4096, seed=11)
    kw = dict(batch=256, shuffle_seed=0x1234567, feed_stride=300, feed_offset=17)
    probe = TorchWideDeepTrainer(twg._model(twg.TOWERS["ref"], seed=4, perturb=False), dp=DPSpec(1e30, 0.0), **kw)
    probe.set_data(rec)
    probe._dp_gradient(probe._batch_idx(), noise=False)
    spec = DPSpec(float(probe.last_norms().median()), noise_multiplier, seed=77)
    gt = twg._general(twg._model(twg.TOWERS["ref"], seed=4, perturb=False), dp=spec, **kw)
    gt.set_data(rec.cuda())
    tt = TorchWideDeepTrainer(twg._model(twg.TOWERS["ref"], seed=4, perturb=False), dp=spec, **kw)
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
    print(f"[wd-dp-feed] noise_multiplier {noise_multiplier} C {spec.l2_norm_clip:.4g} mean |dparam| {d:.4g} "
          f"loss {np.mean(losses[:5]):.4f} -> {np.mean(losses[-5:]):.4f}")
    assert d < 0.05


@pytest.mark.gpu
def test_dp_estimator_end_to_end(tmp_path):
    """WideDeepEstimator(dp=...) on the GPU with the default taxi tower: the general kernel, checkpoint + resume
    bit-identical to the uninterrupted run (the noise is keyed by the step), export, serving, privacy.json."""
    from mifx.serving import saved_model
    from mifx.trainer.general_wide_deep import GeneralWideDeepTrainer

    recs = synthetic_records(64 * 30, seed=3)
    inp = lambda: recs.cuda()  # noqa: E731
    spec = DPSpec(1.0, 0.9)

    def est(d, every):
        return WideDeepEstimator(RunConfig(model_dir=str(tmp_path / d), save_checkpoints_steps=every,
                                           keep_checkpoint_max=1, device="cuda"), batch_size=64, steps_per_graph=7,
                                 dp=spec)

    full = est("full", 100).train(inp, 40)
    tr = full._trainer
    assert isinstance(tr, GeneralWideDeepTrainer) and tr.kernel == "general" and tr.dp.seed == full.noise_seed()
    assert full.cfg.hidden_units == wdm.dnn_hidden_units()
    est("part", 15).train(inp, 30)
    b = est("part", 15)
    assert b.global_step == 30
    b.train(inp, 40)
    assert twg._same_model(full.model, b.model)
    fs, bs = full._trainer.state_dict(), b._trainer.state_dict()
    for k in ("param", "s0", "s1"):
        assert torch.equal(fs[k].cpu(), bs[k].cpu()), k
    want = b.predict_logits(recs[:333].cuda())
    path = b.export_saved_model(str(tmp_path / "export"))
    with open(os.path.join(path, "privacy.json")) as f:
        spent = json.load(f)
    assert spent == b.privacy_spent(len(recs)) and spent["steps"] == 40 and np.isfinite(spent["epsilon"])
    loaded = saved_model.load(path, device="cuda")
    dense, ids, _ = wdm.records_to_tensors(recs[:333])
    cols = {k: dense[:, j].numpy() for j, k in enumerate(b.cfg.dense_features)}
    cols.update({k: ids[:, j].numpy() for j, (k, _) in enumerate(b.cfg.wide)})
    got = loaded.wd_logits(cols)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=0.05 * (np.abs(want).max() + 1))
