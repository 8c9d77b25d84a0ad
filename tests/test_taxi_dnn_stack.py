"""KFP taxi DNN with hidden_units = [H1, .., HL]: model, CPU trainer, the `dnntrainer` step's export, and the GPU
stack kernels (csrc/tdnn_stack.hip + the first-layer entry points of csrc/embag_mlp.hip).

Every numeric check is against `Ref`, a double-precision implementation of the training step written here with plain
torch ops (forward, BCE sum, TF Adagrad with accumulators at 0.1); it does not import the trainer. Tolerances for
trained parameters and logits: rtol 1e-4, atol 1e-5; the loss at rel 1e-4. The fp32 CPU recipe uses at most 9 % of
that against `Ref` on these inputs, so a GPU result outside it is a defect."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from mifx.data.shuffle import record_indices
from mifx.models.taxi_dnn import TaxiDNN, TaxiDNNConfig
from mifx.trainer.taxi_dnn_trainer import TaxiDNNTrainer
from test_taxi_dnn import _data

RTOL, ATOL, LOSS_REL = 1e-4, 1e-5, 1e-4


class Ref:
    """fp64 step of the stack on global W1 rows: parameters `p` and Adagrad accumulators `acc` by state_dict name."""

    def __init__(self, model: TaxiDNN, lr=0.1, acc0=0.1):
        self.p = {k: v.detach().double().clone() for k, v in model.named_parameters()}
        self.acc = {k: torch.full_like(v, acc0) for k, v in self.p.items()}
        self.L = len(model.cfg.hidden_units)
        self.row0 = model.cfg.sparse_rows
        self.lr = lr
        self.loss = float("nan")

    def logits(self, p, rows, xd):
        a = torch.relu(p["b1"] + p["W1"][rows].sum(1) + xd.double() @ p["W1"][self.row0:])
        for k in range(self.L - 1):
            a = torch.relu(a @ p[f"Wh.{k}"] + p[f"bh.{k}"])
        return a @ p["w2"] + p["b2"]

    def step(self, rows, xd, y):
        p = {k: v.clone().requires_grad_(True) for k, v in self.p.items()}
        z, y = self.logits(p, rows, xd), y.double()
        # BCE with logits = log(1 + e^z) - z y, as logaddexp: stable, and differentiable at z == 0 exactly (a dead
        # last layer gives logit = b2 = 0 at the start), where clamp / abs forms have a subgradient that is not sigmoid - y
        loss = (torch.logaddexp(torch.zeros_like(z), z) - z * y).sum()
        names = list(p)
        for n, g in zip(names, torch.autograd.grad(loss, [p[n] for n in names])):
            self.acc[n] += g * g
            self.p[n] -= self.lr * g / self.acc[n].sqrt()
        self.loss = float(loss.detach())


@functools.lru_cache(maxsize=None)
def _case(units: tuple, batch: int, steps: int, n: int, seed: int):
    """(cfg, data, global rows, Ref after `steps` steps in stored record order); computed once, never modified."""
    cfg = TaxiDNNConfig(hidden_units=list(units))
    ids, dense, y = _data(n, cfg, seed=seed)
    model = TaxiDNN(cfg, seed=seed + 1)
    rows = model.rows(ids)
    ref = Ref(model)
    for s in range(steps):
        idx = torch.from_numpy(record_indices(s, batch, n, batch, 0, 0))
        ref.step(rows[idx], dense[idx], y[idx])
    return cfg, (ids, dense, y), rows, ref


def _check(tr: TaxiDNNTrainer, ref: Ref, data, rows):
    ids, dense, _ = data
    assert tr.last_loss() == pytest.approx(ref.loss, rel=LOSS_REL)
    sd = dict(tr.model.named_parameters())
    assert set(sd) == set(ref.p)
    for k, want in ref.p.items():
        torch.testing.assert_close(sd[k].detach().cpu().double(), want, rtol=RTOL, atol=ATOL, msg=lambda m: f"{k}: {m}")
    np.testing.assert_allclose(tr.predict_logits(ids, dense).astype(np.float64), ref.logits(ref.p, rows, dense).numpy(),
                               rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------------------------ model (CPU)

def test_stack_model_shapes_and_forward():
    cfg = TaxiDNNConfig(hidden_units=[64, 32])
    assert cfg.hidden == 64 and cfg.hidden_units == [64, 32]
    m = TaxiDNN(cfg, seed=1)
    assert sum(p.numel() for p in m.parameters()) == 6170 * 64 + 64 + 64 * 32 + 32 + 32 + 1
    assert [tuple(p.shape) for p in m.Wh] == [(64, 32)] and [tuple(p.shape) for p in m.bh] == [(32,)]
    assert tuple(m.w2.shape) == (32,)
    ids, dense, _ = _data(16, cfg)
    x = torch.zeros(16, cfg.input_dim)
    x.scatter_(1, m.rows(ids), 1.0)
    x[:, cfg.sparse_rows:] = dense
    want = torch.relu(torch.relu(x @ m.W1 + m.b1) @ m.Wh[0] + m.bh[0]) @ m.w2 + m.b2
    torch.testing.assert_close(m(ids, dense), want, rtol=1e-5, atol=1e-5)
    # exports pass their config as keywords
    m2 = TaxiDNN(hidden_units=[64, 32], seed=1)
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))


def test_one_layer_is_bit_identical_to_the_single_layer_model():
    g = torch.Generator().manual_seed(5)
    lim1, lim2 = (6.0 / (6170 + 64)) ** 0.5, (6.0 / (64 + 1)) ** 0.5
    W1 = (torch.rand(6170, 64, generator=g) * 2 - 1) * lim1
    w2 = (torch.rand(64, generator=g) * 2 - 1) * lim2
    for m in (TaxiDNN(TaxiDNNConfig(hidden=64), seed=5), TaxiDNN(TaxiDNNConfig(), seed=5, hidden=64),
              TaxiDNN(TaxiDNNConfig(hidden_units=[64]), seed=5)):
        assert m.cfg.hidden == 64 and m.cfg.hidden_units == [64]
        assert list(m.state_dict()) == ["W1", "b1", "w2", "b2", "offsets"]
        assert torch.equal(m.W1, W1) and torch.equal(m.w2, w2)
        assert not m.b1.any() and not m.b2.any()
    assert TaxiDNNConfig().hidden_units == [1500]
    for bad in ([], [16, 0], [-3]):
        with pytest.raises(ValueError):
            TaxiDNNConfig(hidden_units=bad)
    with pytest.raises(ValueError):
        TaxiDNNConfig(hidden=32, hidden_units=[16, 8])


def test_cpu_trainer_stack_matches_fp64_reference():
    cfg, data, rows, ref = _case((100, 70, 50), 32, 6, 32 * 3 + 17, 4)
    tr = TaxiDNNTrainer(TaxiDNN(cfg, seed=5), batch=32, lr=0.1, device="cpu")
    tr.set_data(*data)
    for _ in range(6):
        tr.step()
    _check(tr, ref, data, rows)


# ------------------------------------------------------------------------------------------------ dnntrainer (CPU)

def _transformed(tmp_path, n_train=400, n_eval=120):
    from mifx.io import dataset

    cfg = TaxiDNNConfig()
    tdir = tmp_path / "transformed"
    out = {}
    for split, n, seed in (("train", n_train, 1), ("eval", n_eval, 2)):
        ids, dense, y = _data(n, cfg, seed=seed)
        cols = {k: ids[:, i].numpy() for i, (k, _) in enumerate(cfg.sparse)}
        cols.update({k: dense[:, i].numpy() for i, k in enumerate(cfg.dense)})
        cols[cfg.label] = y.numpy().astype(np.int64)
        dataset.write_split(str(tdir / split), cols)
        out[split] = (ids, dense, y)
    return str(tdir), out


def _dnntrainer(tdir, outdir, hidden, steps=7, device="cpu", num_gpus=1):
    from mifx.kfp_components import taxi

    taxi.main(["dnntrainer", "--transformed_data_dir", tdir, "--training_output_dir", str(outdir),
               "--hidden_layer_size", hidden, "--steps", str(steps), "--device", device, "--num_gpus", str(num_gpus)])
    return os.path.join(str(outdir), "export", "export", "1")


def test_dnntrainer_trains_and_exports_every_layer(tmp_path, monkeypatch):
    from safetensors.torch import load_file

    from mifx.serving.saved_model import load

    monkeypatch.delenv("WORLD_SIZE", raising=False)
    tdir, splits = _transformed(tmp_path)
    export = _dnntrainer(tdir, tmp_path / "out", "16,8")
    meta = json.load(open(os.path.join(export, "saved_model.json")))
    assert meta["model_config"]["hidden_units"] == [16, 8]
    sd = load_file(os.path.join(export, "variables", "variables.safetensors"))
    assert tuple(sd["W1"].shape) == (6170, 16) and tuple(sd["Wh.0"].shape) == (16, 8)
    assert tuple(sd["bh.0"].shape) == (8,) and tuple(sd["w2"].shape) == (8,)
    model = load(export, "cpu").model
    assert isinstance(model, TaxiDNN) and model.cfg.hidden_units == [16, 8]
    # the same training run, here: the served model computes the trainer's logits
    tr = TaxiDNNTrainer(TaxiDNN(TaxiDNNConfig(hidden_units=[16, 8]), seed=0), batch=32, lr=0.1, device="cpu",
                        shuffle_seed=0x5EED)
    tr.set_data(*splits["train"])
    tr.run(7)
    eids, edense, _ = splits["eval"]
    with torch.no_grad():
        got = model(eids, edense).numpy()
    np.testing.assert_allclose(got, tr.predict_logits(eids, edense), rtol=1e-6, atol=1e-6)

    # an export written before hidden_units existed still loads
    old = tmp_path / "old_export"
    os.makedirs(old / "variables")
    from safetensors.torch import save_file

    m1 = TaxiDNN(TaxiDNNConfig(hidden=16), seed=3)
    save_file({k: v.detach().contiguous() for k, v in m1.state_dict().items()},
              str(old / "variables" / "variables.safetensors"))
    meta["model_config"] = {"hidden": 16, "seed": None}
    json.dump(meta, open(old / "saved_model.json", "w"))
    lm = load(str(old), "cpu").model
    assert lm.cfg.hidden_units == [16] and torch.equal(lm.W1, m1.W1) and torch.equal(lm.w2, m1.w2)


@pytest.mark.parametrize("hidden", ["16,0", "", "16,-2"])
def test_dnntrainer_rejects_bad_hidden_layer_size(tmp_path, monkeypatch, hidden):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="hidden_layer_size"):
        _dnntrainer(str(tmp_path / "nothing_is_read"), tmp_path / "out", hidden)


def test_dnntrainer_rejects_gpu_data_parallel_stack_before_launching_ranks(tmp_path, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="single-layer"):
        _dnntrainer(str(tmp_path / "nothing_is_read"), tmp_path / "out", "16,8", device="cuda", num_gpus=2)
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------------------------------------ GPU kernels

@pytest.mark.gpu
@pytest.mark.parametrize("units,batch", [((64, 32), 32), ((100, 70, 50), 32), ((100, 70, 50), 96), ((33, 7), 5),
                                         ((300, 70), 32), ((64, 1), 32)])
def test_hip_stack_step_matches_fp64_reference(units, batch):
    """6 eager steps. Widths off the 4 / 16 / 64 grids; B = 96 > 64: the chunked dense-row path; (33, 7) x 5: less than
    one MFMA tile in every dimension; 300: two 256-wide gather blocks, the second ragged; a width-1 layer."""
    cfg, data, rows, ref = _case(units, batch, 6, batch * 3 + 17, 4)
    tr = TaxiDNNTrainer(TaxiDNN(cfg, seed=5), batch=batch, lr=0.1, device="cuda", graph=False)
    assert tr.stack is not None
    tr.set_data(*data)
    for _ in range(6):
        tr.step()
    assert int(tr.step_ctr.item()) == 6
    _check(tr, ref, data, rows)


@pytest.mark.gpu
def test_hip_stack_graph_run_matches_reference_and_eager_bits():
    """run(23) = one eager step, 4 replays of a 5-step graph, 2 single-step replays, over records that wrap around;
    the summation order is fixed, so the same 23 steps launched eagerly give the same bits."""
    units, batch, steps = (100, 70, 50), 96, 23
    cfg, data, rows, ref = _case(units, batch, steps, batch * 3 + 17, 7)
    gr = TaxiDNNTrainer(TaxiDNN(cfg, seed=8), batch=batch, lr=0.1, device="cuda", steps_per_graph=5)
    ea = TaxiDNNTrainer(TaxiDNN(cfg, seed=8), batch=batch, lr=0.1, device="cuda", graph=False)
    for tr in (gr, ea):
        tr.set_data(*data)
    gr.run(steps)
    for _ in range(steps):
        ea.step()
    assert gr.graph_multi is not None and ea.graph is None
    assert gr.step_idx == steps and int(gr.step_ctr.item()) == steps and int(ea.step_ctr.item()) == steps
    _check(gr, ref, data, rows)
    for (k, a), (_, b) in zip(gr.model.named_parameters(), ea.model.named_parameters()):
        assert torch.equal(a, b), k
    for k in gr.accs:
        assert torch.equal(gr.accs[k], ea.accs[k]), k
    assert gr.last_loss() == ea.last_loss()


@pytest.mark.gpu
def test_hip_stack_zero_gradient_leaves_state_untouched():
    cfg = TaxiDNNConfig(hidden_units=[40, 24, 12])
    ids, dense, y = _data(64, cfg, seed=9)
    m = TaxiDNN(cfg, seed=9)
    dead = 5
    with torch.no_grad():
        m.bh[0][dead] = -1e6  # unit `dead` of layer 2 is off for every example
    tr = TaxiDNNTrainer(m, batch=32, lr=0.1, device="cuda", graph=False)
    tr.set_data(ids, dense, y)
    before = {k: (tr.params[k].clone(), tr.accs[k].clone()) for k in tr.params}
    tr.step()
    torch.cuda.synchronize()
    for k, sel in (("Wh.0", (slice(None), dead)), ("bh.0", (dead,)), ("Wh.1", (dead, slice(None)))):
        for now, was in zip((tr.params[k], tr.accs[k]), before[k]):
            assert torch.equal(now[sel], was[sel]), k
    live = [j for j in range(24) if j != dead]
    assert not torch.equal(tr.params["Wh.0"][:, live], before["Wh.0"][0][:, live])  # (the step did train)
    touched = torch.zeros(cfg.input_dim, dtype=torch.bool)
    touched[m.rows(ids[:32].cuda()).cpu().flatten()] = True
    touched[cfg.sparse_rows:] = True
    for now, was in zip((tr.params["W1"], tr.accs["W1"]), before["W1"]):
        assert torch.equal(now[~touched], was[~touched])
        assert not torch.equal(now[touched], was[touched])


@pytest.mark.gpu
def test_hip_stack_limits_raise_before_any_launch(tmp_path):
    from mifx.ops import tdnn_stack

    assert tdnn_stack.limits() == {"max_layers": 8, "max_hidden": 4096, "max_batch": 8192}
    torch.cuda.synchronize()
    mem = torch.cuda.memory_allocated()
    small = TaxiDNNConfig(sparse=[("a", 4)], dense=["x"], hidden_units=[8, 4097])
    with pytest.raises(ValueError, match="4096"):
        TaxiDNNTrainer(TaxiDNN(small, seed=0), batch=4, device="cuda")
    nine = TaxiDNNConfig(sparse=[("a", 4)], dense=["x"], hidden_units=[4] * 9)
    with pytest.raises(ValueError, match="9 hidden layers"):
        TaxiDNNTrainer(TaxiDNN(nine, seed=0), batch=4, device="cuda")
    torch.distributed.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        two = TaxiDNNConfig(sparse=[("a", 4)], dense=["x"], hidden_units=[8, 4])
        with pytest.raises(ValueError, match="single-layer"):
            TaxiDNNTrainer(TaxiDNN(two, seed=0), batch=4, device="cuda", process_group=torch.distributed.group.WORLD)
    finally:
        torch.distributed.destroy_process_group()
    assert torch.cuda.memory_allocated() == mem  # nothing reached the device
