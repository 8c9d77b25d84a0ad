"""The BERT fine-tuning recipe on FlatAdamW (csrc/adamw.hip): global-norm clipping, in-graph linear
warmup / decay schedule, per-parameter weight decay; through BertTrainer, its CLI and the pipeline component.

Master / m / v tolerance: the project's AdamW tolerance (tests/test_flat_adamw.py), rtol 1e-5, atol 1e-6."""
import json
import os
import types

import pytest
import torch

from mifx.ops.adamw import scheduled_lr
from mifx.trainer.optim import FlatAdamW

TOL = dict(rtol=1e-5, atol=1e-6)


def _no_decay(p):
    return p.ndim <= 1


def _mlp():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.LayerNorm(7), torch.nn.Linear(7, 3))


def _lambda(warmup, total):
    return lambda t: t / max(1, warmup) if t < warmup else max(0.0, (total - t) / max(1, total - warmup))


# ---------------------------------------------------------------------------------------------------- CPU
def test_cpu_recipe_matches_stock_pytorch():
    """C1: the reference (FlatAdamW on the CPU) against torch.optim.AdamW with two param groups, clip_grad_norm_
    and LambdaLR. The schedule ("linear", 2, 6) has lr_t = 0 at updates 0, 6 and 7: those leave the parameters
    bitwise unchanged."""
    m1, m2 = _mlp(), _mlp()
    dec, nod = [p for p in m1.parameters() if p.ndim > 1], [p for p in m1.parameters() if p.ndim <= 1]
    ref = torch.optim.AdamW([{"params": dec, "weight_decay": 0.01}, {"params": nod, "weight_decay": 0.0}], lr=1e-2)
    sched = torch.optim.lr_scheduler.LambdaLR(ref, _lambda(2, 6))
    opt = FlatAdamW(m2.parameters(), lr=1e-2, weight_decay=0.01, dtype=torch.float32, max_grad_norm=0.5,
                    schedule=("linear", 2, 6), no_decay=_no_decay)
    x = torch.randn(16, 5)
    clipped = 0
    for i in range(8):
        ref.zero_grad()
        m1(x).pow(2).sum().backward()
        torch.nn.utils.clip_grad_norm_(m1.parameters(), 0.5)
        ref.step()
        sched.step()
        before = opt.flat.clone()
        opt.zero_grad()
        m2(x).pow(2).sum().backward()
        opt.step()
        clipped += opt.last_grad_norm() > 0.5
        assert opt.last_lr() == pytest.approx(1e-2 * _lambda(2, 6)(i), rel=1e-6)
        if i in (0, 6, 7):
            assert opt.last_lr() == 0.0 and torch.equal(opt.flat, before)
        else:
            assert not torch.equal(opt.flat, before)
        for a, b in zip(m1.parameters(), m2.parameters()):
            torch.testing.assert_close(b, a, **TOL)
    assert clipped > 0  # the clipping was active
    assert int(opt.step_count) == 8


def test_value_errors():
    """C2."""
    for bad in (("linear", 3, 3), ("linear", 4, 3), ("linear", -1, 3), ("cosine", 1, 3)):
        with pytest.raises(ValueError):
            FlatAdamW(_mlp().parameters(), dtype=torch.float32, schedule=bad)
    for kw in (dict(max_grad_norm=1.0), dict(schedule=("linear", 1, 3)), dict(no_decay=_no_decay)):
        with pytest.raises(ValueError, match="overlap"):
            FlatAdamW(_mlp().parameters(), dtype=torch.float32, overlap=True, **kw)

    from mifx.models.bert import BertConfig
    from mifx.trainer.bert_trainer import BertTrainer

    cfg = BertConfig.tiny()
    tp2 = types.SimpleNamespace(size=2, rank=0, ipc=None)  # raises before the model is built
    with pytest.raises(ValueError, match="max_grad_norm"):
        BertTrainer(cfg, 2, 16, "cpu", tp=tp2, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="graph"):
        BertTrainer(cfg, 2, 16, "cpu", flat_adamw=False, graph=True, warmup_steps=1, total_steps=4)
    with pytest.raises(ValueError):
        BertTrainer(cfg, 2, 16, "cpu", warmup_steps=4, total_steps=4)


def test_checkpoint_resume_continues_the_schedule():
    """C3: 3 steps, state_dict() into a fresh optimizer, 3 steps == 6 straight steps, bitwise."""
    kw = dict(lr=1e-2, weight_decay=0.01, dtype=torch.float32, max_grad_norm=0.5, schedule=("linear", 2, 6),
              no_decay=_no_decay)
    x = torch.randn(16, 5, generator=torch.Generator().manual_seed(3))

    def run(model, opt, n):
        for _ in range(n):
            opt.zero_grad()
            model(x).pow(2).sum().backward()
            opt.step()

    ma = _mlp()
    oa = FlatAdamW(ma.parameters(), **kw)
    run(ma, oa, 6)
    mb = _mlp()
    ob = FlatAdamW(mb.parameters(), **kw)
    run(mb, ob, 3)
    sd = {k: v.clone() for k, v in ob.state_dict().items()}
    mc = _mlp()
    oc = FlatAdamW(mc.parameters(), **kw)
    oc.load_state_dict(sd)
    assert int(oc.step_count) == 3 and oc.last_lr() == ob.last_lr()
    run(mc, oc, 3)
    for name in ("flat", "master", "m", "v"):
        assert torch.equal(getattr(oc, name), getattr(oa, name)), name
    assert int(oc.step_count) == 6
    for a, c in zip(ma.parameters(), mc.parameters()):
        assert torch.equal(a, c)


def test_component_records_resolved_optimizer_settings(tmp_path):
    """C4: the BertTrainer component on the CPU with a linear schedule."""
    from mifx.components import EvalArgs, TrainArgs
    from mifx.components.bert import BertTrainer, TextExampleGen
    from mifx.orchestration import LocalDagRunner, Pipeline

    tiny = dict(vocab_size=1000, hidden=64, layers=2, heads=4, intermediate=128, max_position=64, dropout=0.0)
    eg = TextExampleGen(num_synthetic=96, seq_len=32, vocab_size=1000, num_labels=2, seed=3)
    tr = BertTrainer(examples=eg.outputs.examples, train_args=TrainArgs(num_steps=8), eval_args=EvalArgs(num_steps=1),
                     custom_config=dict(tiny, tp=1, batch_size=8, learning_rate=1e-3, graph=False, lr_schedule="linear",
                                        warmup_proportion=0.5, max_grad_norm=1.0, no_decay_bias_norm=True))
    p = Pipeline(pipeline_name="recipe", pipeline_root=str(tmp_path / "recipe"), components=[eg, tr],
                 metadata_db_root=str(tmp_path / "md"))
    res = LocalDagRunner(device="cpu").run(p)
    assert res.succeeded
    art = res.components["BertTrainer"].outputs["output"][0]
    o = json.load(open(os.path.join(art.uri, "metrics.json")))["optimizer"]
    assert o["lr_schedule"] == "linear" and o["warmup_steps"] == 4 and o["total_steps"] == 8
    assert o["warmup_proportion"] == 0.5 and o["max_grad_norm"] == 1.0 and o["no_decay_bias_norm"] is True
    assert o["learning_rate"] == 1e-3
    assert o["final_lr"] == pytest.approx(1e-3 * (8 - 7) / (8 - 4), rel=1e-6)  # the 8th update runs at t = 7
    assert o["final_grad_norm"] > 0


# ---------------------------------------------------------------------------------------------------- GPU
# numel 1, 7, 8, 2047, 2048 (exactly one chunk), 2049, 5000 (several chunks + tail); then a parameter that never
# gets a gradient and one whose gradient is a 2-byte-offset view (the unaligned scalar path over 3 chunks)
SHAPES = [(1,), (7,), (2, 4), (2047,), (2048,), (2049,), (50, 100), (13,), (4099,)]
NOGRAD, OFFSET = 7, 8


def _edge_params(device):
    g = torch.Generator().manual_seed(11)
    return [torch.nn.Parameter(torch.randn(s, generator=g).bfloat16().to(device)) for s in SHAPES]


def _edge_grads(seed):
    """bf16 randn * 0.1 per parameter on the CPU (None for the gradient-less one)."""
    g = torch.Generator().manual_seed(seed)
    out = [(torch.randn(s, generator=g) * 0.1).bfloat16() for s in SHAPES]
    out[NOGRAD] = None
    return out


def _assign(params, grads, device):
    for i, (p, g) in enumerate(zip(params, grads)):
        if g is None:
            p.grad = None
        elif i == OFFSET and device != "cpu":
            buf = torch.zeros(g.numel() + 8, dtype=torch.bfloat16, device=device)
            buf[1:1 + g.numel()].copy_(g)
            p.grad = buf[1:1 + g.numel()]
            assert p.grad.data_ptr() % 16 == 2 and p.grad.is_contiguous()
        else:
            p.grad = g.to(device)


def _norm64(grads):
    return float(sum(g.double().pow(2).sum() for g in grads if g is not None).sqrt())


@pytest.mark.gpu
def test_gpu_global_norm_edge_shapes_and_reproducible():
    """G1. 1e-5 relative: each thread adds at most 8 squares, then a 256-wide tree, all fp32 (a few 2^-24)."""
    params = _edge_params("cuda")
    opt = FlatAdamW(params, lr=1e-3, weight_decay=0.01, max_grad_norm=0.25)
    assert opt.mode == "own" and opt._partial.numel() == opt.bp.numel() == 14
    grads = _edge_grads(5)
    _assign(params, grads, "cuda")
    want = _norm64(grads)
    opt._partial.fill_(float("nan"))  # every partial is rewritten on every launch
    opt.step()
    first = opt.clip.clone()
    opt.step()
    torch.cuda.synchronize()
    coef, norm = first.tolist()
    print(f"norm {norm!r} fp64 {want!r} rel {abs(norm - want) / want:.3e} coef {coef!r}")
    assert abs(norm - want) <= 1e-5 * want
    assert opt.last_grad_norm() == norm
    assert coef == pytest.approx(0.25 / (want + 1e-6), rel=1e-5) and coef < 1
    assert torch.equal(opt.clip, first)  # bit-identical on a second run
    assert float(opt._partial[opt.bp == NOGRAD].abs().sum()) == 0.0 and bool(torch.isfinite(opt._partial).all())


@pytest.mark.gpu
@pytest.mark.parametrize("nblocks", [3, 4099, 20003])
def test_gpu_global_norm_many_partials(nblocks):
    """The one-workgroup finalize over many partials (BERT-base has ~53k): 16-element chunks of one gradient, so that
    its unrolled 16-byte loop (> 4096 groups of four), the plain loop and the n % 4 tail all run. fp64 sum of fp32
    partials of <= 16 squares each: 1e-5 relative holds with room."""
    from mifx.ops.adamw import clip_coef_

    g = (torch.randn(nblocks * 16 - 5, generator=torch.Generator().manual_seed(nblocks)) * 0.1).bfloat16()
    gd = g.cuda()
    gptr = torch.tensor([gd.data_ptr()], dtype=torch.int64, device="cuda")
    bp = torch.zeros(nblocks, dtype=torch.int32, device="cuda")
    bo = torch.arange(nblocks, dtype=torch.int32, device="cuda") * 16
    bn = torch.full((nblocks,), 16, dtype=torch.int32, device="cuda")
    bn[-1] = 11
    partial = torch.full((nblocks,), float("nan"), device="cuda")
    clips = [torch.zeros(2, device="cuda") for _ in range(2)]
    for c in clips:
        clip_coef_(gptr, bp, bo, bn, partial, 2.0, c)
    want = float(g.double().pow(2).sum().sqrt())
    coef, norm = clips[0].tolist()
    print(f"nblocks {nblocks}: norm {norm!r} fp64 {want!r} rel {abs(norm - want) / want:.3e}")
    assert abs(norm - want) <= 1e-5 * want
    assert coef == pytest.approx(min(1.0, 2.0 / (want + 1e-6)), rel=1e-5)
    assert torch.equal(clips[0], clips[1])


@pytest.mark.gpu
@pytest.mark.parametrize("active", [True, False], ids=["clipping", "not_clipping"])
def test_gpu_recipe_matches_cpu_reference(active):
    """G2."""
    steps = [_edge_grads(100 + i) for i in range(6)]
    max_norm = _norm64(steps[0]) * (0.5 if active else 1e3)
    kw = dict(lr=1e-3, weight_decay=0.01, max_grad_norm=max_norm, schedule=("linear", 2, 5), no_decay=_no_decay)
    pc, pg = _edge_params("cpu"), _edge_params("cuda")
    oc, og = FlatAdamW(pc, **kw), FlatAdamW(pg, **kw)
    assert oc.mode == "views" and og.mode == "own"
    untouched, start = pg[NOGRAD].detach().clone(), og.master.clone()
    for i, grads in enumerate(steps):
        _assign(pc, grads, "cpu")
        _assign(pg, grads, "cuda")
        oc.step()
        og.step()
        assert og.last_lr() == oc.last_lr() == scheduled_lr(1e-3, ("linear", 2, 5), i)
        assert og.last_grad_norm() == pytest.approx(oc.last_grad_norm(), rel=1e-5)
        assert (float(og.clip[0]) < 1.0) == active
    assert og.last_lr() == 0.0 and int(og.step_count) == 6
    for i, (c, g) in enumerate(zip(pc, pg)):
        oo, og_o, k = oc._offs[i], og._offs[i], c.numel()
        for name in ("master", "m", "v"):
            torch.testing.assert_close(getattr(og, name)[og_o:og_o + k].cpu(), getattr(oc, name)[oo:oo + k], **TOL,
                                       msg=lambda s, i=i, name=name: f"param {i} {name}: {s}")
    assert torch.equal(og.flat, og.master.bfloat16())
    assert torch.equal(pg[NOGRAD].detach(), untouched)
    moved = og.master != start
    assert all(bool(moved[o:o + p.numel()].all()) == (i != NOGRAD) for i, (o, p) in enumerate(zip(og._offs, pg)))


def _wide_mlp(extra=False):
    torch.manual_seed(1)
    layers = [torch.nn.Linear(5, 7), torch.nn.GELU(), torch.nn.Linear(7, 20000), torch.nn.Linear(20000, 3)]
    if extra:
        layers.append(torch.nn.Linear(3, 9))
    return torch.nn.Sequential(*layers).cuda().bfloat16()


@pytest.mark.gpu
def test_gpu_neutral_options_change_nothing():
    """G3: the extended kernel with neutral arguments against the plain one, bit for bit."""
    ma, mb = _wide_mlp(), _wide_mlp()
    oa = FlatAdamW(list(ma.parameters()), lr=1e-3, weight_decay=0.01, grads="own")
    ob = FlatAdamW(list(mb.parameters()), lr=1e-3, weight_decay=0.01, grads="own", max_grad_norm=1e30, schedule=None,
                   no_decay=lambda p: False)
    assert ob.recipe and not oa.recipe
    x = torch.randn(64, 5, device="cuda", dtype=torch.bfloat16, generator=torch.Generator("cuda").manual_seed(2))
    for _ in range(4):
        for m, o in ((ma, oa), (mb, ob)):
            o.zero_grad()
            m(x).float().pow(2).mean().backward()
            o.step()
    torch.cuda.synchronize()
    assert float(ob.clip[0]) == 1.0 and ob.last_grad_norm() > 0
    for name in ("flat", "master", "m", "v"):
        assert torch.equal(getattr(oa, name), getattr(ob, name)), name


@pytest.mark.gpu
def test_gpu_captured_recipe_step_equals_eager():
    """G4: lr_t and the clip coefficient are computed on the device on every replay."""
    x = torch.randn(64, 5, device="cuda", dtype=torch.bfloat16, generator=torch.Generator("cuda").manual_seed(2))
    out = []
    for captured in (False, True):
        m = _wide_mlp(extra=True)
        o = FlatAdamW(list(m.parameters()), lr=1e-3, weight_decay=0.01, grads="own", max_grad_norm=1e-4,
                      schedule=("linear", 2, 5), no_decay=_no_decay)

        def step():
            o.zero_grad()
            m(x).float().pow(2).mean().backward()
            o.step()

        if not captured:
            for _ in range(8):
                step()
        else:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    step()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            o.zero_grad()
            o.begin_capture()
            with torch.cuda.graph(g):
                step()
            for _ in range(6):
                g.replay()
        torch.cuda.synchronize()
        assert int(o.step_count) == 8
        assert o.last_grad_norm() > 1e-4 and float(o.clip[0]) < 1.0  # the clipping is active
        assert o.last_lr() == 0.0
        out.append(o)
    for name in ("flat", "master", "m", "v", "clip"):
        assert torch.equal(getattr(out[0], name), getattr(out[1], name)), name
    assert not torch.equal(out[0].m, torch.zeros_like(out[0].m))


@pytest.mark.gpu
def test_gpu_bert_trainer_recipe_captured_equals_eager():
    """G5: BertTrainer with all three options, hipGraph against graph=False, bitwise; the no-decay set matters."""
    from mifx.models.bert import BertConfig
    from mifx.trainer.bert_trainer import BertTrainer

    cfg = BertConfig(layers=2, dropout=0.0)
    kw = dict(lr=1e-3, max_grad_norm=1.0, warmup_steps=2, total_steps=10)
    eager = BertTrainer(cfg, 8, 64, "cuda", graph=False, no_decay_bias_norm=True, **kw)
    graphed = BertTrainer(cfg, 8, 64, "cuda", graph=True, no_decay_bias_norm=True, **kw)
    decayed = BertTrainer(cfg, 8, 64, "cuda", graph=False, no_decay_bias_norm=False, **kw)
    assert eager.flat and graphed.flat and graphed.use_graph and eager.opt.recipe
    le = [float(eager.step()) for _ in range(8)]
    lg = [float(graphed.step()) for _ in range(5)]  # capture runs 3 eager warmup steps first
    for _ in range(8):
        decayed.step()
    assert graphed.graph is not None
    assert lg == le[3:]
    assert torch.equal(graphed.opt.flat, eager.opt.flat) and torch.equal(graphed.opt.master, eager.opt.master)
    assert int(graphed.opt.step_count) == int(eager.opt.step_count) == 8
    want_lr = scheduled_lr(1e-3, ("linear", 2, 10), 7)
    assert want_lr == pytest.approx(1e-3 * 3 / 8, rel=1e-6)

    def master_of(tr, i):
        return tr.opt.master[tr.opt._offs[i]:tr.opt._offs[i] + tr.opt.params[i].numel()]

    small = [i for i, p in enumerate(eager.opt.params) if p.ndim <= 1]
    differ = [i for i in small if not torch.equal(master_of(eager, i), master_of(decayed, i))]
    assert (len(differ) > 0 and eager.last_lr() == graphed.last_lr() == decayed.last_lr() == want_lr
            and graphed.last_grad_norm() == eager.last_grad_norm() and eager.last_grad_norm() > 0), \
        (len(differ), len(small), eager.last_lr(), graphed.last_lr(), decayed.last_lr(), want_lr)
