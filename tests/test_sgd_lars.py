"""ResNet large-batch recipe: LARS trust ratios and the in-graph learning-rate schedule of the fused SGD
(csrc/sgd.hip: sqnorm2_chunks, lars_finalize, sgd_chunks_ex; mifx.ops.sgd), label smoothing, and their wiring
through ResNetTrainer and the ImageTrainer component.

The fp64 reference of the GPU tests is `_formula_step` below, the recipe's formulas written out element by element;
`lars_reference_` (stock torch ops) is checked against it on the CPU."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(__file__))
VARIANTS = [(True, 0.0), (False, 0.0), (False, 0.1)]  # (nesterov, dampening)
CHUNK = 2048  # elements per workgroup of csrc/sgd.hip (mifx_sgd_chunk_size)


# ------------------------------------------------------------------------------------------------ fp64 reference
def _formula_step(w, g, buf, wd, a, eta, eps, clip, mom, damp, nest, lr, mutate=None, first_chunk=0, ntensors=0,
                  all_ratios=None):
    """One tensor's update in fp64, in place; returns (ratio, wn, gn, max |g'|). `mutate` plants one of the bugs of
    test_inputs_tell_the_mutations_apart into the reference."""
    wn, gn = math.sqrt(float((w * w).sum())), math.sqrt(float((g * g).sum()))
    r = 1.0
    if a and wn != 0 and gn != 0:
        den = gn + (0.0 if mutate == "no_wd" else wd * wn) + (0.0 if mutate == "no_eps" else eps)
        r = eta * wn / den
        if clip:
            r = min(r / lr, 1.0) if lr != 0 else 1.0
    gp = (g + wd * w) * r
    if mutate == "chunk_index":  # the update reads ratio[chunk] instead of ratio[tensor]
        flat = (g + wd * w).reshape(-1).clone()
        for c, o in enumerate(range(0, flat.numel(), CHUNK)):
            flat[o:o + CHUNK] *= all_ratios[min(first_chunk + c, ntensors - 1)]
        gp = flat.reshape(g.shape)
    buf.mul_(mom).add_(gp, alpha=1 - damp)
    u = gp + mom * buf if nest else buf
    w.sub_(lr * u)
    return r, wn, gn, float(gp.abs().max()) if gp.numel() else 0.0


def _reference_run(case, steps, schedule, eta, eps, clip, mom, damp, nest, mutate=None, t0=0):
    """fp64 run of `steps` updates over the tensors of `case` (flattened); returns weights, buffers, the per-step
    ratios / norms / learning rates and R = the largest |r (g + wd w)| met."""
    from mifx.ops.sgd import scheduled_lr

    w = [t.double().reshape(-1).clone() for t in case["w"]]
    g = [t.double().reshape(-1).clone() for t in case["g"]]
    b = [t.double().reshape(-1).clone() for t in case["b"]]
    kind, base, warmup, total, end = schedule
    out = {"ratios": [], "norms": [], "lrs": [], "R": 0.0}
    for s in range(steps):
        t = t0 + s
        lr = scheduled_lr(kind, base, warmup, total, end, t + 1 if mutate == "t_plus_1" and t >= warmup else t)
        lr32 = float(np.float32(lr))  # the kernel rounds the schedule to fp32 once
        ratios = None
        if mutate == "chunk_index":  # (the finalize is right, the update's index is not)
            ratios = [_formula_step(w[i].clone(), g[i], b[i].clone(), case["wd"][i], case["adapt"][i], eta, eps,
                                    clip, mom, damp, nest, lr32)[0] for i in range(len(w))]
        rs, ns, first = [], [], 0
        for i in range(len(w)):
            r, wn, gn, m = _formula_step(w[i], g[i], b[i], case["wd"][i], case["adapt"][i], eta, eps, clip, mom, damp,
                                         nest, lr32, mutate, first, len(w), ratios)
            first += (w[i].numel() + CHUNK - 1) // CHUNK
            rs.append(r)
            ns.append((wn, gn))
            out["R"] = max(out["R"], m)
        out["ratios"].append(torch.tensor(rs, dtype=torch.float64))
        out["norms"].append(torch.tensor(ns, dtype=torch.float64))
        out["lrs"].append(lr32)
    out["w"], out["b"] = w, b
    return out


SIZES = [7, 64, 1000, 2048, 2048 * 3 + 5, 4096 + 3, 2048 * 1200 + 3]
ETA, EPS = 0.001, 1e-8


def _case(largest=True):
    """The tensors of G1 / G2 (fp32, CPU). Adapt flags alternate from True. Scales (powers of ten) per tensor:
    0 adapted, all-zero g; 1 plain; 2 adapted, all-zero w; 3 plain, channels_last 4-D; 4 adapted, four chunks, wd 0,
    tiny g so that eps carries 11 % of the denominator (ratio ~ 9e5); 5 plain; 6 adapted, 1201 chunks, wd |w| equal
    to |g| in the denominator (ratio ~ 0.05). The adapted ratios (1, 1, ~9e5, ~0.05) differ pairwise by more than
    2x; |g'| <= 2 eta |w| for an adapted tensor and |g| + wd |w| otherwise keep R below 0.25."""
    gen = torch.Generator().manual_seed(1234)
    wscale = [1.0, 1.0, 0.0, 1.0, 1.0, 0.1, 0.01]
    gscale = [0.0, 0.01, 0.01, 0.01, 1e-9, 0.01, 1e-4]
    wds = [1e-4, 0.0, 1e-4, 1e-4, 0.0, 1e-4, 1e-2]
    n = len(SIZES) if largest else len(SIZES) - 1
    shape = lambda i: (32, 16, 2, 2) if i == 3 else (SIZES[i],)  # noqa: E731
    mk = lambda i, s: torch.randn(shape(i), generator=gen) * s  # noqa: E731
    case = {"w": [mk(i, wscale[i]) for i in range(n)], "g": [mk(i, gscale[i]) for i in range(n)],
            "b": [mk(i, 0.01) for i in range(n)], "wd": wds[:n], "adapt": [i % 2 == 0 for i in range(n)]}
    for k in "wgb":
        case[k][3] = case[k][3].contiguous(memory_format=torch.channels_last)
    return case


@pytest.fixture(scope="module")
def g1_case():
    return _case(True)


@pytest.fixture(scope="module")
def g2_case():
    return _case(False)


G2_SCHEDULE = ("cosine", 0.1, 1, 6, 0.001)


@pytest.fixture(scope="module")
def g2_refs(g2_case):
    """The fp64 reference of G2, computed once per (nesterov, dampening)."""
    return {v: _reference_run(g2_case, 3, G2_SCHEDULE, ETA, EPS, False, 0.9, v[1], v[0]) for v in VARIANTS}


def _g2_atol(R):
    return 3 * (1e-6 + 4e-6 * R)


# ------------------------------------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("nesterov,damp", VARIANTS)
def test_lars_reference_matches_formulas_fp64(nesterov, damp, clip):
    """C1: lars_reference_ (torch.linalg.vector_norm + sgd_reference_) against the formulas, three steps."""
    from mifx.ops.sgd import lars_reference_

    gen = torch.Generator().manual_seed(7)
    shapes = [(5, 3), (11,), (4, 2, 3, 3), (9,), (6, 6), (13,)]
    adapt = [True, False, True, True, True, True]
    wds = [1e-2, 0.0, 5e-3, 0.0, 1e-2, 1e-2]
    w = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    g = [torch.randn(s, generator=gen, dtype=torch.float64) * 0.1 for s in shapes]
    b = [torch.randn(s, generator=gen, dtype=torch.float64) * 0.1 for s in shapes]
    w[4].zero_()  # adapted, all-zero w
    g[5].zero_()  # adapted, all-zero g
    w2, b2 = [t.clone() for t in w], [t.clone() for t in b]
    for step in range(3):
        lr = 0.05 * (step + 1)
        got = lars_reference_(w, g, b, wds, adapt, 0.02, 1e-8, clip, 0.9, damp, nesterov, lr)
        want = [_formula_step(w2[i], g[i], b2[i], wds[i], adapt[i], 0.02, 1e-8, clip, 0.9, damp, nesterov, lr)[0]
                for i in range(len(w))]
        torch.testing.assert_close(torch.stack(got), torch.tensor(want, dtype=torch.float64), rtol=1e-13, atol=0)
        assert float(got[1]) == 1.0 and float(got[5]) == 1.0  # not adapted / zero g: exactly 1
        if step == 0:
            assert float(got[4]) == 1.0  # zero w (the first update moves it off zero)
    for a, c in zip(w + b, w2 + b2):
        torch.testing.assert_close(a, c, rtol=1e-12, atol=1e-15)


def test_lars_reference_step_length_fp64():
    """C1: one adapted tensor, wd = 0, no momentum, eps = 0: the step has length lr * eta * ||w||."""
    from mifx.ops.sgd import lars_reference_

    gen = torch.Generator().manual_seed(8)
    w = torch.randn(37, 5, generator=gen, dtype=torch.float64)
    g = torch.randn(37, 5, generator=gen, dtype=torch.float64) * 3
    w0 = w.clone()
    lars_reference_([w], [g], [torch.zeros_like(w)], [0.0], [True], 0.01, 0.0, False, 0.0, 0.0, False, 0.3)
    torch.testing.assert_close((w - w0).norm(), 0.3 * 0.01 * w0.norm(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("nesterov,damp", VARIANTS)
def test_lars_reference_ratio_one_is_torch_sgd(nesterov, damp):
    """C1: tensors that are not adapted, all-zero w, or all-zero g take ratio exactly 1 and follow torch.optim.SGD
    (its momentum buffers pre-seeded with zeros, so the first step applies the dampening as later ones do)."""
    from mifx.ops.sgd import lars_reference_

    gen = torch.Generator().manual_seed(9)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    w = [mk(6, 4), torch.zeros(5, 5, dtype=torch.float64), mk(8, 3)]
    g = [mk(6, 4), mk(5, 5), torch.zeros(8, 3, dtype=torch.float64)]
    adapt, wds = [False, True, True], [1e-2, 1e-3, 1e-2]
    b = [torch.zeros_like(t) for t in w]
    ps = [torch.nn.Parameter(t.clone()) for t in w]
    opt = torch.optim.SGD([{"params": [p], "weight_decay": wd} for p, wd in zip(ps, wds)], lr=0.1, momentum=0.9,
                          dampening=damp, nesterov=nesterov)
    for p, gi in zip(ps, g):
        p.grad = gi.clone()
        opt.state[p]["momentum_buffer"] = torch.zeros_like(p)
    opt.step()
    r = lars_reference_(w, g, b, wds, adapt, 0.001, 1e-8, False, 0.9, damp, nesterov, 0.1)
    assert [float(x) for x in r] == [1.0, 1.0, 1.0]
    for a, p in zip(w, ps):
        torch.testing.assert_close(a, p.detach(), rtol=1e-13, atol=1e-16)
    for a, p in zip(b, ps):
        torch.testing.assert_close(a, opt.state[p]["momentum_buffer"], rtol=1e-13, atol=1e-16)


def test_scheduled_lr():
    """C2."""
    from mifx.ops.sgd import scheduled_lr

    base, warmup, total, end = 0.4, 5, 17, 0.003
    for t in range(total + 4):
        assert scheduled_lr("constant", base, warmup, None, 0.0, t) == base * min(1.0, (t + 1) / max(1, warmup))
        assert scheduled_lr("constant", base, 0, None, 0.0, t) == base
    for kind in ("cosine", "poly"):
        lrs = [scheduled_lr(kind, base, warmup, total, end, t) for t in range(total + 4)]
        for t in range(warmup):
            assert lrs[t] == base * min(1.0, (t + 1) / warmup)
        assert lrs[warmup - 1] == base and lrs[warmup] == base
        assert all(v == end for v in lrs[total:])
        assert all(lrs[t + 1] <= lrs[t] for t in range(warmup, total + 3))
        assert lrs[total - 1] > end
    mid = warmup + (total - warmup) // 2
    assert scheduled_lr("cosine", base, warmup, total, end, mid) == pytest.approx(end + (base - end) * 0.5, rel=1e-12)
    assert scheduled_lr("poly", base, warmup, total, end, mid) == pytest.approx(end + (base - end) * 0.25, rel=1e-12)
    for bad in (("linear", 0.1, 1, 5, 0.0, 0), ("cosine", 0.1, 5, 5, 0.0, 0), ("poly", 0.1, 6, 5, 0.0, 9),
                ("cosine", 0.1, 5, None, 0.0, 0), ("constant", -0.1, 1, None, 0.0, 0), ("cosine", 0.1, 1, 5, -1.0, 0),
                ("poly", 0.1, -1, 5, 0.0, 0), ("constant", 0.1, 1, None, 0.0, -1)):
        with pytest.raises(ValueError):
            scheduled_lr(*bad)


def _toy_trainer(**kw):
    from mifx.trainer.resnet_trainer import ResNetTrainer, synthetic_imagenet

    imgs, labels = synthetic_imagenet(40, 40, 5, seed=3)
    return ResNetTrainer(4, "cpu", imgs, labels, num_classes=5, warmup_steps=2, crop=32, **kw)


def test_trainer_recipe_resume_equals_uninterrupted(tmp_path):
    """C3: LARS + cosine + label smoothing on the CPU path; 2 steps, checkpoint, restore, 2 more == 4 straight."""
    from mifx.ops.sgd import scheduled_lr

    kw = dict(lars=True, lr_schedule="cosine", total_steps=4, label_smoothing=0.1)

    def run(tr, n):
        for _ in range(n):
            t = tr.step_idx
            tr.step()
            assert tr.last_lr() == scheduled_lr("cosine", 0.1, 2, 4, 0.0, t)
            r = tr.last_trust_ratios()
            assert r.shape == (len(list(tr.model.parameters())),)
            for p, ri in zip(tr.model.parameters(), r):
                assert p.ndim > 1 or float(ri) == 1.0

    a = _toy_trainer(**kw)
    run(a, 4)
    assert a.last_lr() < 0.1 and (a.last_trust_ratios() != 1).any()
    b = _toy_trainer(**kw)
    run(b, 2)
    path = b.save_checkpoint(str(tmp_path / "ck"))
    c = _toy_trainer(**kw)
    c.restore(path)
    assert c.step_idx == 2
    run(c, 2)
    sa, sc = a.state_dict(), c.state_dict()
    assert set(sa) == set(sc) and any(k.startswith("opt.momentum") for k in sa)
    for k in sa:
        torch.testing.assert_close(sc[k], sa[k], rtol=0, atol=0, msg=k)


def test_trainer_recipe_changes_the_update_and_validates():
    """Each option moves the weights away from the default run's; invalid combinations are refused."""
    base = _toy_trainer()
    base.step()
    ref = torch.cat([p.detach().reshape(-1) for p in base.model.parameters()])
    for kw in (dict(lars=True), dict(label_smoothing=0.1)):
        tr = _toy_trainer(**kw)
        tr.step()
        assert not torch.equal(torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]), ref), kw
    for bad in (dict(lr_schedule="step"), dict(lr_schedule="cosine"), dict(lr_schedule="cosine", total_steps=2),
                dict(total_steps=5), dict(end_lr=0.01), dict(lars_clip=True), dict(lars_eta=0.01),
                dict(lars=True, lars_eta=0.0), dict(label_smoothing=1.0), dict(label_smoothing=-0.1)):
        with pytest.raises(ValueError):
            _toy_trainer(**bad)


def test_trainer_default_construction():
    """C5."""
    tr = _toy_trainer()
    assert tr.last_trust_ratios() is None and tr.last_lr() is None
    assert tr.lr_schedule == "constant" and tr.lars is None and tr.label_smoothing == 0.0
    tr.step()
    assert tr.last_trust_ratios() is None and tr.last_lr() == 0.1 * 0.5


def _run_component(tmp_path, name, num_gpus, batch, accum, optimizer, steps=3):
    from safetensors.torch import load_file

    from mifx.orchestration import LocalDagRunner

    spec = importlib.util.spec_from_file_location("rp", os.path.join(ROOT, "examples/image/resnet_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.create_pipeline(str(tmp_path / name), 48, 40, 32, 5, steps, batch, num_gpus, 0, accum, name=name,
                            optimizer=optimizer)
    res = LocalDagRunner(device="cpu").run(p)
    assert res.succeeded
    out = res.components["ImageTrainer"].outputs["output"][0]
    md = os.path.join(out.uri, "serving_model_dir")
    with open(os.path.join(out.uri, "metrics.json")) as f:
        metrics = json.load(f)
    return out, load_file(os.path.join(md, f"ckpt-{steps}.safetensors")), metrics


def test_component_recipe_dp_two_ranks_equal_one_process_accumulating(tmp_path):
    """C4: two gloo ranks at accum 1 == one process at accum 2 with LARS + cosine (the norms are taken on the
    averaged gradients); the component records the resolved recipe."""
    from mifx.ops.sgd import scheduled_lr

    opt = {"lars": True, "lr_schedule": "cosine", "end_lr": 0.001, "label_smoothing": 0.1}
    o1, one, m1 = _run_component(tmp_path, "acc", 1, 4, 2, opt)
    o2, dp, m2 = _run_component(tmp_path, "dp", 2, 4, 1, opt)
    ws = [k for k in one if k.startswith("model.") and "running" not in k and "num_batches" not in k]
    assert len(ws) > 100
    for k in ws:
        np.testing.assert_allclose(dp[k].numpy(), one[k].numpy(), rtol=2e-4, atol=2e-6, err_msg=k)
    want = {"learning_rate": 0.1, "lr_schedule": "cosine", "warmup_steps": 1, "total_steps": 3, "end_lr": 0.001,
            "lars": True, "lars_eta": 0.001, "lars_clip": False, "label_smoothing": 0.1,
            "final_lr": scheduled_lr("cosine", 0.1, 1, 3, 0.001, 2)}
    for out, m, world in ((o1, m1, 1), (o2, m2, 2)):
        assert m["optimizer"] == want and m["world"] == world
        cp = out.custom_properties
        assert cp["num_replicas"] == world and cp["lr_schedule"] == "cosine" and cp["lars"] == 1
        assert cp["total_steps"] == 3 and cp["end_lr"] == 0.001 and cp["label_smoothing"] == 0.1
        assert cp["lars_clip"] == 0 and cp["lars_eta"] == 0.001 and cp["final_lr"] == want["final_lr"]


def test_component_optimizer_config():
    from mifx.components.image import resolve_optimizer_config

    d = resolve_optimizer_config({}, 0.1, 100)
    assert d["lr_schedule"] == "constant" and d["total_steps"] is None and d["warmup_steps"] == 10
    assert d["lars"] is False and d["label_smoothing"] == 0.0 and d["end_lr"] == 0.0
    for bad in ({"lr_schedule": "linear"}, {"end_lr": 0.1}, {"lars_eta": 0.01}, {"lars_clip": True}):
        with pytest.raises(ValueError):
            resolve_optimizer_config(bad, 0.1, 100)


MUTATIONS = ["chunk_index", "no_wd", "no_eps", "t_plus_1"]


@pytest.mark.parametrize("mutate", MUTATIONS)
def test_inputs_tell_the_mutations_apart(mutate, g1_case, g2_case, g2_refs):
    """The inputs and tolerances of G1 / G2 separate each of these bugs, planted into the fp64 reference, from the
    right result: the ratio indexed by chunk instead of by tensor, wd * wn dropped from the denominator, eps
    dropped, t + 1 used after the warmup."""
    good1 = _reference_run(g1_case, 1, ("constant", 0.1, 0, None, 0.0), ETA, EPS, False, 0.9, 0.0, True)
    bad1 = _reference_run(g1_case, 1, ("constant", 0.1, 0, None, 0.0), ETA, EPS, False, 0.9, 0.0, True, mutate)
    g1_fails = not torch.allclose(bad1["ratios"][0], good1["ratios"][0], rtol=4e-6, atol=0)
    good2 = g2_refs[(True, 0.0)]
    bad2 = _reference_run(g2_case, 3, G2_SCHEDULE, ETA, EPS, False, 0.9, 0.0, True, mutate)
    atol = _g2_atol(good2["R"])
    g2_fails = any(not torch.allclose(x, y, rtol=1e-6, atol=atol)
                   for x, y in zip(bad2["w"] + bad2["b"], good2["w"] + good2["b"]))
    assert g1_fails or g2_fails
    assert g1_fails == (mutate in ("no_wd", "no_eps")) and g2_fails == (mutate in ("chunk_index", "no_eps", "t_plus_1"))


# ------------------------------------------------------------------------------------------------ GPU tests
def _tables(case, lars, device="cuda"):
    from mifx.ops.sgd import FusedSGDTables

    w, g, b = ([t.to(device) for t in case[k]] for k in "wgb")
    for ts in (w, g, b):  # (.to keeps channels_last)
        assert ts[3].stride() == case["w"][3].stride()
    return FusedSGDTables(w, b, case["wd"], grads=g, lars=lars), w, g, b


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [False, True])
def test_trust_ratios_and_norms_gpu(clip, g1_case):
    """G1. Bound: each squared norm passes through at most 16 fp32 roundings of a sum of non-negative terms (8
    FMAs, 4 DPP steps, 2 + 2 combines), <= 16 * 2^-24 ~ 9.5e-7 relative; the norms half of that; the quotient of
    two such plus a few fp32 operations <= 1.5e-6; 4e-6 leaves more than 2x."""
    schedule = ("constant", 0.1, 0, None, 0.0)
    ref = _reference_run(g1_case, 1, schedule, ETA, EPS, clip, 0.9, 0.0, True)
    tab, w, g, b = _tables(g1_case, dict(eta=ETA, eps=EPS, clip=clip, adapt=g1_case["adapt"]))
    assert tab.last_lr() is None and tab.last_trust_ratios() is None and tab.last_norms() is None
    assert tab.nblocks > 1024 + 12
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab.step_ex(step, schedule, 0.9, 0.0, True)
    r, n = tab.last_trust_ratios().double(), tab.last_norms().double()
    print("ratios", r.tolist(), "\nreference", ref["ratios"][0].tolist(),
          "\nrel err", ((r - ref["ratios"][0]) / ref["ratios"][0]).abs().tolist(),
          "\nnorm rel err", ((n - ref["norms"][0]) / ref["norms"][0].clamp_min(1e-30)).abs().tolist())
    torch.testing.assert_close(r, ref["ratios"][0], rtol=4e-6, atol=0)
    torch.testing.assert_close(n, ref["norms"][0], rtol=4e-6, atol=0)
    for i in (0, 1, 2, 3, 5):  # zero g, zero w and the tensors that are not adapted: exactly 1
        assert float(r[i]) == 1.0
    assert float(n[0, 1]) == 0.0 and float(n[2, 0]) == 0.0
    if not clip:  # the ratios met (1, tensor 4's, tensor 6's) differ pairwise by 2x or more: a wrong index shows
        lo, mid, hi = sorted([1.0, float(r[4]), float(r[6])])
        assert mid >= 2 * lo and hi >= 2 * mid
    else:
        assert float(r[4]) == 1.0 and float(r[6]) < 1.0  # LARC: min(ratio / lr, 1)
    assert tab.last_lr() == float(np.float32(0.1))


@pytest.mark.gpu
@pytest.mark.parametrize("nesterov,damp", VARIANTS)
def test_step_ex_matches_fp64_reference_gpu(nesterov, damp, g2_case, g2_refs):
    """G2. rtol 1e-6 and atol 3 * (1e-6 + 4e-6 R): 1e-6 / 1e-6 is the plain kernel's tolerance
    (tests/test_sgd_fused.py), the second term carries G1's ratio bound through three steps; R = the largest
    |r (g + wd w)| the reference meets (asserted <= 0.25)."""
    ref = g2_refs[(nesterov, damp)]
    assert ref["R"] <= 0.25
    tab, w, g, b = _tables(g2_case, dict(eta=ETA, eps=EPS, clip=False, adapt=g2_case["adapt"]))
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    for t in range(3):
        step.fill_(t)
        tab.step_ex(step, G2_SCHEDULE, 0.9, damp, nesterov)
        assert tab.last_lr() == pytest.approx(ref["lrs"][t], rel=2.0 ** -23)
        torch.testing.assert_close(tab.last_trust_ratios().double(), ref["ratios"][t], rtol=4e-6, atol=0)
    atol = _g2_atol(ref["R"])
    err = max(float((a.cpu().double().reshape(-1) - c).abs().max()) for a, c in zip(w + b, ref["w"] + ref["b"]))
    print(f"R = {ref['R']:.4g}, atol = {atol:.3g}, largest |error| = {err:.3g}")
    for a, c in zip(w + b, ref["w"] + ref["b"]):
        torch.testing.assert_close(a.cpu().double().reshape(-1), c, rtol=1e-6, atol=atol)
    assert all(torch.equal(x.cpu(), y) for x, y in zip(g, g2_case["g"]))  # gradients are read only


@pytest.mark.gpu
@pytest.mark.parametrize("nesterov,damp", VARIANTS)
def test_step_ex_neutral_is_bitwise_step_gpu(nesterov, damp):
    """G3: every adapt flag off + the constant schedule == `step` with a host-filled -lr, bit for bit."""
    from mifx.ops.sgd import FusedSGDTables, scheduled_lr

    torch.manual_seed(4)
    sizes = [7, 1001, 2048 + 3, 2048 * 2 + 1, 4099]
    wds = [1e-4 if i % 2 else 0.0 for i in range(len(sizes))]
    mk = lambda: [torch.randn(n, device="cuda") for n in sizes]  # noqa: E731
    p, g, b = mk(), mk(), mk()
    p2, b2 = [t.clone() for t in p], [t.clone() for t in b]
    schedule = ("constant", 0.05, 2, None, 0.0)
    ex = FusedSGDTables(p, b, wds, grads=g, lars=dict(adapt=[False] * len(sizes)))
    plain = FusedSGDTables(p2, b2, wds, grads=g)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    neg_lr = torch.zeros((), device="cuda")
    for t in range(3):
        step.fill_(t)
        ex.step_ex(step, schedule, 0.9, damp, nesterov)
        neg_lr.fill_(-scheduled_lr(*schedule, t))
        plain.step(neg_lr, 0.9, damp, nesterov)
        assert ex.last_lr() == -float(neg_lr)
        assert torch.equal(ex.last_trust_ratios(), torch.ones(len(sizes)))
    for a, c in zip(p + b, p2 + b2):
        assert torch.equal(a, c)


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["cosine", "constant"])
def test_step_ex_captured_follows_device_step_gpu(kind):
    """G4: one capture of set_grads + step_ex, replayed with the device step at 0..5, equals six eager calls bit for
    bit; the learning rate read back follows scheduled_lr (cosine: within one fp32 ulp, the double cos may differ in
    its last bit before the one rounding to fp32; constant: the same bits)."""
    from mifx.ops.sgd import FusedSGDTables, scheduled_lr

    schedule = (kind, 0.2, 2, 5 if kind == "cosine" else None, 0.01 if kind == "cosine" else 0.0)
    torch.manual_seed(5)
    shapes = [(3000,), (64, 33), (17,)]
    mk = lambda s: [torch.randn(x, device="cuda") * s for x in shapes]  # noqa: E731
    p, g, b = mk(1.0), mk(0.1), mk(0.0)
    p2, b2 = [t.clone() for t in p], [t.clone() for t in b]
    wds = [1e-4, 1e-4, 0.0]
    lars = dict(eta=0.005, clip=True)
    cap, eager = FusedSGDTables(p, b, wds, lars=lars), FusedSGDTables(p2, b2, wds, grads=g, lars=lars)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cap.set_grads(g)
            cap.step_ex(step, schedule, 0.9, 0.0, True)
    torch.cuda.current_stream().wait_stream(s)
    for t in range(6):
        step.fill_(t)
        graph.replay()
        want = float(np.float32(scheduled_lr(*schedule, t)))
        got = cap.last_lr()
        if kind == "constant":
            assert got == want
        else:
            assert abs(got - want) <= _ulp32(want), (t, got, want)
        r_cap = cap.last_trust_ratios()
        eager.step_ex(step, schedule, 0.9, 0.0, True)
        assert eager.last_lr() == got and torch.equal(eager.last_trust_ratios(), r_cap)
        assert float(r_cap[0]) == 1.0 and float(r_cap[2]) == 1.0  # 1-D tensors are not adapted by default
        assert t != 1 or 0.0 < float(r_cap[1]) < 1.0  # (at the top of the schedule the clip does not bind)
    torch.cuda.synchronize()
    for a, c in zip(p + b, p2 + b2):
        assert torch.equal(a, c)
    if kind == "cosine":
        assert cap.last_lr() == float(np.float32(0.01))  # t >= total: the end value


@pytest.mark.gpu
def test_trainer_recipe_wiring_gpu():
    """G5: LARS + poly + label smoothing through ResNetTrainer: two eager steps, then the captured step takes the
    learning rate and the ratios from the device. The ratios of one captured step are recomputed in fp64 from the
    weights before it and the gradients after it, with the trainer's weight-decay groups and the ndim rule."""
    from mifx.ops.sgd import scheduled_lr
    from mifx.trainer.resnet_trainer import ResNetTrainer, synthetic_imagenet

    imgs, labels = synthetic_imagenet(48, 72, 10, device="cuda")
    tr = ResNetTrainer(6, "cuda", imgs, labels, num_classes=10, crop=64, warmup_steps=2, lars=True, lr_schedule="poly",
                       total_steps=6, label_smoothing=0.1)
    params = list(tr.model.parameters())
    losses = []
    for t in range(5):
        before = [p.detach().clone() for p in params] if t == 3 else None
        losses.append(float(tr.step()))
        want = float(np.float32(scheduled_lr("poly", 0.1, 2, 6, 0.0, t)))
        assert abs(tr.last_lr() - want) <= _ulp32(want), (t, tr.last_lr(), want)
        assert (tr._gA is not None) == (t >= 2) and tr._lr_on_device == (t >= 2)
        if before is not None:
            got = tr.last_trust_ratios().double()
            want_r = []
            for w, p in zip(before, params):
                wd = 5e-5 if p.ndim > 1 else 0.0
                wn, gn = float(w.double().norm()), float(p.grad.double().norm())
                want_r.append(1e-3 * wn / (gn + wd * wn + 1e-8) if p.ndim > 1 and wn != 0 and gn != 0 else 1.0)
            want_r = torch.tensor(want_r, dtype=torch.float64)
            print("largest ratio error", float(((got - want_r) / want_r).abs().max()))
            torch.testing.assert_close(got, want_r, rtol=4e-6, atol=0)
            assert (got != 1).sum() == sum(p.ndim > 1 for p in params)
    assert all(np.isfinite(losses))
    assert tr._sgd_tab is not None
