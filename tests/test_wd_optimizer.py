"""The Wide&Deep slab reduction + optimizer kernels (csrc/wide_deep.hip, update math in csrc/wd_opt.h) against an
fp64 reference written from the TF / Adam definitions.

Inputs: slab entries are k * 2**-8 with integer |k| <= 1024 over at most 300 rows, so every partial sum is exact in
fp32 in any order. All reduction variants must therefore give BIT-identical results, and the comparison with the
reference measures only the optimizer arithmetic. Tolerance per (config, step, tensor): E = max error of the same
update evaluated in float32 numpy against the fp64 reference; the GPU may be off by 8 * E + 2 float32 ulps of the
tensor's maximum magnitude (device rsqrtf / powf / sqrtf are allowed a few ulp where numpy rounds correctly)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mifx.models import wide_deep as wdm
from mifx.trainer.fused_wide_deep import OptSpec

STEPS = 3
STEP_MULT = (2, 1, 4)  # power of two the base slab is multiplied by on each step (entries stay k * 2**-8, |k| <= 1024)
STEP_SLOTS = 512       # csrc/wd_opt.h

# Row counts at the loop edges of the reductions: slab_column_sum sums RU * RG = 8 * 16 = 128 rows per main iteration
# (row group r runs it while r + 112 < G); wd_reduce_res / wd_reduce_res_fused 8 residues x 4 waves x U = 8 = 256
# rows per round; wd_reduce / wd_optimizer unroll rows / partials by 4; G == 1 is its own kernel (wd_opt1_sc).
G_ALL = (1, 2, 7, 8, 9, 33, 127, 128, 129, 256, 300)
XCD_MAX_G = 256  # mifx_wd_reduce_xcd_opt rejects more rows
# Strides at the column edges: 64 columns per wd_reduce_opt_sc workgroup, 256 per level-1 chunk, level-2 workgroup
# and wd_opt1_sc workgroup; plus the chained trainer's own stride.
SMALL_STRIDE = 68
MODEL_STRIDE = int(wdm.chain_maps()[1])
STRIDES = (4, 68, 256, 260, 1028, MODEL_STRIDE)
G_PER_STRIDE = (1, 9, 129)
PAIRS = tuple(dict.fromkeys([(g, SMALL_STRIDE) for g in G_ALL] + [(g, MODEL_STRIDE) for g in G_ALL]
                            + [(g, s) for s in STRIDES for g in G_PER_STRIDE]))

# l1 = 1.5 against summed gradients of standard deviation ~1.5-3: see test_ftrl_l1_splits_the_reference_columns
_FTRL_REG = dict(l1=1.5, l2=0.5)
CONFIGS = {  # name -> (DNN spec, wide spec, preset of every step slot)
    "default": (OptSpec("adagrad", lr=0.05), OptSpec("ftrl", lr=0.2), 0),
    "ftrl_l1l2": (OptSpec("adagrad", lr=0.05), OptSpec("ftrl", lr=0.2, lr_power=-0.5, **_FTRL_REG), 0),
    "ftrl_pow075": (OptSpec("adagrad", lr=0.05), OptSpec("ftrl", lr=0.2, lr_power=-0.75, **_FTRL_REG), 0),
    "swapped": (OptSpec("ftrl", lr=0.2, lr_power=-0.75, **_FTRL_REG), OptSpec("adagrad", lr=0.05), 0),
    "adam_step0": (OptSpec("adam", lr=3e-3), OptSpec("adam", lr=1e-2), 0),
    "adam_step999": (OptSpec("adam", lr=3e-3), OptSpec("adam", lr=1e-2), 999),
    "sgd": (OptSpec("sgd", lr=1e-3), OptSpec("sgd", lr=4e-3), 0),
}

SENTINEL = (np.float32(7.25), np.float32(-3.5), np.float32(11.0))  # param / s0 / s1 of columns nothing may touch
WT_SENTINEL = 0x5A5A  # bf16 image entries nothing may write


# ------------------------------------------------------------------------------------------------ reference
def ref_update(kind, w, g, a0, a1, step, hyper, dtype=np.float64):
    """One optimizer step on arrays, every operation in `dtype` (fp64: the reference; fp32: the emulation whose
    error defines the tolerance). hyper: the 8 float32 values of OptSpec.encode(), widened. Returns (w, a0, a1).

    sgd      ApplyGradientDescent: var -= lr * grad
    adagrad  ApplyAdagrad (no epsilon): accum += grad^2; var -= lr * grad / sqrt(accum)                [a0 = accum]
    ftrl     ApplyFtrl: accum_new = accum + grad^2; p = -lr_power (sqrt for lr_power == -0.5)
             linear += grad - (accum_new^p - accum^p) / lr * var; quadratic = accum_new^p / lr + 2 * l2
             var = |linear| > l1 ? (sign(linear) * l1 - linear) / quadratic : 0       [a0 = accum, a1 = linear]
    adam     m = b1 m + (1 - b1) grad; v = b2 v + (1 - b2) grad^2
             var -= lr * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)                     [a0 = m, a1 = v]"""
    dt = np.dtype(dtype).type
    w, g, a0, a1 = (np.asarray(v, dtype=dtype) for v in (w, g, a0, a1))
    _, lr, beta1, beta2, eps, l1, l2, lr_power = (dt(v) for v in hyper)
    if kind == "sgd":
        return w - lr * g, a0, a1
    if kind == "adagrad":
        accum = a0 + g * g
        return w - lr * g / np.sqrt(accum), accum, a1
    if kind == "ftrl":
        accum_new = a0 + g * g
        if lr_power == dt(-0.5):
            p_new, p_old = np.sqrt(accum_new), np.sqrt(a0)
        else:
            p_new, p_old = np.power(accum_new, -lr_power), np.power(a0, -lr_power)
        linear = a1 + (g - (p_new - p_old) / lr * w)
        quadratic = p_new / lr + dt(2) * l2
        var = np.where(np.abs(linear) > l1, (np.sign(linear) * l1 - linear) / quadratic, dt(0))
        return var, accum_new, linear
    assert kind == "adam"
    t = dt(step)
    m = beta1 * a0 + (dt(1) - beta1) * g
    v = beta2 * a1 + (dt(1) - beta2) * g * g
    m_hat = m / (dt(1) - beta1 ** t)
    v_hat = v / (dt(1) - beta2 ** t)
    return w - lr * m_hat / (np.sqrt(v_hat) + eps), m, v


def _hyper(spec):
    return spec.encode().numpy().astype(np.float64)


class Case:
    """One optimizer problem on n state entries: which are live / DNN, the exact summed gradient of each step,
    and the initial float32 state (sentinels on entries that are not live)."""

    def __init__(self, live, dnn, grads, specs, rng):
        self.live, self.dnn, self.grads = live, dnn, grads
        n = live.size
        p = rng.uniform(-0.1, 0.1, n).astype(np.float32)
        s0 = np.zeros(n, np.float32)
        for sel, spec in ((dnn, specs[0]), (~dnn, specs[1])):
            if spec.kind in ("adagrad", "ftrl"):
                s0[sel] = np.float32(spec.initial_accumulator_value)
        s1 = np.zeros(n, np.float32)
        self.init = [p, s0, s1]
        for v, sent in zip(self.init, SENTINEL):
            v[~live] = sent


def _groups(case, specs):
    """(entries, their optimizer): the live DNN entries and the live wide entries."""
    return (case.live & case.dnn, specs[0]), (case.live & ~case.dnn, specs[1])


def _entries_of(case, specs, kind):
    sel = np.zeros_like(case.live)
    for s, spec in _groups(case, specs):
        if spec.kind == kind:
            sel |= s
    return sel


def _step_all(case, specs, state, grad, step, dtype):
    """One step of every live entry from the float32 state, computed in dtype; returns the state in dtype."""
    new = [v.astype(dtype) for v in state]
    for sel, spec in _groups(case, specs):
        res = ref_update(spec.kind, state[0][sel], grad[sel], state[1][sel], state[2][sel], step, _hyper(spec), dtype)
        for dst, v in zip(new, res):
            assert v.dtype == dtype
            dst[sel] = v
    return new


def reference(case, specs, step0):
    """Per step: val[k] the fp64 reference of param / s0 / s1 (state rounded to float32 between steps, as the kernels
    store it), E[k] the error of the float32 emulation (which runs its own trajectory), mag[k] the tensor's maximum
    magnitude, bound[k] = 8 E + 2 ulp, and alt: the fp64 param had the step number been one less / one more."""
    live = case.live
    state = {np.float64: case.init, np.float32: case.init}
    out = []
    for i in range(STEPS):
        step = step0 + i + 1
        new = {dt: _step_all(case, specs, state[dt], case.grads[i], step, dt) for dt in state}
        r = SimpleNamespace(val=new[np.float64], alt=[])
        if any(spec.kind == "adam" for spec in specs):
            r.alt = [_step_all(case, specs, state[np.float64], case.grads[i], other, np.float64)[0]
                     for other in (step - 1, step + 1) if other >= 1]
        r.E = [float(np.abs(a[live].astype(np.float64) - b[live]).max()) for a, b in zip(new[np.float32], r.val)]
        r.mag = [float(np.abs(b[live]).max()) for b in r.val]
        r.bound = [8 * e + 2 * float(np.spacing(np.float32(m))) for e, m in zip(r.E, r.mag)]
        out.append(r)
        state = {dt: [v.astype(np.float32) for v in new[dt]] for dt in new}
    return out


# ------------------------------------------------------------------------------------------------ inputs
_SLABS = {}


def slab_data(G, stride):
    """(base slab float32 [G, stride], exact column sums fp64 [stride]); entries k * 2**-8, |k| <= kmax(G) <= 256
    (so |k| <= 1024 after STEP_MULT), kmax shrinking with sqrt(G) to keep the column sums at a few units."""
    key = (G, stride)
    if key not in _SLABS:
        rng = np.random.default_rng([G, stride, 1])
        kmax = max(4, 256 >> int(round(np.log2(np.sqrt(G)))))
        base = (rng.integers(-kmax, kmax + 1, size=(G, stride)).astype(np.float32) * np.float32(2.0 ** -8))
        gsum = base.astype(np.float64).sum(0)
        # exact in fp32 whatever the order: also after the largest step multiplier
        assert np.array_equal(base.sum(0, dtype=np.float32).astype(np.float64), gsum)
        assert np.abs(base).max() * max(STEP_MULT) <= 4.0 and np.abs(gsum).max() * max(STEP_MULT) < 2.0 ** 15
        _SLABS[key] = (base, gsum)
    return _SLABS[key]


def synthetic_wsc(stride):
    """wsc [stride]: a mix of -1 (padding), -2 (wide) and DNN columns whose offsets are distinct entries of a bf16
    image with a few entries more than DNN columns. Returns (wsc, image size)."""
    rng = np.random.default_rng([stride, 2])
    kind = rng.choice(np.array([-1, -2, 0]), size=stride, p=[0.15, 0.25, 0.6])
    kind[:3] = (0, -2, -1)
    dnn = kind == 0
    wt_n = int(dnn.sum()) + 7
    wsc = kind.astype(np.int32)
    wsc[dnn] = rng.permutation(wt_n)[: int(dnn.sum())].astype(np.int32)
    return wsc, wt_n


def sc_case(G, stride, specs):
    _, gsum = slab_data(G, stride)
    wsc, wt_n = synthetic_wsc(stride)
    case = Case(wsc != -1, wsc >= 0, [gsum * m for m in STEP_MULT], specs, np.random.default_rng([G, stride, 3]))
    case.wsc, case.wt_n = wsc, wt_n
    return case


def zero_fractions(case, specs, ref):
    """Per step: share of the FTRL columns the reference leaves at exactly 0 (|linear| <= l1)."""
    sel = _entries_of(case, specs, "ftrl")
    if not sel.any():
        return 0, []
    return int(sel.sum()), [float((r.val[0][sel] == 0).mean()) for r in ref]


def _uses_l1(specs):
    return any(s.kind == "ftrl" and s.l1 > 0 for s in specs)


def assert_l1_split(case, specs, ref, tag):
    """Both sides of |linear| > l1 hold 20-80 % of the FTRL columns at some step (asserted where there are
    enough columns for a share to mean something)."""
    n, zf = zero_fractions(case, specs, ref)
    if _uses_l1(specs) and n >= 100:
        assert any(0.2 <= z <= 0.8 for z in zf), (tag, n, zf)
    return zf


# ------------------------------------------------------------------------------------------------ CPU tests
def _torch_optimizer(spec, p, step0):
    from mifx.trainer.optim import Ftrl, TFAdagrad

    h = _hyper(spec)
    lr, b1, b2, eps, l1, l2, lr_power = (float(v) for v in h[1:])
    init = float(np.float32(spec.initial_accumulator_value))
    if spec.kind == "adagrad":
        return TFAdagrad([p], lr=lr, initial_accumulator_value=init), ("acc", None)
    if spec.kind == "ftrl":
        return Ftrl([p], lr=lr, lr_power=lr_power, initial_accumulator_value=init, l1=l1, l2=l2), ("acc", "lin")
    if spec.kind == "sgd":
        return torch.optim.SGD([p], lr=lr), (None, None)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": torch.zeros_like(p),
                    "exp_avg_sq": torch.zeros_like(p)}
    return opt, ("exp_avg", "exp_avg_sq")


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reference_matches_cpu_optimizers(name):
    """ref_update in fp64 (state carried in fp64 here) against the optimizers the CPU trainer uses, on fp64 tensors:
    TFAdagrad, Ftrl, torch.optim.Adam, torch.optim.SGD; three steps, the GPU tests' hyperparameters and gradients."""
    dnn_spec, wide_spec, step0 = CONFIGS[name]
    _, gsum = slab_data(9, 260)
    for spec in (dnn_spec, wide_spec):
        rng = np.random.default_rng(7)
        w = rng.uniform(-0.1, 0.1, gsum.size)
        a0 = np.full(gsum.size, float(np.float32(spec.initial_accumulator_value))
                     if spec.kind in ("adagrad", "ftrl") else 0.0)
        a1 = np.zeros(gsum.size)
        p = torch.tensor(w, dtype=torch.float64, requires_grad=True)
        opt, names = _torch_optimizer(spec, p, step0)
        for i, mult in enumerate(STEP_MULT):
            g = gsum * mult
            w, a0, a1 = ref_update(spec.kind, w, g, a0, a1, step0 + i + 1, _hyper(spec))
            p.grad = torch.tensor(g, dtype=torch.float64)
            opt.step()
            np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-12, atol=1e-15, err_msg=f"{spec.kind} w {i}")
            for mine, key in zip((a0, a1), names):
                if key is not None:
                    np.testing.assert_allclose(mine, opt.state[p][key].numpy(), rtol=1e-12, atol=1e-15,
                                               err_msg=f"{spec.kind} {key} {i}")
        if spec.kind == "ftrl" and spec.l1 > 0:
            assert 0 < (w == 0).mean() < 1


@pytest.mark.parametrize("name", [k for k, v in CONFIGS.items() if _uses_l1(v[:2])])
def test_ftrl_l1_splits_the_reference_columns(name):
    """The reference takes both branches of the L1 shrinkage on 20-80 % of the FTRL columns at some step, for every
    row count (small strides: few columns, checked at stride 1028 here and on every large case in the GPU tests)."""
    specs = CONFIGS[name][:2]
    for G in G_ALL:
        case = sc_case(G, 1028, specs)
        zf = assert_l1_split(case, specs, reference(case, specs, 0), (name, G))
        print(f"[wd-opt-l1] {name} G={G} zero share per step {['%.2f' % z for z in zf]}")


def test_tolerance_is_tight():
    """The float32 emulation stays within a few float32 ulps (relative to the tensor's maximum) of the fp64
    reference over the three steps, so 8 * E + 2 ulp is a tight bound, not a loose one: the worst E allowed here is
    2**-18 of the magnitude (32 float32 epsilons)."""
    for name, (hd, hw, step0) in CONFIGS.items():
        for G, stride in ((1, 1028), (129, 1028), (300, 1028)):
            case = sc_case(G, stride, (hd, hw))
            for i, r in enumerate(reference(case, (hd, hw), step0)):
                rel = [e / m if m else 0.0 for e, m in zip(r.E, r.mag)]
                print(f"[wd-opt-E] {name} G={G} step {step0 + i + 1} E/max param {rel[0]:.2e} s0 {rel[1]:.2e} "
                      f"s1 {rel[2]:.2e}")
                assert max(rel) <= 2.0 ** -18, (name, G, i, rel)


# ------------------------------------------------------------------------------------------------ GPU harness
TENSORS = ("param", "s0", "s1")


class Stats:
    """Worst figures of one config over all its cases, relative to the tensor's maximum magnitude."""

    def __init__(self, name):
        self.name, self.runs, self.identical = name, 0, True
        self.worst = {t: [0.0, 0.0, 0.0] for t in TENSORS}  # E / max, GPU error / max, GPU error / bound

    def add(self, tensor, e, err, bound, mag):
        w = self.worst[tensor]
        if mag == 0:  # a state tensor this optimizer never writes: nothing to relate an error to
            assert e == 0
            mag = 1.0
        for k, v in enumerate((e / mag, err / mag, err / bound)):
            w[k] = max(w[k], v)

    def report(self, what):
        for t in TENSORS:
            e, g, b = self.worst[t]
            print(f"[wd-opt-err] {what} {self.name} {t}: E/max {e:.2e} gpu/max {g:.2e} gpu/bound {b:.3f}")
        print(f"[wd-opt-err] {what} {self.name}: {self.runs} runs, variants bit-identical: {self.identical}")


def _bf16_bits(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).view(torch.int16).numpy()


def _bits(x):
    return x.view(np.uint32)


def run_steps(case, slabs, call, step0, wt_n, post=None):
    """STEPS consecutive calls on fresh device state; after each: (state [3, n], bf16 image, step slots) as numpy."""
    state = torch.from_numpy(np.stack(case.init)).cuda()
    wt = torch.full((wt_n,), WT_SENTINEL, dtype=torch.int16, device="cuda")
    ctr = torch.full((STEP_SLOTS,), step0, dtype=torch.int64, device="cuda")
    outs = []
    for slab in slabs:
        call(slab, state[0], state[1], state[2], wt, ctr)
        torch.cuda.synchronize()
        if post is not None:
            post()
        outs.append((state.cpu().numpy(), wt.cpu().numpy(), ctr.cpu().numpy()))
    return outs


def check_run(tag, case, ref, outs, step0, wt_pos, wt_off, owned, all_slots, stats):
    """wt_pos: state entries whose bf16 image the entry point writes, wt_off: their image offsets. owned: step slots
    of the launched workgroups; all_slots: the kernel promises to keep every slot equal."""
    live = case.live
    stats.runs += 1
    for i, (state, wt, ctr) in enumerate(outs):
        r = ref[i]
        for k, t in enumerate(TENSORS):
            got = state[k]
            assert np.array_equal(_bits(got[~live]), _bits(case.init[k][~live])), (tag, i, t, "sentinel touched")
            err = np.abs(got[live].astype(np.float64) - r.val[k][live])
            worst = float(err.max())
            stats.add(t, r.E[k], worst, r.bound[k], r.mag[k])
            assert worst <= r.bound[k], (tag, f"step {step0 + i + 1}", t, f"err {worst:.3e} E {r.E[k]:.3e} "
                                         f"bound {r.bound[k]:.3e} at live entry {int(err.argmax())}")
        want = np.full(wt.size, WT_SENTINEL, np.int16)
        want[wt_off] = _bf16_bits(state[0][wt_pos])
        assert np.array_equal(wt, want), (tag, i, "bf16 image")
        slots = np.full(STEP_SLOTS, step0, np.int64)
        slots[:STEP_SLOTS if all_slots else owned] = step0 + i + 1
        assert np.array_equal(ctr, slots), (tag, i, "step slots", ctr[:4], int((ctr != slots).sum()))
        # Adam: wherever the reference at step -/+ 1 is told apart from the reference at the step (by more than
        # twice the bound), the kernel's value must be nearer the latter
        for alt in r.alt:
            sep = live & (np.abs(alt - r.val[0]) > 2 * r.bound[0])
            wrong = np.abs(state[0][sep] - alt[sep]) <= np.abs(state[0][sep] - r.val[0][sep])
            assert not wrong.any(), (tag, f"step {step0 + i + 1}", int(wrong.sum()), "entries match another step")


def assert_steps_separable(case, ref, specs, step0, tag):
    """At steps 1..3 Adam's bias correction must tell step -/+ 1 apart on (nearly) every live Adam entry."""
    adam = _entries_of(case, specs, "adam")
    if step0 != 0 or adam.sum() < 100:
        return
    for r in ref:
        for alt in r.alt:
            share = float((np.abs(alt - r.val[0])[adam] > 2 * r.bound[0]).mean())
            assert share >= 0.9, (tag, share)


def assert_same_bits(tag, a, b, stats):
    for i, ((sa, wa, _), (sb, wb, _)) in enumerate(zip(a, b)):
        same = np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(wa, wb)
        stats.identical &= same
        assert same, (tag, i, "not bit-identical to the first variant")


def _tall_slabs(G, stride):
    """The slab of every step with NaN rows below row G (nothing may read them)."""
    tall = torch.full((G + 3, stride), float("nan"), device="cuda")
    tall[:G] = torch.from_numpy(slab_data(G, stride)[0]).cuda()
    return [tall * m for m in STEP_MULT]


def _xcd_labels(G):
    g = torch.Generator(device="cpu").manual_seed(5)
    return (("mod8", torch.arange(G) % 8), ("all13", torch.full((G,), 13)),
            ("rand16", torch.randint(0, 16, (G,), generator=g)), ("all3", torch.full((G,), 3)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_slab_order_entry_points_match_reference(name):
    """reduce_apply_sc (wd_reduce_opt_sc, wd_opt1_sc at G == 1), ResReduce.apply_sc two-launch (wd_reduce_res +
    wd_res_opt_sc<1>) and fused (wd_reduce_res_fused) and XcdReduce.apply_sc (wd_reduce_xcd + wd_xcd_opt_sc<1>,
    four row-label patterns) on synthetic wsc: three consecutive calls, each compared with the fp64 reference, and
    all variants bit-identical to each other (230 runs of three calls per config).

    Observed on MI355X, worst over all cases and steps, as E / max, GPU error / max [GPU error / bound] per tensor
    (max = the tensor's maximum magnitude; printed with -s as [wd-opt-err]); all variants bit-identical everywhere:
      default       param 2.5e-7, 2.3e-7 [0.19]   s0 5.9e-8, 5.9e-8 [0.08]   s1 1.7e-7, 1.4e-7 [0.33]
      ftrl_l1l2     param 2.2e-7, 2.2e-7 [0.16]   s0 5.9e-8, 5.9e-8 [0.08]   s1 1.3e-7, 1.3e-7 [0.24]
      ftrl_pow075   param 3.1e-7, 2.5e-7 [0.21]   s0 5.9e-8, 5.9e-8 [0.08]   s1 1.5e-7, 1.6e-7 [0.23]
      swapped       param 2.8e-7, 2.4e-7 [0.34]   s0 5.9e-8, 5.9e-8 [0.08]   s1 1.9e-7, 1.9e-7 [0.24]
      adam_step0    param 5.1e-7, 5.1e-7 [0.12]   s0 1.1e-7, 1.1e-7 [0.11]   s1 9.5e-8, 9.5e-8 [0.10]
      adam_step999  param 2.2e-7, 1.6e-7 [0.17]   s0 1.1e-7, 1.1e-7 [0.11]   s1 9.5e-8, 9.5e-8 [0.10]
      sgd           param 1.2e-7, 5.3e-8 [0.08]   s0, s1 untouched
    The GPU error never exceeded E by more than a few per cent (the device's contracted FMAs round once where the
    emulation rounds twice, so the two differ in the last bit here and there). No entry was nearer the reference
    of step -/+ 1: the step read without a barrier in wd_res_opt_sc<1> / wd_reduce_res_fused was not seen to
    misbehave. Before opt_update's Adam branch was excluded from FMA contraction, the Adam variants were within
    the bound but NOT bit-identical from the second call on (first seen: G = 1, stride 68, wd_opt1_sc against
    wd_res_opt_sc<1>)."""
    from mifx.ops import wide_deep as wdk

    hd, hw, step0 = CONFIGS[name]
    specs = (hd, hw)
    h_dnn, h_wide = hd.encode(), hw.encode()
    stats, reducers = Stats(name), {}
    try:
        for G, stride in PAIRS:
            tag = (name, G, stride)
            case = sc_case(G, stride, specs)
            ref = reference(case, specs, step0)
            assert_l1_split(case, specs, ref, tag)
            assert_steps_separable(case, ref, specs, step0, tag)
            slabs = _tall_slabs(G, stride)
            wsc = torch.from_numpy(case.wsc).cuda()
            if stride not in reducers:
                reducers[stride] = (wdk.ResReduce(stride, "cuda", fused=False),
                                    wdk.ResReduce(stride, "cuda", fused=True), wdk.XcdReduce(stride, "cuda"))
            res2, res1, xr = reducers[stride]
            wt_pos = np.nonzero(case.wsc >= 0)[0]
            wt_off = case.wsc[wt_pos]

            def via(fn):
                return lambda s, p, a, b, wt, c: fn(s, G, wsc, p, a, b, wt, c, h_dnn, h_wide)

            def tickets_zero():
                assert int(res1.ticket.abs().sum()) == 0, (tag, "ticket not reset")

            owned = -(-stride // 256) if G == 1 else -(-stride // 64)  # wd_opt1_sc / wd_reduce_opt_sc workgroups
            first = run_steps(case, slabs, via(wdk.reduce_apply_sc), step0, case.wt_n)
            check_run(tag + ("reduce_apply_sc",), case, ref, first, step0, wt_pos, wt_off, owned, False, stats)
            runs = [("res", via(res2.apply_sc), None), ("res_fused", via(res1.apply_sc), tickets_zero)]
            if G <= XCD_MAX_G:
                for lname, labels in _xcd_labels(G):
                    def xcd_call(s, p, a, b, wt, c, labels=labels):
                        xr.xcd_of[:G] = labels.to(torch.int32).cuda()
                        xr.apply_sc(s, G, wsc, p, a, b, wt, c, h_dnn, h_wide)

                    runs.append(("xcd_" + lname, xcd_call, None))
            for vname, call, post in runs:
                outs = run_steps(case, slabs, call, step0, case.wt_n, post)
                check_run(tag + (vname,), case, ref, outs, step0, wt_pos, wt_off, STEP_SLOTS, True, stats)
                assert_same_bits(tag + (vname,), first, outs, stats)
    finally:
        stats.report("slab-order")


def _model_maps():
    """(name, gidx, mask, stride, inv, wmap or None, image size) of the tile kernel and of the chained kernel, built
    as FusedWideDeepTrainer.__init__ builds them."""
    out = []
    gidx, mask = wdm.canonical_index_maps()
    out.append(("tile", gidx, mask, int(wdm.compact_tile_map()[1]), None, wdm.WTOT))
    _, stride, gidx, mask, wmap = wdm.chain_maps()
    out.append(("chain", gidx, mask, int(stride), wmap, wdm.CHAIN_LWEND))
    res = []
    for mname, gidx, mask, stride, wmap, wt_n in out:
        inv = np.full(stride, -1, dtype=np.int32)
        live = np.nonzero(mask)[0]
        inv[gidx[live]] = live.astype(np.int32)
        res.append((mname, gidx, mask, stride, inv, wmap, wt_n))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_canonical_entry_points_match_reference(name):
    """reduce_apply (wd_reduce_opt<true>; canonical image and through wmap) and reduce + optimizer (wd_reduce +
    wd_optimizer, several splits) on the model's own index maps: canonical-order state, the same reference; the
    two-launch state must equal reduce_apply's bit for bit (98 runs of three calls per config).

    Observed on MI355X (E / max, GPU error / max [GPU error / bound], as in the slab-order test), all variants
    bit-identical:
      default       param 2.3e-7, 2.0e-7 [0.13]   s0 5.3e-8, 5.3e-8 [0.08]   s1 1.6e-7, 1.6e-7 [0.15]
      ftrl_l1l2     param 2.8e-7, 2.0e-7 [0.13]   s0 5.3e-8, 5.3e-8 [0.08]   s1 1.6e-7, 1.2e-7 [0.14]
      ftrl_pow075   param 2.6e-7, 2.6e-7 [0.19]   s0 5.3e-8, 5.3e-8 [0.08]   s1 1.7e-7, 1.9e-7 [0.18]
      swapped       param 3.2e-7, 2.9e-7 [0.14]   s0 5.3e-8, 5.3e-8 [0.08]   s1 1.9e-7, 1.8e-7 [0.16]
      adam_step0    param 3.3e-7, 3.3e-7 [0.12]   s0 1.1e-7, 1.1e-7 [0.10]   s1 8.0e-8, 8.0e-8 [0.10]
      adam_step999  param 2.1e-7, 1.6e-7 [0.11]   s0 1.1e-7, 1.1e-7 [0.10]   s1 8.0e-8, 8.0e-8 [0.10]
      sgd           param 1.2e-7, 5.3e-8 [0.08]   s0, s1 untouched"""
    from mifx.ops import wide_deep as wdk

    hd, hw, step0 = CONFIGS[name]
    specs = (hd, hw)
    h_dnn, h_wide = hd.encode(), hw.encode()
    n = wdm.WTOT + wdm.NWIDE
    dnn = np.arange(n) < wdm.WTOT
    stats = Stats(name)
    try:
        for mname, gidx, mask, stride, inv, wmap, wt_n in _model_maps():
            live = mask.astype(bool)
            gidx_t, mask_t, inv_t = (torch.from_numpy(v).cuda() for v in (gidx, mask, inv))
            wmap_t = None if wmap is None else torch.from_numpy(wmap).cuda()
            live_dnn = np.nonzero(live & dnn)[0]
            for G in G_ALL:
                tag = (name, mname, G)
                gsum = slab_data(G, stride)[1]
                case = Case(live, dnn, [np.where(live, (gsum * m)[gidx], 0.0) for m in STEP_MULT], specs,
                            np.random.default_rng([G, stride, 4]))
                ref = reference(case, specs, step0)
                assert_l1_split(case, specs, ref, tag)
                assert_steps_separable(case, ref, specs, step0, tag)
                slabs = _tall_slabs(G, stride)
                first = run_steps(case, slabs, lambda s, p, a, b, wt, c: wdk.reduce_apply(
                    s, G, inv_t, p, a, b, wt, c, h_dnn, h_wide, wmap_t), step0, wt_n)
                check_run(tag + ("reduce_apply",), case, ref, first, step0, live_dnn,
                          live_dnn if wmap is None else wmap[live_dnn], -(-stride // 64), False, stats)
                # wd_reduce splits the rows into nsplit chunks (4-way unrolled), wd_optimizer adds the nsplit
                # partials (4-way unrolled); the trainer's own split is max(1, min(16, G // 8))
                splits = sorted({s for s in (1, 3, 5, 16, max(1, min(16, G // 8))) if s <= G})
                for ns in ([None] if G == 1 else []) + splits:
                    partial = None if ns is None else torch.full((ns + 1, stride), float("nan"), device="cuda")

                    def two_launch(s, p, a, b, wt, c, ns=ns, partial=partial):
                        if ns is None:  # one slab row: the optimizer reads it directly
                            wdk.optimizer(s, 1, gidx_t, mask_t, p, a, b, wt, c, h_dnn, h_wide)
                            return
                        wdk.reduce(s, G, ns, partial)
                        wdk.optimizer(partial, ns, gidx_t, mask_t, p, a, b, wt, c, h_dnn, h_wide)

                    outs = run_steps(case, slabs, two_launch, step0, wdm.WTOT)
                    allc = np.arange(wdm.WTOT)  # wd_optimizer re-emits every DNN entry, frozen ones included
                    check_run(tag + ("reduce+optimizer", ns), case, ref, outs, step0, allc, allc, (n + 255) // 256,
                              False, stats)
                    for i, ((sa, _, _), (sb, _, _)) in enumerate(zip(first, outs)):  # (images differ in layout)
                        same = np.array_equal(_bits(sa), _bits(sb))
                        stats.identical &= same
                        assert same, (tag, ns, i, "reduce+optimizer state differs from reduce_apply")
    finally:
        stats.report("canonical")
