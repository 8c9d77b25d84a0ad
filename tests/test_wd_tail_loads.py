"""wd_res_opt_sc (through ResReduce.apply_sc) and wd_opt1_sc (reduce_apply_sc on one slab row) issue every load of a
column -- partials or slab entry, wsc, param, s0, s1, step slot -- unconditionally at the column clamped into
[0, stride), and decide by wsc and by gi < stride only what is STORED (csrc/wd_opt.h sc_load / sc_landed / sc_update).
What that can break, checked on synthetic state:

  * a stride that is no multiple of 256: the last workgroup has threads past the last column, which load the clamped
    column and must store nothing;
  * padding (-1), wide (-2) and DNN columns interleaved inside one wave, and one whole wave of padding: param, s0, s1
    and the bf16 image keep a sentinel bit pattern at every padding column;
  * the live columns against the fp64 reference of tests/test_wd_optimizer.py (its inputs make every fp32 column sum
    exact in any order, so the fixed-order sums of the kernels are the exact sums; its bound 8 E + 2 ulp);
  * every step slot (the fanned-out ones included) moved by one per call; two runs byte-equal."""
import numpy as np
import pytest
import torch

from tests.test_wd_optimizer import (CONFIGS, STEP_MULT, STEP_SLOTS, STEPS, Case, Stats, assert_same_bits, check_run,
                                     reference, run_steps, slab_data)

STRIDE = 2 * 256 + 100  # three level-2 / wd_opt1_sc workgroups, the last with 156 threads past the last column
KINDS = {"default": ("adagrad", "ftrl"), "adam_step999": ("adam", "adam"), "sgd": ("sgd", "sgd"),
         "swapped": ("ftrl", "adagrad")}


def interleaved_wsc(stride):
    """Column c: padding, wide, DNN, DNN, wide, padding, DNN in turn (every wave of 64 holds all three kinds next to
    each other), columns 64..127 -- the second wave of the first workgroup -- all padding. DNN columns get distinct
    offsets into an image with a few entries more than DNN columns."""
    kind = np.array([-1, -2, 0, 0, -2, -1, 0])[np.arange(stride) % 7]
    kind[64:128] = -1
    dnn = kind == 0
    wt_n = int(dnn.sum()) + 5
    wsc = kind.astype(np.int32)
    wsc[dnn] = np.random.default_rng(11).permutation(wt_n)[: int(dnn.sum())].astype(np.int32)
    return wsc, wt_n


def _case(G, specs):
    _, gsum = slab_data(G, STRIDE)
    wsc, wt_n = interleaved_wsc(STRIDE)
    case = Case(wsc != -1, wsc >= 0, [gsum * m for m in STEP_MULT], specs, np.random.default_rng([G, STRIDE, 3]))
    case.wsc, case.wt_n = wsc, wt_n
    return case


def test_synthetic_columns():
    assert STRIDE % 256 and STRIDE % 4 == 0 and STEPS == 3
    wsc, wt_n = interleaved_wsc(STRIDE)
    assert (wsc[64:128] == -1).all()
    for w0 in range(0, STRIDE, 64):
        if w0 != 64:
            assert {-1, -2} <= set(wsc[w0:w0 + 64].tolist()) and (wsc[w0:w0 + 64] >= 0).any()
    off = wsc[wsc >= 0]
    assert len(np.unique(off)) == len(off) and off.max() < wt_n
    assert {k for v in KINDS.values() for k in v} == {"sgd", "adagrad", "ftrl", "adam"}
    for name, kinds in KINDS.items():
        assert tuple(s.kind for s in CONFIGS[name][:2]) == kinds


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 8, 16])
@pytest.mark.parametrize("name", list(KINDS))
def test_tail_kernels_store_only_live_columns(name, G):
    from mifx.ops import wide_deep as wdk

    hd, hw, step0 = CONFIGS[name]
    specs = (hd, hw)
    h_dnn, h_wide = hd.encode(), hw.encode()
    case = _case(G, specs)
    ref = reference(case, specs, step0)
    tall = torch.full((G + 3, STRIDE), float("nan"), device="cuda")  # rows below G: nothing may read them
    tall[:G] = torch.from_numpy(slab_data(G, STRIDE)[0]).cuda()
    slabs = [tall * m for m in STEP_MULT]
    wsc = torch.from_numpy(case.wsc).cuda()
    wt_pos = np.nonzero(case.wsc >= 0)[0]
    wt_off = case.wsc[wt_pos]
    stats = Stats(name)
    if G == 1:  # wd_opt1_sc: its workgroups own ceil(stride / 256) slots and fan nothing out
        fn, owned, all_slots = wdk.reduce_apply_sc, -(-STRIDE // 256), False
    else:       # wd_reduce_res + wd_res_opt_sc
        fn, owned, all_slots = wdk.ResReduce(STRIDE, "cuda", fused=False).apply_sc, STEP_SLOTS, True

    def call(s, p, a, b, wt, c):
        fn(s, G, wsc, p, a, b, wt, c, h_dnn, h_wide)

    tag = (name, G, STRIDE)
    first = run_steps(case, slabs, call, step0, case.wt_n)
    check_run(tag, case, ref, first, step0, wt_pos, wt_off, owned, all_slots, stats)
    ctr = first[-1][2]
    assert (ctr[:owned] == step0 + STEPS).all()
    again = run_steps(case, slabs, call, step0, case.wt_n)
    assert_same_bits(tag + ("second run",), first, again, stats)
    assert np.array_equal(first[-1][2], again[-1][2])
    stats.report("tail-loads")
