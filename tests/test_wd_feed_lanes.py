"""The record fetch of the chained Wide&Deep kernel (csrc/wd_chain.hip fetch, through csrc/feed.h) at the shapes
tests/test_shuffle.py does not reach. A wave of the T = 256 build carries two 16-row column blocks; a lane evaluates
the feed for one of them and takes the other block's record index from lane ^ 16, so a wrong lane pairing, a wrong
block or a wrong row clamp trains on another record and changes the weights. The T = 64 and T = 128 builds evaluate
the feed per block; they run the same cases.

Training: a trainer with a shuffle seed must end with parameters torch.equal to a trainer fed
mifx.data.shuffle.record_indices in stored order, on every build (T = 64: batches 33 and 40; T = 128: 129; T = 256: 256
and 257), with n_data % 4 in {1, 2, 3} (records past the last whole shuffle group keep their place) and n_data chosen so
that within the first 6 steps one batch crosses the epoch boundary strictly inside a 16-row block and another exactly
between the two 16-row blocks of a wave's 32 rows (the two lanes of a pair then sit in different epochs). Batch 256
cannot have the second kind with n_data % 4 != 0 (pick_n says why) and takes a crossing inside a wave's second block.

Eval / predict (no step counter, fixed start s): the logits of rows s .. s + batch - 1 must equal, bit for bit, the
logits from start 0 over the records shifted by s."""
import functools

import numpy as np
import pytest
import torch

from mifx.data import shuffle as sh
from mifx.data.synthetic import synthetic_records
from mifx.models import wide_deep as wdm

gpu = pytest.mark.gpu
STEPS = 6


def crossings(batch, n, steps=STEPS):
    """Rows (0 < row < batch) at which a step's batch passes from one epoch into the next."""
    rows = []
    for s in range(steps):
        start = (s * batch) % n
        if start + batch > n:
            rows.append(n - start)
    return rows


@functools.lru_cache(maxsize=None)
def pick_n(batch, mod):
    """The smallest n_data > batch with n % 4 == mod whose first STEPS steps hold a crossing strictly inside a 16-row
    block (row % 16 != 0) and one exactly between the two blocks of a wave's 32 rows (row % 32 == 16). Rows count from
    the start of the batch; every workgroup tile (64, 128, 256) is a multiple of 32, so they are also the rows inside
    the workgroup that meets the crossing.

    A crossing at row r in step s means (k + 1) n = s batch + r for some k. With r = 16 + 32 j and an even batch the
    right side is a multiple of 8 (batch 40) or 16 (batch 256), so an odd n would have to divide 5 s + 2 + 4 j resp.
    16 s + 1 + 2 j, and n = 2 m (m odd) at batch 256 would need m to divide that: both smaller than the batch for
    s < 6. Hence batch 40 has the between-blocks crossing only for n % 4 == 2 and batch 256 for no n % 4 != 0; batch
    256 asks instead (between=False) for a crossing inside the SECOND block of a wave (row % 32 > 16), and the
    between-blocks crossing of the T = 256 build is covered at batch 257."""
    between = batch != 256
    for n in range(batch + 1, 4 * batch + 64):
        rows = crossings(batch, n)
        if n % 4 == mod and any(r % 16 for r in rows) and any(r % 32 == 16 if between else r % 32 > 16 for r in rows):
            return n
    raise AssertionError((batch, mod))




def _trainer(batch, tile, **kw):
    from mifx.trainer.fused_wide_deep import FusedWideDeepTrainer

    if tile == 256:  # as tests/test_wd_chain_live_tiles.py: T = 256 when ceil(batch / 128) > max_grid >= ceil(batch / 256)
        kw = {"large_tile": True, "max_grid": (batch + 255) // 256, **kw}
    else:
        kw = {"large_tile": False, "small_tile": tile == 64, **kw}
    tr = FusedWideDeepTrainer(wdm.WideDeepModel(seed=2), batch=batch, device=torch.device("cuda"), **kw)
    assert (tr.tile, tr.grid) == (tile, (batch + tile - 1) // tile)
    return tr


@functools.lru_cache(maxsize=None)
def _records(n):
    return synthetic_records(n, device="cuda", seed=5)


def _train(tile, batch, recs, seed):
    tr = _trainer(batch, tile, shuffle_seed=seed)
    tr.set_data(recs)
    for _ in range(STEPS):
        tr.step()
    torch.cuda.synchronize()
    assert tr.steps_done == STEPS
    return tr


CASES = [(64, 33, 1), (64, 33, 2), (64, 40, 2), (128, 129, 1), (128, 129, 2), (128, 129, 3), (256, 256, 1),
         (256, 256, 3), (256, 257, 1), (256, 257, 2), (256, 257, 3)]


def test_chosen_sizes_cross_the_epoch_inside_and_between_blocks():
    assert {m for _, _, m in CASES} == {1, 2, 3} and {b for _, b, _ in CASES} == {33, 40, 129, 256, 257}
    for _, batch, mod in CASES:
        n = pick_n(batch, mod)
        rows = crossings(batch, n)
        assert n % 4 == mod and n > batch
        assert any(r % 16 for r in rows), (batch, n, rows)
        assert any(r % 32 == 16 if batch != 256 else r % 32 > 16 for r in rows), (batch, n, rows)
        assert (n >> 2) << 2 < n  # records past the last whole group
        print(f"[feed-lanes] batch {batch} n {n}: epoch crossings at rows {rows}")


@gpu
@pytest.mark.parametrize("seed", [0, 0xC0FFEE])
@pytest.mark.parametrize("tile,batch,mod", CASES)
def test_fetches_the_named_records(tile, batch, mod, seed):
    n = pick_n(batch, mod)
    recs = _records(n)
    a = _train(tile, batch, recs, seed)
    order = np.concatenate([sh.record_indices(s, batch, n, seed=seed) for s in range(STEPS)])
    if seed == 0:
        assert np.array_equal(order, np.arange(STEPS * batch) % n)
    b = _train(tile, batch, recs[torch.from_numpy(order).cuda()].contiguous(), 0)
    for name in ("param", "s0", "s1"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (name, n)
    assert a.last_loss() == b.last_loss()
    again = _train(tile, batch, recs, seed)  # two runs: byte-equal
    for name in ("param", "s0", "s1", "wt"):
        assert torch.equal(getattr(a, name), getattr(again, name)), name


@gpu
@pytest.mark.parametrize("tile,batch", [(64, 40), (128, 257), (256, 257)])
def test_fixed_start_reads_the_shifted_records(tile, batch):
    from mifx.ops import wd_chain as wdc

    n = batch + 35  # n % 4 == 3 (batch 40) / 0 (batch 257): the fixed start ignores the shuffle groups either way
    recs = _records(n)
    tr = _trainer(40 if tile == 64 else 129 if tile == 128 else 256, tile)
    grid, waves = (batch + tile - 1) // tile, 4 if tile == 64 else 8

    def logits(records, n_data, start):
        out = torch.full((batch,), float("nan"), device="cuda")
        wdc.fused(records, n_data, batch, start, None, tr.wt, tr.wide_weights, None, None, out, 1.0, grid, False, None,
                  waves, None, tile=tile)
        torch.cuda.synchronize()
        return out

    for s in (0, 5, 31):
        got = logits(recs, n, s)
        want = logits(recs[s:s + batch].contiguous(), batch, 0)
        assert torch.isfinite(got).all()
        assert torch.equal(got, want), s
        assert torch.equal(got, logits(recs, n, s)), (s, "second run")
    assert not torch.equal(logits(recs, n, 0), logits(recs, n, 5))
