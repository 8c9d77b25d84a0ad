"""GPU runs of the shared pool and tile-statistics grids (tests/bn_pool_ref.py), importable and runnable.

The A/B switches of csrc/pool.hip (MIFX_POOL_PAIR, MIFX_POOL_EVEN) and csrc/bn_relu.hip (MIFX_BN_TILES_ONE_LAUNCH)
are read once per process, so tests/test_bn_pool_variants.py computes the grids in its own process (default paths)
with the functions below and starts this file once as a fresh child with the switches set:

    python tests/bn_pool_child.py OUT.npz

The child requires the three switches in its environment, recomputes both grids (each tile case twice in a row: the
one-launch finalize's arrival ticket must be back at zero for the second call) and writes the raw outputs to OUT.npz.
"""
from __future__ import annotations

import os
import sys

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import bn_pool_ref as R

EPS = 1e-5
SWITCHES = {"MIFX_POOL_PAIR": "0", "MIFX_POOL_EVEN": "0", "MIFX_BN_TILES_ONE_LAUNCH": "1"}
TILE_Y_MAX_T = 1000  # y = bn_apply(stats) is kept up to this T (the larger case's y would dominate the file)


def bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()


def run_pool_case(x, pt, pl, OH, OW, relu, dy):
    """(y, pos, dx) of the HIP pool on the GPU; pos is the uint8 [N, OH, OW, C] tensor the forward saved."""
    from mifx.ops.pool import _MaxPool3s2

    xg = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_()
    y = _MaxPool3s2.apply(xg, pt, pl, OH, OW, relu)
    (pos,) = y.grad_fn.saved_tensors
    y.backward(dy.cuda())
    return y.detach(), pos, xg.grad


def run_tile_case(x, part, momentum=0.1, relu=True, apply=True):
    """(y, stats, run_mean, run_var) of the tile-statistics forward on the GPU, from fresh running statistics."""
    import mifx.ops.bn_relu as bnr

    w, b, rm0, rv0 = (t.cuda() for t in R.bn_params(x.shape[1]))
    y, _, stats = bnr._fwd_tiles(x.cuda(), part.cuda(), w, b, rm0, rv0, momentum, EPS, relu, apply=apply)
    return y, stats, rm0, rv0


def pool_outputs() -> dict:
    out = {}
    for name, *case in R.pool_grid():
        for key, t in zip(("y", "pos", "dx"), run_pool_case(*case)):
            out[f"pool__{name}__{key}"] = bits(t)
    return out


def tile_outputs() -> dict:
    out = {}
    for name, x, part in R.tile_grid():
        for call in (0, 1):
            y, stats, rm, rv = run_tile_case(x, part)
            for key, t in (("stats", stats), ("run_mean", rm), ("run_var", rv)):
                out[f"tile__{name}__{call}__{key}"] = bits(t)
        if part.shape[1] <= TILE_Y_MAX_T:
            out[f"tile__{name}__y"] = bits(y)
    return out


def main(path: str) -> None:
    for k, v in SWITCHES.items():
        assert os.environ.get(k) == v, f"{k} must be {v} in the child's environment"
    out = pool_outputs()
    out.update(tile_outputs())
    torch.cuda.synchronize()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
