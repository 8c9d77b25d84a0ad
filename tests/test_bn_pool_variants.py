"""The A/B variants of the pool and tile-statistics kernels give the bits of the default paths.

csrc/pool.hip promises that maxpool_fwd (one window per thread, MIFX_POOL_PAIR=0) and maxpool_bwd on even pad-1
images (MIFX_POOL_EVEN=0) are bit-identical to maxpool_fwd2 / maxpool_bwd_even, and csrc/bn_relu.hip that the
one-launch tile finalize (MIFX_BN_TILES_ONE_LAUNCH, fences + arrival ticket) merges in the same order as the two-launch
form. The switches are read once per process, so one fresh child process (tests/bn_pool_child.py) recomputes the
grids of test_pool_exact.py and of test_bn_relu_exact.py's tile statistics with the switches set; this process
computes them on the default paths, which those two modules pin to the references.

Not reached: the `long long` index instantiations of the pool kernels, which need more than 4e9 work items.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bn_pool_child as child


@pytest.mark.gpu
def test_variant_kernels_are_bit_identical_to_default_paths(tmp_path):
    for k in child.SWITCHES:
        assert k not in os.environ, f"{k} is set: this process would not run the default path"
    out = tmp_path / "variants.npz"
    env = dict(os.environ, **child.SWITCHES)
    r = subprocess.run([sys.executable, child.__file__, str(out)], env=env, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, f"child exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    want = child.pool_outputs()
    want.update(child.tile_outputs())
    with np.load(out) as got:
        assert sorted(got.files) == sorted(want)
        diff = [k for k in want if got[k].shape != want[k].shape or got[k].tobytes() != want[k].tobytes()]
    assert not diff, f"{len(diff)} of {len(want)} outputs differ from the default path, first: {diff[:8]}"
    # the ticket reset: the second call of every tile case (in either process) repeats the first
    twice = [k for k in want if "__0__" in k and want[k].tobytes() != want[k.replace("__0__", "__1__")].tobytes()]
    assert not twice, twice[:8]
