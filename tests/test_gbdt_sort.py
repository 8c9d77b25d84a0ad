"""The batched radix sort of feature columns (csrc/gbdt_sort.hip, mifx.ops.gbdt_prep.device_sort_columns) against
numpy: per column the same multiset of bit patterns in nondecreasing order with the NaNs last, the same bits for any
tile, column range and grouping, and through device_cuts the host's cuts on both sort routes."""
import numpy as np
import pytest
import torch

from mifx.ops import gbdt_prep as P
from test_gbdt_prep import DEV, host_tables, mixed_matrix, up

pytestmark = pytest.mark.gpu

T = P.SORT_TILE
DTYPES = [np.float64, np.float32]


def table(n, dtype, seed):
    """mixed_matrix plus the columns a radix sort can get wrong: [n, 12 + 6] of `dtype`."""
    r = np.random.default_rng(seed)
    u = {np.float64: np.uint64, np.float32: np.uint32}[dtype]
    shift = 32 if dtype is np.float64 else 0  # NaNs of both signs, quiet and signalling, with payloads
    nans = (np.array([0xFFF80000, 0x7FF00001, 0xFFF40123, 0x7FFFFFFF], np.uint64) << shift).astype(u).view(dtype)
    assert np.isnan(nans).all()
    odd = r.standard_normal(n).astype(dtype)
    pick = r.random(n) < 0.4
    odd[pick] = nans[r.integers(0, 4, int(pick.sum()))]
    tiny = (r.integers(-3, 4, n) * np.finfo(dtype).smallest_subnormal).astype(dtype)
    tiny[r.random(n) < 0.2] = -0.0
    step = 16 if dtype is np.float64 else 2  # exponents that differ in the key's top byte only
    top = (np.where(r.random(n) < 0.5, -1.0, 1.0) * 2.0 ** (step * r.integers(-60, 61, n))).astype(dtype)
    low = (1 + r.integers(0, 256, n) * np.finfo(dtype).eps).astype(dtype)  # nextafter steps from 1.0
    extra = [odd, tiny, np.arange(n, dtype=dtype), np.arange(n, dtype=dtype)[::-1], top, low]
    return np.ascontiguousarray(np.concatenate([mixed_matrix(n, 16, seed).astype(dtype), np.stack(extra, 1)], 1))


def sort_np(Xd, *args, **kw):
    srt, nan_count = P.device_sort_columns(Xd, *args, **kw)
    assert srt.dtype == torch.float64 and nan_count.dtype == torch.int64 and srt.device == nan_count.device == DEV
    return srt.cpu().numpy(), nan_count.cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 63, 65, 257, 1000, T - 1, T, T + 1, 3 * T + 17])
def test_sorted_columns_equal_numpy(n, dtype):
    X = table(n, dtype, seed=n)
    srt, nan_count = sort_np(up(X))
    assert srt.shape == (X.shape[1], n)
    wide = X.astype(np.float64)  # float32: its exact widening
    for j in range(X.shape[1]):
        col, s = wide[:, j], srt[j]
        m = n - int(np.isnan(col).sum())
        assert nan_count[j] == n - m, f"column {j}"
        assert (s[:m][:-1] <= s[:m][1:]).all(), f"column {j} is not ascending"
        assert np.array_equal(np.sort(s[:m].view(np.int64)), np.sort(col[~np.isnan(col)].view(np.int64))), \
            f"column {j}: not the column's bit patterns"
        assert np.isnan(s[m:]).all(), f"column {j}: NaNs last"


@pytest.mark.parametrize("dtype", DTYPES)
def test_same_bits_for_any_geometry(dtype):
    Xd = up(mixed_matrix(3 * T + 17, 16, seed=3).astype(dtype))
    f = Xd.shape[1]
    ref, ref_nan = sort_np(Xd)
    fns = P._sort_fns()
    for tile in (fns["tile_step"](), T, fns["max_tile"]()):
        for j0, j1 in ((0, f), (0, 1), (5, 12)):
            srt, nan_count = sort_np(Xd, j0, j1, _tile=tile)
            assert np.array_equal(srt.view(np.int64), ref[j0:j1].view(np.int64)), f"tile {tile} columns {j0}:{j1}"
            assert np.array_equal(nan_count, ref_nan[j0:j1])
    reps = np.arange(40) % f  # more columns than one load tile of 32
    srt, nan_count = sort_np(Xd[:, torch.from_numpy(reps).to(DEV)].contiguous())
    assert np.array_equal(srt.view(np.int64), ref[reps].view(np.int64)) and np.array_equal(nan_count, ref_nan[reps])
    want = P.device_cuts(Xd, 16)
    for group in (1, 5, f):
        got = P.device_cuts(Xd, 16, _group=group)
        assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0])), f"group {group}"
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:])), f"group {group}"


@pytest.mark.parametrize("max_bins", [2, 16, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_both_routes_give_the_host_cuts(dtype, max_bins):
    for X in (mixed_matrix(3 * T + 17, 16, seed=3).astype(dtype), mixed_matrix(5000, 256, seed=4).astype(dtype)):
        want = host_tables(X.astype(np.float64), max_bins)
        for route in ("torch", None):
            got = P.device_cuts(up(X), max_bins, _sort=route)
            assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0])), f"route {route}"
            assert all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:])), f"route {route}"


def test_refusals():
    Xd = up(np.zeros((8, 3)))
    for bad in (dict(_tile=T + 1), dict(_tile=2 * P._sort_fns()["max_tile"]()), dict(j0=2, j1=2), dict(j0=0, j1=4)):
        with pytest.raises(ValueError):
            P.device_sort_columns(Xd, **bad)
    for X in (torch.zeros(8, 3, dtype=torch.float64), Xd.t()):  # on the host; not contiguous
        with pytest.raises(ValueError, match="contiguous"):
            P.device_sort_columns(X)
