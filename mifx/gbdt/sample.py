"""numpy twin of csrc/gbdt_sample.h: the draws of subsample, colsample_bytree and colsample_bylevel.

One integer-only, counter-based rule (uint64 wrap-around throughout):

    G = 0x9E3779B97F4A7C15, mix64 = murmur3's fmix64
    key(seed, round, site) = mix64(seed ^ mix64(round * G + site))

* rows (site 1): row i is in round t's sample iff (mix64(key + i * G) >> 32) < thr, thr = int(subsample * 2^32);
* features (site 2 per tree over all features, site 3 + d for level d over the tree's set): of the candidates c the
  k = max(1, int(rate * len(c))) with the smallest (mix64(key + j * G), j); a rate of 1.0 skips the draw.

The host learners use the C functions (mifx_gbdt_sample_rows, mifx_gbdt_level_mask in csrc/gbdt.cpp), the device
hashes the rows itself; the tests hold all three to these functions."""
from __future__ import annotations

import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
SITE_ROWS, SITE_TREE, SITE_LEVEL0 = 1, 2, 3
_M64 = (1 << 64) - 1


def mix64(z):
    """murmur3 fmix64 of a uint64 array (or scalar)."""
    z = np.asarray(z, np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(33)
        z *= np.uint64(0xFF51AFD7ED558CCD)
        z ^= z >> np.uint64(33)
        z *= np.uint64(0xC4CEB9FE1A85EC53)
        z ^= z >> np.uint64(33)
    return z


def key(seed: int, round: int, site: int) -> np.uint64:
    inner = int(mix64(np.uint64(((int(round) & _M64) * int(G) + int(site)) & _M64)))
    return np.uint64(int(mix64(np.uint64((int(seed) & _M64) ^ inner))))


def row_threshold(subsample: float) -> int:
    return int(float(subsample) * 4294967296.0)


def _hash(k: np.uint64, idx: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return mix64(k + idx.astype(np.uint64) * G)


def row_mask(seed: int, round: int, subsample: float, n: int) -> np.ndarray:
    """bool [n]: the rows of round `round`'s sample."""
    thr = row_threshold(subsample)
    if thr >= 1 << 32:
        return np.ones(n, bool)
    return (_hash(key(seed, round, SITE_ROWS), np.arange(n)) >> np.uint64(32)) < np.uint64(thr)


def choose_features(seed: int, round: int, site: int, rate: float, candidates) -> np.ndarray:
    """The chosen feature indices (ascending) among `candidates` (feature indices)."""
    c = np.asarray(candidates, np.int64)
    k = max(1, int(float(rate) * len(c)))
    h = _hash(key(seed, round, site), c)
    order = np.lexsort((c, h))  # by hash, ties by index
    return np.sort(c[order[:k]])


def level_mask(seed: int, round: int, f: int, max_depth: int, colsample_bytree: float = 1.0,
               colsample_bylevel: float = 1.0) -> np.ndarray:
    """uint8 [max_depth, f]: the features level d may split on."""
    tree = np.arange(f) if colsample_bytree >= 1.0 else choose_features(seed, round, SITE_TREE, colsample_bytree,
                                                                         np.arange(f))
    mask = np.zeros((max_depth, f), np.uint8)
    for d in range(max_depth):
        lv = tree if colsample_bylevel >= 1.0 else choose_features(seed, round, SITE_LEVEL0 + d, colsample_bylevel,
                                                                   tree)
        mask[d, lv] = 1
    return mask
