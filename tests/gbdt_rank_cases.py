"""Shared cases of the XGBRanker gradient tests and a plain numpy float64 reference: a direct O(m^2) transcription of
the rule in csrc/gbdt_rank.h (every row walks its group's rows in rank order), independent of the code under test."""
import functools

import numpy as np

CAP = 4096  # mifx_gbdt_rank_max_group(): the GPU test checks that the library says the same
OBJECTIVES = ("rank:pairwise", "rank:ndcg")


def reference(objective, margin, y, gptr, topk=0):
    """(g, h, Ag, Ah) in float64: the sums of section "A row's sums" and the sums of their terms' magnitudes."""
    n, G, sizes = len(y), len(gptr) - 1, np.diff(gptr)
    gid = np.repeat(np.arange(G), sizes)
    D = 1.0 / np.log2(np.arange(sizes.max() + 1) + 2.0)
    P = np.concatenate([[0.0], np.cumsum(D[:-1])])
    bits = margin.view(np.uint64)
    key = np.where(bits >> np.uint64(63), ~bits, bits | np.uint64(1 << 63))
    order = np.lexsort((np.arange(n), ~key, gid))  # group, then key descending, then the lower row
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) - gptr[gid]
    label, gain = y.astype(np.int64), np.exp2(y) - 1.0
    idcg = np.zeros(G)
    for q in range(G):
        cnt, above = np.bincount(label[gptr[q]:gptr[q + 1]], minlength=32), 0
        for l in range(31, 0, -1):
            idcg[q] += gain.dtype.type(2.0 ** l - 1.0) * (P[above + cnt[l]] - P[above])
            above += cnt[l]
    g, h, Ag, Ah = (np.zeros(n) for _ in range(4))
    with np.errstate(over="ignore"):
        for r in range(sizes.max()):  # every row of a group longer than r meets the group's row of rank r
            i = np.flatnonzero(sizes[gid] > r)
            j = order[gptr[gid[i]] + r]
            pair = label[i] != label[j]
            if topk > 0:
                pair &= np.minimum(rank[i], r) < topk
            hi = label[i] > label[j]
            rho = 1.0 / (1.0 + np.exp(np.where(hi, margin[i] - margin[j], margin[j] - margin[i])))
            delta = np.ones(len(i))
            if objective == "rank:ndcg":
                z = idcg[gid[i]]
                delta = np.where(z > 0, np.abs((gain[i] - gain[j]) * (D[rank[i]] - D[r])) / np.where(z > 0, z, 1.0), 0.0)
            lam = np.where(pair, rho * delta, 0.0)
            eta = np.where(pair, 2.0 * np.maximum(rho * (1.0 - rho), 1e-16) * delta, 0.0)
            g[i] = np.where(hi, g[i] - lam, g[i] + lam)
            h[i] += eta
            Ag[i] += lam
            Ah[i] += eta
    return g, h, Ag, Ah


def within(got, want, A):
    """The derived bound: one float32 ulp for the cast of a double sum that may straddle a rounding boundary, plus
    2^-40 A for the terms' few double ulps (exp) and the order-fixed sum's m 2^-52 A (m <= 4096 = 2^12)."""
    want32 = want.astype(np.float32)
    bound = np.spacing(np.abs(want32)).astype(np.float64) + 2.0 ** -40 * A
    return np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= bound


@functools.lru_cache(maxsize=None)
def table():
    """(margin, y, gptr): one table of groups at every size where a route can go wrong -- 1, 2, the wave route's last
    sizes 63 and 64, the workgroup route's first 65, 257 (more than one row per thread), the size-class boundary
    512 / 513, CAP - 1 and CAP -- in an order that makes the work list permute them, followed by the special groups on
    both routes: all labels equal, all labels 0, tied margins with a +0.0 / -0.0 pair, margins 800 apart."""
    rng = np.random.default_rng(5)
    sizes = [65, 1, CAP, 2, 63, 513, 257, 64, CAP - 1, 512]
    margin = [np.round(rng.normal(size=m), 1) for m in sizes]  # one decimal: many ties
    y = [rng.integers(0, 5, m).astype(np.float64) for m in sizes]
    y[4][:2] = 31.0  # the largest gain
    for m in (5, 70):
        margin += [rng.normal(size=m), rng.normal(size=m)]
        y += [np.full(m, 2.0), np.zeros(m)]  # no pair; IDCG 0
        z = np.round(rng.normal(size=m))
        z[z == 0.0] = np.where(np.arange((z == 0.0).sum()) % 2, -0.0, 0.0)
        z[1], z[3] = 0.0, -0.0
        margin += [z, rng.choice([-800.0, 0.0, 800.0], m) + rng.normal(size=m)]
        y += [rng.integers(0, 4, m).astype(np.float64), rng.integers(0, 3, m).astype(np.float64)]
    gptr = np.concatenate([[0], np.cumsum([len(a) for a in y])]).astype(np.int64)
    return np.concatenate(margin), np.concatenate(y), gptr


@functools.lru_cache(maxsize=None)
def table_reference(objective, topk):
    return reference(objective, *table(), topk)


@functools.lru_cache(maxsize=None)
def flat_reference(objective):
    """float32 (g, h) of the table with every margin 0.0 (a fit's first round): exp(0) = 1, so exact for everyone."""
    margin, y, gptr = table()
    return tuple(a.astype(np.float32) for a in reference(objective, np.zeros_like(margin), y, gptr)[:2])


def planted(seed=3):
    """(X, y, qid): 40 groups of 5 to 40 rows, the label a step function of feature 0, no noise."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(5, 41, 40)
    X = rng.normal(size=(int(sizes.sum()), 6))
    return X, np.digitize(X[:, 0], [-1.0, -0.3, 0.3, 1.0]).astype(np.float64), np.repeat(np.arange(40), sizes)
