"""interaction_constraints and colsample_bynode on the host learners (csrc/gbdt.cpp, the rule of csrc/gbdt_nodeset.h):
the first tree against a plain float64 grower that restricts every node to `drawn & A(S)` with Python sets, the promise
on every path of a boosted model, the numpy twin of the draw against the C rule, the defaults, validation."""
import ctypes

import numpy as np
import pytest

import gbdt_monotone_cases as M
from mifx.gbdt import XGBRegressor, sample, xgb

LOSSGUIDE = dict(grow_policy="lossguide", max_leaves=8, max_depth=0)
OVERLAP = [[0, 2], [1, 2]]  # overlapping groups; feature 3 is in no group
SINGLE = [[3], [0, 1, 2]]   # a group of one


def admissible(S, groups, f):
    """A(S): every feature at the root or without groups, else S and the groups that hold all of S."""
    if not S or groups is None:
        return set(range(f))
    return set(S).union(*[g for g in groups if set(S) <= set(g)])


def best_split(X, g, h, cuts, feats, mono, lo, hi, lam=1.0, mcw=1.0):
    """The node's best candidate among `feats`, in (feature, cut, direction) order with the learners' tie rules:
    (gain, feature, cut, default_left, left rows, wl, wr) or None. mono None: the unconstrained gain."""
    G, H = float(g.sum()), float(h.sum())
    w = M._clamp(-G / (H + lam), lo, hi)
    best, best_gain = None, 0.0
    for j in sorted(feats):
        miss, fbest, fgain = np.isnan(X[:, j]), None, 0.0
        for cut in cuts[j]:
            for dl in (False, True):
                if dl and not miss.any():
                    break
                L = (X[:, j] < cut) | (miss & dl)
                GL, HL = float(g[L].sum()), float(h[L].sum())
                GR, HR = G - GL, H - HL
                if HL < mcw or HR < mcw:
                    continue
                wl, wr = M._clamp(-GL / (HL + lam), lo, hi), M._clamp(-GR / (HR + lam), lo, hi)
                if mono is None:
                    gain = 0.5 * (GL * GL / (HL + lam) + GR * GR / (HR + lam) - G * G / (H + lam))
                elif (mono[j] > 0 and wl > wr) or (mono[j] < 0 and wl < wr):
                    continue
                else:
                    gain = 0.5 * (M._score(GL, HL, lam, wl) + M._score(GR, HR, lam, wr) - M._score(G, H, lam, w))
                if gain > fgain:
                    fbest, fgain = (j, cut, dl, L, wl, wr), gain
        if fbest is not None and fgain > best_gain + 1e-12 * abs(best_gain):
            best, best_gain = fbest, fgain
    return (best_gain,) + best if best is not None and best_gain > 1e-6 else None


def ref_grow(X, y, cuts, groups, rate, mono, depth, leaves, eta=0.3, lam=1.0):
    """The first tree (base_score 0) in the learners' numbering, as a list of (feature, cut, default_left, left, right)
    or (-1, value). depth None: no limit; leaves 0: depth-wise (the open node with the lowest index is split next, which
    is level order), else best first (largest gain, ties to the lowest index) up to `leaves` leaves."""
    g, h, f = (0.0 - y).astype(np.float32).astype(np.float64), np.ones(len(y)), X.shape[1]
    nodes = []

    def add(rows, S, d, lo, hi):
        k, cand = len(nodes), None
        if (depth is None or d < depth) and len(rows) >= 2:
            feats = set(sample.node_mask(0, 0, k, range(f), rate).tolist()) & admissible(S, groups, f)
            cand = best_split(X[rows], g[rows], h[rows], cuts, feats, mono, lo, hi)
        nodes.append(dict(rows=rows, S=S, d=d, lo=lo, hi=hi, cand=cand, out=None))

    add(np.arange(len(y)), frozenset(), 0, -M.INF, M.INF)
    n_leaves = 1
    while not leaves or n_leaves < leaves:
        open_ = [k for k, nd in enumerate(nodes) if nd["cand"] is not None and nd["out"] is None]
        if not open_:
            break
        k = max(open_, key=lambda i: (nodes[i]["cand"][0], -i)) if leaves else open_[0]
        nd = nodes[k]
        _, j, cut, dl, L, wl, wr = nd["cand"]
        lo, hi, mid = nd["lo"], nd["hi"], 0.5 * (wl + wr)
        dirn = 0 if mono is None else mono[j]
        bl, br = ((lo, hi), (lo, hi)) if dirn == 0 else ((lo, mid), (mid, hi)) if dirn > 0 else ((mid, hi), (lo, mid))
        nd["out"] = (j, cut, dl, len(nodes), len(nodes) + 1)
        add(nd["rows"][L], nd["S"] | {j}, nd["d"] + 1, *bl)
        add(nd["rows"][~L], nd["S"] | {j}, nd["d"] + 1, *br)
        n_leaves += 1
    for nd in nodes:
        if nd["out"] is None:
            G, H = float(g[nd["rows"]].sum()), float(h[nd["rows"]].sum())
            nd["out"] = (-1, -eta * G / (H + lam) if mono is None else eta * M._clamp(-G / (H + lam), nd["lo"], nd["hi"]))
    return [nd["out"] for nd in nodes]


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("policy", [dict(max_depth=4), LOSSGUIDE], ids=["depthwise", "lossguide"])
@pytest.mark.parametrize("mono", [None, M.MONO])
@pytest.mark.parametrize("groups,rate", [(OVERLAP, 1.0), (OVERLAP, 0.5), (SINGLE, 1.0), (SINGLE, 0.5), (None, 0.5)])
def test_first_tree_equals_the_plain_reference(groups, rate, mono, policy, fixed):
    X, y = M.table()
    m = XGBRegressor(n_estimators=1, max_bins=32, base_score=0.0, fixed_point=fixed, interaction_constraints=groups,
                     colsample_bynode=rate, monotone_constraints=mono, **policy).fit(X, y)
    lg = "grow_policy" in policy
    ref = ref_grow(X, y, m._cuts, groups, rate, mono, None if lg else 4, 8 if lg else 0)
    fe, thr, dl, le, ri, val = m._trees[0]
    assert len(fe) == len(ref) and len(ref) > 3
    for k, out in enumerate(ref):
        got = (fe[k], val[k]) if fe[k] < 0 else (fe[k], thr[k], bool(dl[k]), le[k], ri[k])
        assert got == out, f"node {k}: {got} against {out}"


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("policy", [dict(max_depth=4), LOSSGUIDE], ids=["depthwise", "lossguide"])
@pytest.mark.parametrize("groups", [OVERLAP, SINGLE])
def test_every_path_keeps_the_promise(groups, policy, fixed):
    X, y = M.table()
    m = XGBRegressor(n_estimators=10, fixed_point=fixed, interaction_constraints=groups, colsample_bynode=0.75,
                     subsample=0.8, **policy).fit(X, y)
    deepest = 0
    for fe, _, _, le, ri, _ in m._trees:
        todo = [(0, frozenset())]
        while todo:
            k, S = todo.pop()
            if fe[k] >= 0:
                assert fe[k] in admissible(S, groups, 4), f"feature {fe[k]} below {sorted(S)}"
                todo += [(le[k], S | {fe[k]}), (ri[k], S | {fe[k]})]
                deepest = max(deepest, len(S) + 1)
    assert deepest >= 2


@pytest.mark.parametrize("f", [1, 5, 64, 65, 130])
@pytest.mark.parametrize("rate", [0.5, 0.1])
def test_node_mask_is_the_c_rule(f, rate):
    level = np.array([j for j in range(f) if j % 3 != 1 or f == 1])
    cand, out = np.zeros(f, np.uint8), np.empty(f, np.uint8)
    cand[level] = 1
    for node in (0, 1, 77):
        k = xgb._lib().mifx_gbdt_sample_features(9, 4, ctypes.c_uint64(2 ** 32 + node), rate, xgb._p(cand, xgb._U8), f,
                                                 xgb._p(out, xgb._U8))
        got = sample.node_mask(9, 4, node, level, rate)
        assert k == len(got) == max(1, int(rate * len(level))) and np.array_equal(got, np.flatnonzero(out))
        assert np.array_equal(sample.node_mask(9, 4, node, level, 1.0), level)


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("policy", [dict(max_depth=4), LOSSGUIDE], ids=["depthwise", "lossguide"])
def test_defaults_change_no_bit(policy, fixed):
    X, y = M.table()
    kw = dict(n_estimators=3, fixed_point=fixed, subsample=0.8, colsample_bytree=0.75, **policy)
    a = XGBRegressor(**kw).fit(X, y)
    for off in (dict(interaction_constraints=None, colsample_bynode=1.0), dict(interaction_constraints=[])):
        b = XGBRegressor(**kw, **off).fit(X, y)
        assert all(u.tobytes() == v.tobytes() for s, t in zip(a._trees, b._trees) for u, v in zip(s, t))
    del a.__dict__["interaction_constraints"], a.__dict__["colsample_bynode"]  # a model pickled before they existed
    assert a._nodeset(4) is None


@pytest.mark.parametrize("bad", [[[0, 4]], [[0, -1]], [[True, 1]], [["0", "1"]], "[[0, 1]]", [3]])
def test_bad_groups_raise_before_the_first_round(bad):
    X, y = M.table(40)
    m = XGBRegressor(n_estimators=2)
    m.interaction_constraints = bad  # (as set_params would: fit validates again)
    with pytest.raises(ValueError, match="interaction_constraints"):
        m.fit(X, y)
    assert m._trees == []
    if bad != [[0, 4]]:  # an index past the table needs the table; anything else fails at once
        with pytest.raises(ValueError, match="interaction_constraints"):
            XGBRegressor(interaction_constraints=bad)
    with pytest.raises(ValueError, match="colsample_bynode"):
        XGBRegressor(colsample_bynode=0.0)
