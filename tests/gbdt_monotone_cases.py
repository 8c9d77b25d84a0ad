"""Shared by tests/test_gbdt_monotone_cpu.py and tests/test_gbdt_monotone_gpu.py: the table, a brute-force float64
grower that transcribes the monotone_constraints rule of csrc/gbdt_split.h, and the sweep that checks the promise."""
import numpy as np

MONO = (1, -1, 0, 0)
INF = float("inf")


def table(n=300, seed=5):
    """[n, 4] with ~10 % NaN; y rises and falls in feature 0 (so candidates are rejected and weights clamped), falls in
    feature 1, and is a multiple of 1/64: with base_score 0 the first tree's sums are exact in every learner."""
    r = np.random.default_rng(seed)
    X = r.normal(size=(n, 4))
    y = np.round(64 * (np.sin(3 * X[:, 0]) + 0.3 * X[:, 0] - 0.5 * X[:, 1] + X[:, 2] * X[:, 3])) / 64
    X[r.random(X.shape) < 0.1] = np.nan
    return X, y


def _clamp(w, lo, hi):
    return lo if w < lo else (hi if w > hi else w)


def _score(G, H, lam, w):
    return -(2.0 * G * w + (H + lam) * w * w)


def ref_tree(X, g, h, cuts, mono, depth, seen, lo=-INF, hi=INF, lam=1.0, gamma=0.0, mcw=1.0, eta=0.3):
    """The constrained tree by recursion: every cut and both missing directions are candidates, in (feature, cut,
    direction) order; a leaf is {"value"}, a split {"feature", "thr", "dl", "left", "right"}. `seen` counts the clamped
    candidate weights and the rejected candidates."""
    G, H = float(g.sum()), float(h.sum())
    w = _clamp(-G / (H + lam), lo, hi)
    best, best_gain = None, 0.0
    for j in range(X.shape[1] if depth > 0 and len(g) >= 2 else 0):
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
                wl, wr = _clamp(-GL / (HL + lam), lo, hi), _clamp(-GR / (HR + lam), lo, hi)
                seen["clamped"] += wl != -GL / (HL + lam) or wr != -GR / (HR + lam)
                if (mono[j] > 0 and wl > wr) or (mono[j] < 0 and wl < wr):
                    seen["rejected"] += 1
                    continue
                gain = 0.5 * (_score(GL, HL, lam, wl) + _score(GR, HR, lam, wr) - _score(G, H, lam, w)) - gamma
                if gain > fgain:
                    fbest, fgain = (j, cut, dl, L, wl, wr), gain
        if fbest is not None and fgain > best_gain + 1e-12 * abs(best_gain):
            best, best_gain = fbest, fgain
    if best is None or best_gain <= 1e-6:
        return {"value": eta * w}
    j, cut, dl, L, wl, wr = best
    mid = 0.5 * (wl + wr)
    bl, br = ((lo, hi), (lo, hi)) if mono[j] == 0 else ((lo, mid), (mid, hi)) if mono[j] > 0 else ((mid, hi), (lo, mid))
    kw = dict(lam=lam, gamma=gamma, mcw=mcw, eta=eta)
    return {"feature": j, "thr": cut, "dl": dl,
            "left": ref_tree(X[L], g[L], h[L], cuts, mono, depth - 1, seen, *bl, **kw),
            "right": ref_tree(X[~L], g[~L], h[~L], cuts, mono, depth - 1, seen, *br, **kw)}


def assert_tree_is(tree, ref, k=0):
    """A model's tree (feature, thr, default_left, left, right, value), from node k, against ref_tree's: exactly."""
    fe, thr, dl, le, ri, val = tree
    if "value" in ref:
        assert fe[k] < 0 and val[k] == ref["value"], f"node {k}: {fe[k]} {val[k]!r} against the leaf {ref['value']!r}"
        return
    assert (fe[k], thr[k], bool(dl[k])) == (ref["feature"], ref["thr"], ref["dl"]), f"node {k}"
    assert_tree_is(tree, ref["left"], le[k])
    assert_tree_is(tree, ref["right"], ri[k])


def assert_promise(margin_of, X, to_input=lambda a: a):
    """Feature 0 swept upwards never lowers the margin and feature 1 never raises it, the other features fixed at the
    values of several rows (NaN among them): exact comparisons."""
    grid = np.linspace(-3.0, 3.0, 97)
    assert np.isnan(X[:12]).any()
    for j, sign in ((0, 1.0), (1, -1.0)):
        S = np.repeat(X[:12], len(grid), axis=0)
        S[:, j] = np.tile(grid, 12)
        step = np.diff(np.asarray(margin_of(to_input(S))).reshape(12, len(grid)), axis=1) * sign
        assert (step >= 0).all(), f"feature {j}: the margin moves the wrong way by {step.min()}"
        assert (step > 0).any(), f"feature {j} is never used"
