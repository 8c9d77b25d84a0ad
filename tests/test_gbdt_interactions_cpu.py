"""predict_interactions on the host (csrc/gbdt.cpp, mifx_gbdt_interactions) against a brute-force enumeration of the
Shapley interaction index over all subsets of the path-dependent game (tree_value), then the structure of the matrix
on a depth-12 forest and the errors it shares with predict_contribs."""
import itertools
import math
import pickle

import numpy as np
import pytest

from test_gbdt_contribs_cpu import deep, leaf_scale, models, probe_rows, tree_value  # noqa: F401 (two fixtures)


def interaction_oracle(trees, covers, X, f, phi):
    """[n, f + 1, f + 1] from the definition: the pairwise index over every S without i and j, the diagonal from the
    contributions phi [n, f + 1], the bias in (f, f)."""
    sets = [frozenset(s) for r in range(f + 1) for s in itertools.combinations(range(f), r)]
    v = {s: sum(tree_value(t, c, X, s) for t, c in zip(trees, covers)) + np.zeros(len(X)) for s in sets}
    out = np.zeros((len(X), f + 1, f + 1))
    for i, j in itertools.permutations(range(f), 2):
        for s in sets:
            if i not in s and j not in s:
                wt = math.factorial(len(s)) * math.factorial(f - len(s) - 2) / (2 * math.factorial(f - 1))
                out[:, i, j] += wt * (v[s | {i, j}] - v[s | {i}] - v[s | {j}] + v[s])
    for i in range(f):
        out[:, i, i] = phi[:, i] - out[:, i].sum(-1)
    out[:, f, f] = phi[:, f]
    return out


@pytest.mark.parametrize("name", ["f1", "f3_depth6_weighted_subsampled", "f6_depth8_binary", "three_classes",
                                  "early_stopped"])
def test_interactions_equal_brute_force(models, name):
    m, X = models[name]
    P = probe_rows(X)
    f, K, limit = X.shape[1], m._num_class(), m._tree_limit()
    got = m.predict_interactions(P)
    assert got.shape == ((len(P), f + 1, f + 1) if K == 1 else (len(P), K, f + 1, f + 1)) and got.dtype == np.float64
    got = got.reshape(len(P), K, f + 1, f + 1)
    phi = m.predict_contribs(P).reshape(len(P), K, f + 1)
    for k in range(K):
        trees = m._trees[k:limit:K]
        want = interaction_oracle(trees, [s[1] for s in m._node_stats[k:limit:K]], P, f, phi[:, k])
        S = leaf_scale(trees)
        err = np.abs(got[:, k] - want).max()
        print(f"{name} class {k}: max |Phi - oracle| = {err:.3g} = {err / S:.3g} S (S = {S:.4g}, bound 1e-12 S)")
        assert err <= 1e-12 * S
        assert f == 1 or np.abs(want[:, 0, 1:f]).max() > 0  # the case has pairs that interact


def test_structure_on_a_depth_12_forest(deep):
    m, X = deep
    P = probe_rows(X, 100)
    S, f = leaf_scale(m._trees), X.shape[1]
    m.n_jobs = 1
    phi, M = m.predict_contribs(P), m.predict_interactions(P)
    m.n_jobs = 4
    assert np.array_equal(M.view(np.uint64), m.predict_interactions(P).view(np.uint64)), "n_jobs 1 and 4"
    m.n_jobs = None
    rows, sym = np.abs(M.sum(-1) - phi).max(), np.abs(M - M.transpose(0, 2, 1)).max()
    print(f"depth 12: max |row sums - phi| = {rows / S:.3g} S, max |Phi - Phi^T| = {sym / S:.3g} S (bound 1e-12 S)")
    assert rows <= 1e-12 * S and sym <= 1e-12 * S
    assert np.array_equal(M[:, f, f], phi[:, f])
    assert (M[:, f, :f] == 0).all() and (M[:, :f, f] == 0).all()
    assert (M[:, 10] == 0).all() and (M[:, :, 10] == 0).all() and np.abs(M[:, 0, 1]).max() > 0
    P32 = np.where(np.isnan(P), 0.5, P).astype(np.float32)  # a float32 table means its exact widening
    assert np.array_equal(m.predict_interactions(P32), m.predict_interactions(P32.astype(np.float64)))


@pytest.mark.parametrize("case", ["zero_cover", "no_statistics", "features", "one_row"])
def test_errors_of_predict_contribs_are_raised_here_too(models, case):
    src, X = models["f3_depth6_weighted_subsampled"]
    m = pickle.loads(pickle.dumps(src))
    if case == "zero_cover":
        m._node_stats[1][1][int(m._trees[1][3][0])] = 0.0
    elif case == "no_statistics":
        del m.__dict__["_node_stats"]
    with pytest.raises(ValueError, match={"zero_cover": "cover", "no_statistics": "refit"}.get(case, "features")):
        m.predict_interactions(X[:, :2] if case == "features" else X[0] if case == "one_row" else X)
