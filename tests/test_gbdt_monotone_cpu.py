"""monotone_constraints on the host learners (csrc/gbdt.cpp, the rule of csrc/gbdt_split.h): the first tree against a
brute-force float64 transcription of the rule, the promise itself, the unconstrained models unchanged, validation."""
import hashlib

import numpy as np
import pytest

import gbdt_monotone_cases as M
from mifx.gbdt import XGBClassifier, XGBRegressor

LOSSGUIDE = dict(grow_policy="lossguide", max_leaves=8, max_depth=0)


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_first_tree_equals_the_plain_reference(depth):
    X, y = M.table()
    m = XGBRegressor(n_estimators=1, max_depth=depth, max_bins=32, base_score=0.0, monotone_constraints=M.MONO).fit(X, y)
    seen = {"clamped": 0, "rejected": 0}
    ref = M.ref_tree(X, (0.0 - y).astype(np.float32).astype(np.float64), np.ones(len(y)), m._cuts, M.MONO, depth, seen)
    print(f"depth {depth}: {len(m._trees[0][0])} nodes, reference saw {seen}")
    assert seen["rejected"] > 0 and (depth == 1 or seen["clamped"] > 0)
    M.assert_tree_is(m._trees[0], ref)


@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("policy", [dict(max_depth=4), LOSSGUIDE])
@pytest.mark.parametrize("cls", [XGBRegressor, XGBClassifier])
def test_the_promise(cls, policy, fixed):
    X, y = M.table()
    y = y if cls is XGBRegressor else (y > np.median(y)).astype(int)
    m = cls(n_estimators=20, monotone_constraints={0: 1, 1: -1}, fixed_point=fixed, **policy).fit(X, y)
    M.assert_promise(m._margin, X)


# sha256 over the six arrays of every tree of XGBRegressor(n_estimators=3, max_depth=4, <key>).fit(*table()), taken from
# the learners as they were before monotone_constraints existed
# (key: lossguide; the table's sums are exact, so the double and the fixed-point learner grow the same trees)
UNCONSTRAINED = {False: "836724fc44e273bdfa1435ca4104d72227e83ac8abc336fc9c9923cab1f7cf6d",
                 True: "c802b5a76dacecf6002843258cb733eafe1f0113a3f126cc187d05190e8142c6"}


@pytest.mark.parametrize("mono", [{}, dict(monotone_constraints=None), dict(monotone_constraints=[0, 0, 0, 0]),
                                  dict(monotone_constraints={2: 0})], ids=["absent", "none", "zeros", "dict"])
@pytest.mark.parametrize("lossguide", [False, True])
@pytest.mark.parametrize("fixed", [False, True])
def test_unconstrained_trees_are_unchanged(fixed, lossguide, mono):
    X, y = M.table()
    kw = dict(LOSSGUIDE if lossguide else dict(max_depth=4), n_estimators=3, fixed_point=fixed)
    m = XGBRegressor(**kw, **mono).fit(X, y)
    digest = hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for t in m._trees for a in t)).hexdigest()
    assert digest == UNCONSTRAINED[lossguide]


@pytest.mark.parametrize("bad", [[1, 0, 0], [1, 0, 0, 0, 0], [2, 0, 0, 0], [1.0, 0, 0, 0], [True, 0, 0, 0], "1000",
                                 {4: 1}, {0: -2}, {"a": 1}, [[1, 0, 0, 0]]])
def test_bad_constraints_raise_before_the_first_round(bad):
    X, y = M.table(40)
    m = XGBRegressor(n_estimators=2)
    m.monotone_constraints = bad  # (as set_params would: fit validates again)
    with pytest.raises(ValueError, match="monotone"):
        m.fit(X, y)
    assert m._trees == []
    if bad not in ([1, 0, 0], [1, 0, 0, 0, 0], {4: 1}):  # a wrong length needs the table; anything else fails at once
        with pytest.raises(ValueError, match="monotone"):
            XGBRegressor(monotone_constraints=bad)


def test_quantile_objectives_refuse_constraints():
    X, y = M.table(40)
    with pytest.raises(ValueError, match="monotone_constraints with reg:absoluteerror"):
        XGBRegressor(objective="reg:absoluteerror", monotone_constraints=M.MONO).fit(X, y)
