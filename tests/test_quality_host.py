"""`not gpu`: the host half of dynamorph_amd/quality.py -- the trustworthiness formula on given ranks against scikit-learn,
the argument checks (all made before anything touches a device), and the CONDITION of the fixtures test_gpu_quality.py uses:
the float64 rank interval of tests/helpers/rank_reference.py is a single number for nearly every (row, target) pair, so
that test's equality is not vacuous."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import rank_reference as RR  # noqa: E402
import umap_reference as UR  # noqa: E402


def truth_ranks(name, k):
    """Ranks in X of the k nearest neighbours in Y, both by float64 stable (d^2, index)."""
    return RR.rank_stable(RR.d2_of(name, "X"), RR.graph_float64(RR.d2_of(name, "Y"), k))


@pytest.mark.parametrize("name", RR.RANDOM)
def test_formula_equals_scikit_learn(name):
    sklearn_manifold = pytest.importorskip("sklearn.manifold")
    from dynamorph_amd import quality as Q
    X, Y = RR.fixture(name)
    ranks = truth_ranks(name, 15)
    for k in (5, 15):
        want = sklearn_manifold.trustworthiness(np.asarray(X, np.float64), np.asarray(Y, np.float64), n_neighbors=k)
        got = Q.score_from_ranks(ranks, k)
        assert isinstance(got, float) and abs(got - want) <= 1e-12, (name, k, got, want)
        assert abs(RR.trustworthiness_from_ranks(ranks, k) - want) <= 1e-12
        assert abs(UR.trustworthiness(X, Y, k) - want) <= 1e-12


def test_tuple_of_k_from_one_rank_matrix():
    from dynamorph_amd import quality as Q
    ranks = truth_ranks("randn_300x8", 15)
    both = Q.score_from_ranks(ranks, (5, 15))
    assert isinstance(both, tuple) and both == (Q.score_from_ranks(ranks, 5), Q.score_from_ranks(ranks, 15))
    assert both[0] == Q.score_from_ranks(truth_ranks("randn_300x8", 5), 5)      # the first k columns ARE the graph at k
    rec = Q.recall_from_ranks(ranks, (5, 15))
    assert rec == (float((ranks[:, :5] <= 5).mean()), float((ranks[:, :15] <= 15).mean()))
    # a shard of the rows: the penalties add up
    N = ranks.shape[0]
    parts = [1.0 - Q.score_from_ranks(ranks[lo:lo + 150], 15, n_samples=N) for lo in (0, 150)]
    assert abs((1.0 - sum(parts)) - both[1]) <= 1e-15


def test_argument_errors_before_any_device_call():
    from dynamorph_amd import quality as Q
    X, Y = RR.fixture("randn_300x8")
    tg = np.zeros((300, 15), np.int64)
    for fn in (Q.trustworthiness, Q.continuity):
        with pytest.raises(ValueError, match="n_samples / 2"):
            fn(X, Y, n_neighbors=150)
        with pytest.raises(ValueError, match="n_samples / 2"):
            fn(X, Y, n_neighbors=(5, 150))
        with pytest.raises(ValueError, match="rows"):
            fn(X, Y[:299])
        with pytest.raises(ValueError, match="is_wide"):
            fn(np.zeros((300, 16385), np.float32), Y)
    with pytest.raises(ValueError, match="n_samples / 2"):
        Q.embedding_quality(X, {"a": Y}, n_neighbors=150)
    with pytest.raises(ValueError, match="rows"):
        Q.embedding_quality(X, {"a": Y, "b": Y[:10]})
    with pytest.raises(ValueError, match="is_wide"):
        Q.neighbor_ranks(np.zeros((300, 16385), np.float32), tg)
    for bad in (300, -1):
        t = tg.copy()
        t[7, 3] = bad
        with pytest.raises(ValueError, match="outside 0 .. 299"):
            Q.neighbor_ranks(X, t)
    with pytest.raises(ValueError, match="1 .. 256"):
        Q.neighbor_ranks(X, np.zeros((300, 257), np.int64))
    with pytest.raises(ValueError, match=r"\(300, c\)"):
        Q.neighbor_ranks(X, tg[:299])
    with pytest.raises(ValueError, match="rows="):
        Q.neighbor_ranks(X, tg[:10], rows=(295, 10))
    with pytest.raises(ValueError, match="cap"):
        Q.neighbor_ranks(X, tg, cap=0)


@pytest.mark.parametrize("name", RR.RANDOM)
def test_fixtures_meet_their_condition(name):
    """Share of (row, target) pairs with lo == hi at tau = 1e-6, targets from Y's float64 graph at 15 neighbours: computed on
    the CPU as 0.9992 (blobs_700x64), 0.9901 (randn_384x4096), 0.9996 (randn_300x8)."""
    d2 = RR.d2_of(name, "X")
    lo, hi = RR.rank_interval(d2, RR.graph_float64(RR.d2_of(name, "Y"), 15), RR.TAU)
    share = float((lo == hi).mean())
    print(f"{name}: {share:.4f} of the pairs have lo == hi")
    assert (lo <= hi).all() and share >= 0.95


def test_lattice_is_what_it_says():
    X, Y = RR.fixture("lattice_400x6")
    d2 = RR.d2_of("lattice_400x6", "X")
    assert (d2[np.isfinite(d2)] == np.round(d2[np.isfinite(d2)])).all()          # integers: the exact form is exact
    assert len(np.unique(np.round(X @ X.T))) > 1 and len(np.unique(X, axis=0)) < 400      # duplicate rows exist
    lo, hi = RR.rank_interval(d2, RR.graph_float64(d2, 15))
    assert (hi > lo).mean() > 0.5                                                # ties are everywhere
