"""`gpu`: neighbour ranks, trustworthiness and continuity (csrc/knn.hip dm_knn_ranks, dynamorph_amd/quality.py) against the
float64 truth of tests/helpers/rank_reference.py.  Criterion: every rank lies in the float64 interval [lo, hi] at tau = 1e-6
and equals it where lo == hi (0.99 of the pairs and more, test_quality_host.py); the rank of knn_graph's own column c is
c + 1 exactly; on the lattice, where the exact form is exact, the ranks are the stable (d^2, index) ranks with every tie.
The shapes are the smallest at which each part can go wrong: M no multiple of the 128-wide tile, three panels with a partial
last one, F = 7 (no 16-byte rows), 8, 64 and 4096 (sixteen 256-feature slabs), c = 1 and c = 256, and more rows on the
fallback list than one round takes."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import knn_reference as KR  # noqa: E402
import rank_reference as RR  # noqa: E402
import umap_reference as UR  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def gpu_graph(P, k):
    from dynamorph_amd import knn as K
    return K.knn_graph(dev(P), k, include_self=False)[0]


_sliced = {}


def case(name, features=None):
    """(X, Y, float64 d^2 of X, float64 d^2 of Y); features: the first columns of X only."""
    X, Y = RR.fixture(name)
    if features is None:
        return X, Y, RR.d2_of(name, "X"), RR.d2_of(name, "Y")
    if (name, features) not in _sliced:
        _sliced[name, features] = KR.d2_float64(X[:, :features], X[:, :features], self_r0=0)
    return X[:, :features], Y, _sliced[name, features], RR.d2_of(name, "Y")


# (fixture, c, chunk_rows, features)
CRITERION = [
    ("blobs_700x64", 15, 2048, None),
    ("randn_384x4096", 15, 2048, None),
    ("randn_300x8", 15, 128, None),
    ("randn_300x8", 1, 2048, None),
    ("randn_300x8", 256, 2048, None),
    ("randn_300x8", 15, 2048, 7),
]


@pytest.mark.parametrize("name,c,chunk_rows,features", CRITERION)
def test_criterion(name, c, chunk_rows, features):
    from dynamorph_amd import quality as Q
    X, _, d2x, d2y = case(name, features)
    x = dev(X)
    tg = RR.graph_float64(d2y, c)                                   # the c nearest in the embedding
    ranks, namb, nredo = Q.neighbor_ranks(x, tg, chunk_rows=chunk_rows, return_counts=True)
    lo, hi = RR.rank_interval(d2x, tg)
    print(f"{name} c={c} F={X.shape[1]}: {namb / len(X):.1f} columns per row decided one by one, {nredo} rows redone, "
          f"{(lo == hi).mean():.4f} of the pairs have lo == hi")
    assert ranks.dtype == np.int32 and ranks.shape == tg.shape
    bad = np.argwhere((ranks < lo) | (ranks > hi))
    assert not len(bad), f"{len(bad)} ranks outside [lo, hi], e.g. {[(i, t, ranks[i, t], lo[i, t], hi[i, t]) for i, t in bad[:5]]}"
    own = gpu_graph(X, min(c, 200))                                 # its own graph: column t has rank t + 1
    r_own = Q.neighbor_ranks(x, own, chunk_rows=chunk_rows)
    assert np.array_equal(r_own, np.broadcast_to(np.arange(1, own.shape[1] + 1, dtype=np.int32), own.shape))


def test_ties_on_the_lattice():
    from dynamorph_amd import quality as Q
    X, _, d2x, d2y = case("lattice_400x6")
    N = len(X)
    me = np.arange(N)[:, None]
    gy = RR.graph_float64(d2y, 15)
    # neighbours in the embedding, neighbours in X (a duplicate row at distance 0 among them), the row itself, a repeat
    tg = np.concatenate([gy, RR.graph_float64(d2x, 15), me, gy[:, :1]], axis=1)
    assert (d2x.min(1) == 0).sum() >= 2                             # duplicate rows exist
    ranks, namb, nredo = Q.neighbor_ranks(dev(X), tg, return_counts=True)
    print(f"lattice: {namb / N:.1f} columns per row decided one by one, {nredo} rows redone")
    assert np.array_equal(ranks, RR.rank_stable(d2x, tg))
    assert (ranks[:, 30] == 0).all() and np.array_equal(ranks[:, 31], ranks[:, 0])
    assert np.array_equal(ranks[:, 15:30], np.broadcast_to(np.arange(1, 16), (N, 15)))
    forced = Q.neighbor_ranks(dev(X), tg, cap=1)                    # every row through the fallback: the same ties
    assert np.array_equal(forced, ranks)


def test_one_answer_by_every_path():
    from dynamorph_amd import quality as Q
    X, _, d2x, d2y = case("blobs_700x64")
    x = dev(X)
    tg = RR.graph_float64(d2y, 15)
    base, namb, nredo = Q.neighbor_ranks(x, tg, return_counts=True)
    assert nredo == 0 and namb >= 15 * 700                           # (a target is never decided against itself by the filter)
    for cr in (64, 128, 2048):
        assert np.array_equal(Q.neighbor_ranks(x, tg, chunk_rows=cr), base), cr
    halves = [Q.neighbor_ranks(x, tg[r0:r0 + 350], rows=(r0, 350)) for r0 in (0, 350)]
    assert np.array_equal(np.concatenate(halves), base)
    assert np.array_equal(Q.neighbor_ranks(x, tg, shift=None), base)
    forced, namb4, nredo4 = Q.neighbor_ranks(x, tg, cap=4, return_counts=True)
    assert nredo4 == 700 and namb4 == 0                             # 15 targets > 4 entries: three fallback rounds of 256 rows
    assert np.array_equal(forced, base)
    forced = Q.neighbor_ranks(x, tg, cap=4, chunk_rows=300)         # two rounds, the second partial, per panel
    assert np.array_equal(forced, base)


def test_offset_data_without_the_shift_is_redone_and_equal():
    from dynamorph_amd import quality as Q
    X = KR.fixture("offset_257x64")
    x = dev(X)
    own = gpu_graph(X, 15)
    want = np.broadcast_to(np.arange(1, 16, dtype=np.int32), own.shape)
    shifted, _, nredo = Q.neighbor_ranks(x, own, return_counts=True)
    assert nredo == 0 and np.array_equal(shifted, want)
    plain, namb, nredo = Q.neighbor_ranks(x, own, shift=None, return_counts=True)
    assert nredo == 257 and namb == 0                               # A exceeds the distances: nothing is certain
    assert np.array_equal(plain, want)
    d2 = KR.d2_float64(X, X, self_r0=0)
    tg = RR.graph_float64(d2, 40)[:, ::-1].copy()                   # any targets, in any order
    assert np.array_equal(Q.neighbor_ranks(x, tg, shift=None), Q.neighbor_ranks(x, tg))


@pytest.mark.parametrize("name", ["blobs_700x64", "randn_300x8"])
def test_metrics_against_the_interval(name):
    from dynamorph_amd import quality as Q
    X, Y, d2x, d2y = case(name)
    x, y = dev(X), dev(Y)
    N = len(X)
    gy, gx = gpu_graph(Y, 15), gpu_graph(X, 15)
    T = Q.trustworthiness(x, y, (5, 15), y_graph=(gy, None))
    C = Q.continuity(x, y, (5, 15), x_graph=(gx, None))
    assert isinstance(T, tuple) and T == (Q.trustworthiness(x, y, 5), Q.trustworthiness(x, y, 15)) and isinstance(T[1], float)
    assert C == (Q.continuity(x, y, 5), Q.continuity(x, y, 15))
    for k, t, cnt in ((5, T[0], C[0]), (15, T[1], C[1])):
        for got, d2, tg, what in ((t, d2x, gy, "trustworthiness"), (cnt, d2y, gx, "continuity")):
            lo, hi = RR.rank_interval(d2, tg[:, :k])
            ref = RR.trustworthiness_from_ranks(lo, k)
            slack = RR.normalisation(N, k) * float((hi - lo).sum())
            print(f"{name} {what}({k}) = {got:.6f}, reference {ref:.6f}, interval slack {slack:.2e}")
            assert abs(got - ref) <= slack + 1e-15 and 0.0 < got <= 1.0
    with pytest.raises(ValueError, match="self column"):
        Q.continuity(x, y, 15, x_graph=(gx[:, :10], None))


def test_metrics_on_the_lattice_are_exact():
    from dynamorph_amd import quality as Q
    X, Y = (np.array(a) for a in RR.fixture("lattice_400x6"))
    assert Q.trustworthiness(dev(X), dev(Y), 15) == UR.trustworthiness(X, Y, 15)
    assert Q.continuity(dev(X), dev(Y), 15) == UR.trustworthiness(Y, X, 15)
    assert Q.trustworthiness(X, Y, (5, 15)) == (UR.trustworthiness(X, Y, 5), UR.trustworthiness(X, Y, 15))     # host data


def test_embedding_quality_equals_the_separate_calls():
    import dynamorph_amd
    from dynamorph_amd import quality as Q
    assert dynamorph_amd.trustworthiness is Q.trustworthiness and dynamorph_amd.continuity is Q.continuity
    assert dynamorph_amd.embedding_quality is Q.embedding_quality
    X, Y = (np.array(a) for a in RR.fixture("randn_300x8"))
    Y2 =np.ascontiguousarray(X[:, 5:8])
    res = Q.embedding_quality(X, {"svd": Y, "cols": Y2}, n_neighbors=15)
    assert sorted(res) == ["cols", "svd"]
    for name, emb in (("svd", Y), ("cols", Y2)):
        assert sorted(res[name]) == ["continuity", "neighbor_recall", "trustworthiness"]
        assert res[name]["trustworthiness"] == Q.trustworthiness(X, emb, 15)
        assert res[name]["continuity"] == Q.continuity(X, emb, 15)
        ranks = Q.neighbor_ranks(X, gpu_graph(emb, 15))
        assert res[name]["neighbor_recall"] == float((ranks <= 15).mean())
    many = Q.embedding_quality(X, {str(i): Y2 if i % 2 else Y for i in range(3)}, n_neighbors=(5, 100))    # 2 per pass at k = 100
    assert many["0"] == many["2"] and many["1"]["trustworthiness"][0] == Q.trustworthiness(X, Y2, 5)
    assert many["0"]["continuity"] == Q.continuity(X, Y, (5, 100))


def test_score_umap_embeddings_round_trip(tmp_path):
    from dynamorph_amd import dim_reduction as DR
    from dynamorph_amd import quality as Q
    X = UR.fixture(300, 32)
    w = str(tmp_path / "w")
    out = DR.fit_umap_embedding(X, w, labels=list(range(300)), n_nbrs=(5, 15), n_epochs=30, seed=3)
    scores = DR.score_umap_embeddings(X, w, n_neighbors=10)
    names = ["embedding_umap_nbr15_a1.58_b0.9", "embedding_umap_nbr5_a1.58_b0.9"]
    assert sorted(scores) == names and "embedding_quality.pkl" in os.listdir(w)
    with open(os.path.join(w, "embedding_quality.pkl"), "rb") as f:
        back = pickle.load(f)
    assert type(back) is dict and back == scores
    for n, name in ((15, names[0]), (5, names[1])):
        assert scores[name] == Q.embedding_quality(X, {"e": out[(n, 1.58, 0.9)]}, n_neighbors=10)["e"]
        assert all(isinstance(v, float) and 0.0 < v <= 1.0 for v in scores[name].values())
    assert DR.score_umap_embeddings(X, w, n_neighbors=10) == scores      # its own output is not taken for an embedding
