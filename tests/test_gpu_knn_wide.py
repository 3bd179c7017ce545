"""`gpu`: the exact k-nearest-neighbour graph and UMAP of wide latents (more than 16384 features: knn.wide_knn_graph,
knn.wide_knn_query, WidePCA from a given row Gram matrix, UMAPEmbedding above the threshold).

Truth is the float64 reference of tests/helpers/knn_reference.py on the planted fixtures of tests/helpers/knn_wide_fixtures.py
(130 rows -- two ragged tiles -- of 16385 features, the first width past the narrow cap and no multiple of 4, and of 65536,
the VQ_VAE_z32 width, plain and at offset 30).  Where both routes accept the width the wide route must return knn_graph's
indices and distance bits; and its results must not depend on slack, shift, a given Gram matrix, the refine kernels or the
path a row took."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import knn_reference as KR  # noqa: E402
import knn_wide_fixtures as WF  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def dev(X):
    return torch.from_numpy(np.array(X, dtype=np.float32)).cuda()


def wide_graph(X, k, **kw):
    from dynamorph_amd import knn as K
    return K.wide_knn_graph(X if torch.is_tensor(X) else dev(X), k, return_fallback=True, return_pairs=True, **kw)


def same(a, b):
    """Indices equal and distances equal in every bit."""
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def x201():
    """Fixture 201 on the device, once."""
    if "x201" not in _cache:
        _cache["x201"] = dev(WF.wide_case("201_130x16385")[0])
    return _cache["x201"]


# ------------------------------------------------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("k", [1, 15, 129])
@pytest.mark.parametrize("name", sorted(WF.WIDE))
def test_truth(name, k):
    X, d2 = WF.wide_case(name)
    share = KR.clear_share(d2, k)
    print(f"{name} k={k}: {share:.3f} of the rows are bound by index equality")
    assert share >= 0.85                                             # (the reference alone: the fixture binds)
    x = dev(X)
    idx, dist, nfb, npairs = wide_graph(x, k, include_self=False)
    print(f"{name} k={k}: {nfb} of {X.shape[0]} rows took the fallback, {npairs} pair evaluations")
    assert idx.dtype == np.int64 and dist.dtype == np.float32
    KR.assert_passes(idx, dist, d2, k, f"{name} k={k}", self_r0=0)
    idx_s, dist_s, _, _ = wide_graph(x, k, include_self=True)
    KR.assert_passes(idx_s, dist_s, d2, k, f"{name} k={k} include_self", self_r0=0, include_self=True)
    assert np.array_equal(idx_s[:, 1:], idx[:, :k - 1]) and np.array_equal(bits(dist_s[:, 1:]), bits(dist[:, :k - 1]))


def test_smallest_graph():
    """tests/test_gpu_knn.py::test_smallest_graph's answers; the one pair of the graph is evaluated once."""
    X = np.array([[0.5], [-2.0]], np.float32)
    idx, dist, nfb, npairs = wide_graph(X, 1, include_self=False)
    assert idx.tolist() == [[1], [0]] and dist.tolist() == [[2.5], [2.5]] and npairs == 1
    idx, dist, nfb, npairs = wide_graph(X, 2, include_self=True)
    assert idx.tolist() == [[0, 1], [1, 0]] and dist.tolist() == [[0.0, 2.5], [0.0, 2.5]] and npairs == 1
    idx, dist, nfb, npairs = wide_graph(X, 1, include_self=True)
    assert idx.tolist() == [[0], [1]] and dist.tolist() == [[0.0], [0.0]] and nfb == 0 and npairs == 0
    with pytest.raises(ValueError):
        wide_graph(X, 2, include_self=False)


# ------------------------------------------------------------------------------------- 2. the bits of the existing route
def _duplicates():
    Y = KR.randn(114, (400, 8)).copy()
    Y[100:300] = Y[100]
    return Y


def _hub():
    H = KR.randn(300, (300, 16)).copy()
    H[0] = 0
    return H


NARROW = {
    "plain_257x40": (lambda: KR.fixture("plain_257x40"), (15, 200), (None,)),
    "offset_257x64": (lambda: KR.fixture("offset_257x64"), (15, 200), (None,)),
    "randn_1000x64": (lambda: KR.randn(116, (1000, 64)), (15, 200), (None,)),
    "randn_130x4096": (lambda: KR.randn(111, (130, 4096)), (15, 200), (None,)),
    "duplicates_400x8": (_duplicates, (15,), (8,)),
    "hub_300x16": (_hub, (5,), (0, 8)),
}


@pytest.mark.parametrize("name", sorted(NARROW))
def test_same_bits_as_knn_graph(name):
    from dynamorph_amd import knn as K
    make, ks, slacks = NARROW[name]
    X = make()
    x = dev(X)
    N = X.shape[0]
    for k in ks:
        if k > N - 1:
            continue
        for slack in slacks:
            for include_self in (False, True):
                ref = K.knn_graph(x, k, include_self=include_self, slack=slack)
                got = wide_graph(x, k, include_self=include_self, slack=slack)
                assert same(got, ref), (name, k, slack, include_self)
                plain = wide_graph(x, k, include_self=include_self, slack=slack, pair_once=False)
                assert same(plain, ref) and plain[2] == got[2] and plain[3] == 0, (name, k, slack, include_self)
            if name.startswith("hub"):                               # every row lists the hub, the hub lists few of them
                Kc = min(k + slack, N - 1)
                npairs = wide_graph(x, k, include_self=False, slack=slack)[3]
                print(f"hub slack={slack}: {npairs} pair evaluations for {N * Kc} slots")
                assert N * Kc / 2 <= npairs < N * Kc


@pytest.mark.parametrize("name", ["plain_257x40", "randn_130x4096"])
def test_same_bits_as_knn_query(name):
    from dynamorph_amd import knn as K
    X = NARROW[name][0]()
    Q = KR.randn(115, (70, X.shape[1]))
    x = dev(X)
    for k in (15, 200):
        if k > X.shape[0]:
            continue
        ref = K.knn_query(x, dev(Q), k, return_fallback=True)
        assert same(K.wide_knn_query(x, dev(Q), k, return_fallback=True), ref)
        assert same(K.wide_knn_query(x, Q, k, chunk_rows=32), ref)   # host queries, streamed in chunks


# ------------------------------------------------------------------------------ 3. results depend on the inputs only
def test_results_depend_on_the_inputs_only():
    from dynamorph_amd.pca import WidePCA
    x = x201()
    ref = wide_graph(x, 15)
    print(f"fixture 201, k = 15, default slack and shift: {ref[2]} fallback rows, {ref[3]} pair evaluations")
    for slack in (0, 8, 64, 256):
        got = wide_graph(x, 15, slack=slack)
        print(f"slack {slack}: {got[2]} fallback rows, {got[3]} pair evaluations")
        assert same(got, ref), slack
    assert same(wide_graph(x, 15, shift=None), ref)
    with torch.no_grad():
        g = WidePCA().gram(x)
    K0 = g[2].clone()
    assert same(wide_graph(x, 15, gram=g), ref)
    assert torch.equal(g[2], K0)                                     # a given K is left as it was
    assert same(wide_graph(x, 15, pair_once=False), ref)
    again = wide_graph(x, 15)
    assert same(again, ref) and again[2:] == ref[2:]


def test_forced_fallback():
    """3 + 1e-2 randn(130, 16385) without the shift: the bound A = 5.6e-4 F exceeds every d^2 = 2e-4 F, so no row can be
    certified and all 130 go through the fallback -- to the bits of the shifted run."""
    X = (np.float32(3) + np.float32(1e-2) * KR.randn(120, (130, 16385))).astype(np.float32)
    x = dev(X)
    shifted = wide_graph(x, 15)
    print(f"shifted run: {shifted[2]} of 130 rows took the fallback")
    raw = wide_graph(x, 15, shift=None)
    assert raw[2] == 130
    assert same(raw, shifted)


# --------------------------------------------------------------------------------------------- 4. foreign queries at width
def test_foreign_queries_at_width():
    from dynamorph_amd import knn as K
    A = WF.planted(205, 200, 16385)
    X, Q = A[:130], A[130:]
    d2 = KR.d2_float64(Q, X)
    x, q = dev(X), dev(Q)
    full = K.wide_knn_query(x, q, 130, return_fallback=True)
    for k in (1, 15, 130):
        idx, dist, nfb = K.wide_knn_query(x, q, k, return_fallback=True)
        print(f"k={k}: {nfb} of 70 queries took the fallback")
        assert idx.dtype == np.int64 and dist.dtype == np.float32
        KR.assert_passes(idx, dist, d2, k, f"foreign k={k}")
        assert np.array_equal(idx, full[0][:, :k]) and np.array_equal(bits(dist), bits(full[1][:, :k]))
    with pytest.raises(ValueError, match="exceeds"):
        K.wide_knn_query(x, q, 131)
    idx, dist = K.wide_knn_query(x, x[40:43], 2)                     # a query that is a row of X: itself at 0.0
    assert idx[:, 0].tolist() == [40, 41, 42] and dist[:, 0].tolist() == [0.0, 0.0, 0.0] and (dist[:, 1] > 0).all()


# ----------------------------------------------------------------------------------------- 5. WidePCA from a given Gram
def test_wide_pca_from_a_given_gram():
    from dynamorph_amd.pca import _ATTRS, WidePCA
    x = x201()
    plain = WidePCA(n_components=2).fit(x)
    with torch.no_grad():
        g = WidePCA().gram(x)
    K0 = g[2].clone()
    given = WidePCA(n_components=2).fit(x, gram=g)
    assert torch.equal(g[2], K0)                                     # copied, not centred in place
    used = WidePCA(n_components=2)
    y = used.fit_transform(x, gram=g, consume_gram=True)
    for a in _ATTRS:
        for m in (given, used):
            va, vb = getattr(plain, a), getattr(m, a)
            assert np.array_equal(va, vb) if isinstance(va, np.ndarray) else va == vb, a
    assert torch.equal(y, plain.transform(x))


# ------------------------------------------------------------------------------------------------------ 6. UMAP at width
NE = 30


def test_umap_at_width(tmp_path):
    from dynamorph_amd import dim_reduction as DR
    from dynamorph_amd import knn as K
    from dynamorph_amd.umap_layout import UMAPEmbedding, pca_coordinates
    x = x201()
    X = np.array(WF.wide_case("201_130x16385")[0])                   # (writable copies: torch.from_numpy warns otherwise)
    Q = np.array(WF.planted(206, 20, 16385))                         
    model = UMAPEmbedding(n_neighbors=15, n_epochs=NE, seed=3)
    emb = model.fit_transform(x)
    by_hand = UMAPEmbedding(n_neighbors=15, n_epochs=NE, seed=3).fit_graph(*K.wide_knn_graph(x, 15), init=pca_coordinates(x))
    assert emb.shape == (130, 2) and np.array_equal(bits(emb), bits(by_hand.embedding_))
    placed = model.transform(Q)
    expect = model.transform_graph(*K.wide_knn_query(x, Q, 15))
    assert placed.shape == (20, 2) and np.array_equal(bits(placed), bits(expect))
    back = pickle.loads(pickle.dumps(model, protocol=4))
    assert isinstance(back._X, np.ndarray) and back._X.shape == (130, 16385)
    assert np.array_equal(bits(back.transform(Q)), bits(placed))

    w = str(tmp_path / "w")
    out = DR.fit_umap_embedding(X, w, n_nbrs=(5, 15), save_models=True, n_epochs=NE, seed=3)
    names = sorted(os.listdir(w))
    assert names == ["embedding_umap_nbr15_a1.58_b0.9.pkl", "embedding_umap_nbr5_a1.58_b0.9.pkl", "knn_nbr15.pkl",
                     "knn_nbr5.pkl", "umap_model_nbr15_a1.58_b0.9.pkl", "umap_model_nbr5_a1.58_b0.9.pkl"]
    assert np.array_equal(bits(out[(15, 1.58, 0.9)]), bits(emb))     # the pipeline's fit is the model's
    ref = K.wide_knn_graph(x, 15)
    with open(os.path.join(w, "knn_nbr15.pkl"), "rb") as f:
        assert same(tuple(pickle.load(f)), ref)
    os.makedirs(tmp_path / "in")
    with open(tmp_path / "in" / "A_latent_space_after.pkl", "wb") as f:
        pickle.dump(Q, f, protocol=4)
    res = DR.umap_transform(str(tmp_path / "in"), str(tmp_path / "out"), w, "A")
    assert sorted(res) == ["umap_model_nbr15_a1.58_b0.9", "umap_model_nbr5_a1.58_b0.9"]
    assert np.array_equal(bits(res["umap_model_nbr15_a1.58_b0.9"]), bits(placed))
    with open(tmp_path / "out" / "A_latent_space_after_umap_model_nbr5_a1.58_b0.9.pkl", "rb") as f:
        got = pickle.load(f)
    assert got.dtype == np.float32 and got.shape == (20, 2) and np.isfinite(got).all()
