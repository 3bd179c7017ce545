"""`gpu`: the UMAP embedding (csrc/umap.hip, dynamorph_amd/umap_layout.py) against the float64 restatement of DESIGN.md section
3.5c in tests/helpers/umap_reference.py: smooth distances, memberships and the symmetrised graph on randn(300, 32) with five
identical rows (zero distances; rho is the first positive one) at k = 2, 15, 200, 256; one layout epoch, teacher-forced, at
N = 400; determinism of whole fits; the quality of the embedding on two data sets; the pipeline wrapper."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import umap_reference as UR  # noqa: E402

pytestmark = pytest.mark.gpu

KS = (2, 15, 200, 256)
_cache = {}


def graph_at(k):
    """The device's exact graph of the fixture at k = 256, once; its first k columns."""
    from dynamorph_amd import knn as K
    if "g" not in _cache:
        _cache["g"] = K.knn_graph(torch.from_numpy(UR.fixture()).cuda(), 256, include_self=True)
    idx, dist = _cache["g"]
    return np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(dist[:, :k])


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("k", KS)
def test_smooth(k):
    from dynamorph_amd import ops
    idx, dist = graph_at(k)
    rho, sigma, row_mean, global_mean = (t.cpu().numpy() for t in ops.umap_smooth(torch.from_numpy(dist).cuda()))
    rho_ref, _, floored_ref, _ = UR.smooth(dist)
    assert rho.dtype == np.float32 and sigma.dtype == np.float32
    assert np.array_equal(bits(rho), bits(rho_ref))
    assert not dist[:5, 1:min(k, 5)].any()                              # the identical rows: zero distances, and
    assert (rho[:5] > 0).all() if k > 5 else not rho[:5].any()          # rho is the first positive one, or 0 if there is none
    fl, rm, gm = UR.floors(dist, rho)
    np.testing.assert_allclose(row_mean, rm, rtol=1e-14)
    np.testing.assert_allclose(global_mean[0], gm, rtol=1e-13)
    exempt = sigma == fl.astype(np.float32)                             # rows that carry exactly the floor
    assert not (floored_ref & ~exempt).any(), "a row the float64 search floors does not carry the floor"
    err = np.abs(UR.S(dist, rho, sigma.astype(np.float64)) - np.log2(k))
    print(f"k={k}: {exempt.sum()} of {len(rho)} rows carry the floor; |S - log2 k| <= {err[~exempt].max():.2e} on the others")
    assert exempt.mean() <= 0.05
    assert err[~exempt].max() <= 2e-5


@pytest.mark.parametrize("k", KS)
def test_membership_and_graph(k):
    from dynamorph_amd import ops
    from dynamorph_amd import umap_layout as U
    idx, dist = graph_at(k)
    d = torch.from_numpy(dist).cuda()
    i32 = torch.from_numpy(idx.astype(np.int32)).cuda()
    rho, sigma, _, _ = ops.umap_smooth(d)
    a = ops.umap_membership(i32, d, rho, sigma).cpu().numpy()
    want = UR.membership(idx, dist, rho.cpu().numpy(), sigma.cpu().numpy())
    err = np.abs(a.astype(np.float64) - want).max()
    print(f"k={k}: membership within {err:.2e} of the float64 closed form")
    assert err <= 1e-6
    assert not a[:, 0].any() and (a[:, 1] == 1.0).all()
    g1 = U.fuzzy_graph(idx, dist)
    g2 = U.fuzzy_graph(idx, dist)
    indptr, cols, w, rho1, sigma1 = (t.cpu().numpy() for t in g1)
    UR.check_structure(indptr, cols, w, idx, a)
    assert np.array_equal(bits(rho1), bits(rho.cpu().numpy())) and np.array_equal(bits(sigma1), bits(sigma.cpu().numpy()))
    for x, y in zip(g1, g2):                                            # a relaunch gives the same bits
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------ one epoch
def layout_problem():
    """N = 400, k = 15, n_epochs = 200: the pruned graph, the schedule and the state before epochs 0, 1, 57 and 199 of the
    device's own run."""
    from dynamorph_amd import knn as K
    from dynamorph_amd import ops
    from dynamorph_amd import umap_layout as U
    if "layout" in _cache:
        return _cache["layout"]
    X = torch.from_numpy(UR.fixture(400, 32, seed=77)).cuda()
    idx, dist = K.knn_graph(X, 15, include_self=True)
    indptr, cols, w, _, _ = U.fuzzy_graph(idx, dist)
    indptr, cols, w = U.prune(indptr, cols, w, 200)
    eps, eps_neg = U.schedule(w, 5)
    nxt, nxt_neg = eps.clone(), eps_neg.clone()
    y = U.init_layout(U.pca_coordinates(X), 9)
    other = torch.empty_like(y)
    states = {}
    for n in range(200):
        if n in (0, 1, 57, 199):
            states[n] = (y.clone(), nxt.clone(), nxt_neg.clone())
        ops.umap_epoch(indptr, cols, eps, eps_neg, nxt, nxt_neg, y, other, n, 200, 1.58, 0.9, 1.0, 9)
        y, other = other, y
    _cache["layout"] = (indptr, cols, eps, eps_neg, states)
    return _cache["layout"]


COUNTS = {}


@pytest.mark.parametrize("n", [0, 1, 57, 199])
def test_one_epoch_teacher_forced(n):
    """The kernel and the float64 restatement start epoch n from the same float32 positions and the same schedule state.  The
    positions are those of the device's run with three firing pairs made coincident and 40 vertices drawn together on a grid
    of spacing 0.02 (every repulsion inside it is clipped; none falls below the 0.002 where the unclipped gradient is steep).
    The kernel may deviate from float64 by 4 x what a float32 numpy evaluation deviates, plus 1e-5."""
    from dynamorph_amd import ops
    indptr, cols, eps, eps_neg, states = layout_problem()
    y, nxt, nxt_neg = (t.clone() for t in states[n])
    fired = torch.nonzero(nxt <= float(n)).flatten()[:3].cpu().numpy()
    rows = np.repeat(np.arange(400), np.diff(indptr.cpu().numpy()))
    c = cols.cpu().numpy()
    grid = torch.tensor([[0.02 * (t % 8), 0.02 * (t // 8)] for t in range(40)], device="cuda")
    y[100:140] = y[100] + grid
    for e in fired:
        if not (100 <= rows[e] < 140 or 100 <= c[e] < 140):
            y[c[e]] = y[rows[e]]
    y0 = y.cpu().numpy()
    args = (indptr.cpu().numpy(), c, eps.cpu().numpy(), eps_neg.cpu().numpy(), nxt.cpu().numpy(), nxt_neg.cpu().numpy(), y0,
            n, 200, 1.58, 0.9, 1.0, 9)
    y64, nxt64, neg64, counts = UR.epoch(*args, dtype=np.float64)
    y32, nxt32, neg32, _ = UR.epoch(*args, dtype=np.float32)
    assert np.array_equal(bits(nxt64), bits(nxt32)) and np.array_equal(bits(neg64), bits(neg32))
    out = ops.umap_epoch(indptr, cols, eps, eps_neg, nxt, nxt_neg, y, torch.empty_like(y), n, 200, 1.58, 0.9, 1.0, 9)
    assert np.array_equal(bits(nxt.cpu().numpy()), bits(nxt32)), "next differs from the float32 evaluation"
    assert np.array_equal(bits(nxt_neg.cpu().numpy()), bits(neg32)), "next_neg differs from the float32 evaluation"
    dev32 = np.abs(y32.astype(np.float64) - y64).max()
    err = np.abs(out.cpu().numpy().astype(np.float64) - y64).max()
    moved = np.abs(y64 - y0).max()
    print(f"epoch {n}: {counts}; largest move {moved:.3f}; float32 numpy deviates {dev32:.2e}, the kernel {err:.2e} "
          f"(allowed {4 * dev32 + 1e-5:.2e})")
    COUNTS[n] = counts
    if n == 0:
        assert counts["fired"] == 0 and np.array_equal(out.cpu().numpy(), y0)      # next_e = eps_e >= 1: nothing fires yet
    else:
        assert counts["fired"] > 0 and moved > 0.1
    assert err <= 4 * dev32 + 1e-5
    if len(COUNTS) == 4:                                                # the cases together cover the special paths
        for what in ("self", "coincident", "clipped"):
            assert sum(cn[what] for cn in COUNTS.values()) > 0, what


def test_epoch_does_not_depend_on_the_lanes_per_vertex():
    from dynamorph_amd import ops
    indptr, cols, eps, eps_neg, states = layout_problem()
    res = []
    for group in (0, 1, 8, 32):
        y, nxt, nxt_neg = (t.clone() for t in states[57])
        out = ops.umap_epoch(indptr, cols, eps, eps_neg, nxt, nxt_neg, y, torch.empty_like(y), 57, 200, 1.58, 0.9, 1.0, 9, group)
        res.append((out, nxt, nxt_neg))
    for r in res[1:]:
        for x, y in zip(res[0], r):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert not torch.equal(res[0][0], states[57][0])


def test_fits_are_deterministic():
    from dynamorph_amd import umap_layout as U
    X = UR.fixture()
    a = U.UMAPEmbedding(n_neighbors=15, seed=4).fit_transform(X)
    b = U.UMAPEmbedding(n_neighbors=15, seed=4).fit_transform(torch.from_numpy(X).cuda())
    c = U.UMAPEmbedding(n_neighbors=15, seed=5).fit_transform(X)
    assert a.shape == (300, 2) and a.dtype == np.float32 and np.isfinite(a).all()
    assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(bits(a), bits(c))


# --------------------------------------------------------------------------------------------------------------- quality
def test_quality_blobs():
    from dynamorph_amd import umap_layout as U
    X, labels = UR.blobs()
    emb = U.UMAPEmbedding(n_neighbors=15, n_epochs=200)
    Y = emb.fit_transform(X)
    share = UR.neighbour_label_share(Y, labels, 10)
    t_init, t_fit = UR.trustworthiness(X, emb.init_, 15), UR.trustworthiness(X, Y, 15)
    print(f"blobs: {share:.4f} of the 10 nearest 2-D neighbours share the label; trustworthiness(15) {t_init:.4f} (init) -> {t_fit:.4f}")
    assert share >= 0.99
    assert t_fit >= t_init


def test_quality_curve():
    from dynamorph_amd import umap_layout as U
    X = UR.curve()
    emb = U.UMAPEmbedding(n_neighbors=15)
    Y = emb.fit_transform(X)
    t_init, t_fit = UR.trustworthiness(X, emb.init_, 15), UR.trustworthiness(X, Y, 15)
    print(f"curve: trustworthiness(15) {t_init:.4f} (PCA initialisation) -> {t_fit:.4f}")
    assert t_fit > t_init


# -------------------------------------------------------------------------------------------------------------- pipeline
def test_pipeline(tmp_path):
    from dynamorph_amd import dim_reduction as DR
    from dynamorph_amd import umap_layout as U
    rng = np.random.default_rng(21)
    dirs, sizes = [], (120, 90, 130)
    for w, n in enumerate(sizes):
        d = tmp_path / f"well{w}"
        d.mkdir()
        with open(d / "p_latent_space_after.pkl", "wb") as f:
            pickle.dump(rng.standard_normal((n, 32)).astype(np.float32) + w, f, protocol=4)
        dirs.append(str(d))
    wdir = tmp_path / "weights"
    out = DR.dim_reduction_umap_embedding(dirs, str(wdir), "p", n_nbrs=(15, 200), n_epochs=50, seed=2)
    names = sorted(os.listdir(wdir))
    assert names == ["embedding_umap_nbr15_a1.58_b0.9.pkl", "embedding_umap_nbr200_a1.58_b0.9.pkl", "knn_nbr15.pkl", "knn_nbr200.pkl"]
    pooled, labels = DR.pool_latents(dirs, "p")
    assert labels == [0] * 120 + [1] * 90 + [2] * 130
    with open(wdir / "knn_nbr200.pkl", "rb") as f:
        idx, dist = pickle.load(f)
    from dynamorph_amd import knn as K
    ref_idx, ref_dist = K.knn_graph(pooled, 200)
    assert np.array_equal(idx, ref_idx) and np.array_equal(bits(dist), bits(ref_dist))      # rows in pool_latents order
    for n in (15, 200):
        with open(wdir / f"embedding_umap_nbr{n}_a1.58_b0.9.pkl", "rb") as f:
            emb, lab = pickle.load(f)
        assert emb.shape == (340, 2) and emb.dtype == np.float32 and lab == labels
        assert np.array_equal(bits(emb), bits(out[(n, 1.58, 0.9)]))
    direct = U.UMAPEmbedding(n_neighbors=15, n_epochs=50, seed=2).fit_graph(idx[:, :15], dist[:, :15], U.pca_coordinates(pooled))
    assert np.array_equal(bits(direct.embedding_), bits(out[(15, 1.58, 0.9)]))
    g = direct.graph()
    assert g.shape == (340, 340) and g.dtype == np.float32 and (g != g.T).nnz == 0
