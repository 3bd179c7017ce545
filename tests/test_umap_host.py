"""`not gpu`: the host half of the UMAP embedding (dynamorph_amd/umap_layout.py) -- the float64
restatement's own smooth-distance search, the torch plumbing (symmetrise, prune, schedule) on CPU tensors against scipy and
float32 numpy, argument refusal before any device call, the file names of the pipeline wrapper, the generator, and the
helper's trustworthiness against scikit-learn's."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import umap_reference as UR  # noqa: E402

from dynamorph_amd import umap_layout as U  # noqa: E402

KS = (2, 15, 200, 256)


@pytest.fixture(scope="module")
def graphs():
    X = UR.fixture()
    idx, dist = UR.knn_float64(X, 256)
    return {k: (np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(dist[:, :k])) for k in KS}


@pytest.mark.parametrize("k", KS)
def test_helper_sigma_solves_its_equation(graphs, k):
    idx, dist = graphs[k]
    assert not dist[:5, 1:min(k, 5)].any() and (dist[5:, 1] > 0).all()          # the zero distances of the identical rows
    rho, sigma, floored, out_of_steps, sigma64 = UR.smooth(dist, full=True)
    exempt = floored | out_of_steps
    print(f"k={k}: {floored.sum()} rows floored, {out_of_steps.sum()} out of steps, of {len(rho)}")
    assert exempt.mean() <= 0.05
    assert not (out_of_steps & ~floored).any()          # a search that runs out of steps has gone to 0 and is floored
    first_pos = np.array([r[r > 0][0] if (r > 0).any() else 0.0 for r in dist[:, 1:]], np.float32)
    assert np.array_equal(rho, first_pos)
    err64 = np.abs(UR.S(dist, rho, sigma64) - np.log2(k))
    assert err64[~exempt].max() <= 1e-5
    # stored as float32 (2^-24 relative, times sigma dS/dsigma <= (k - 1) / e) the same rows stay within 2e-5
    err32 = np.abs(UR.S(dist, rho, sigma.astype(np.float64)) - np.log2(k))
    print(f"k={k}: |S - log2 k| <= {err64[~exempt].max():.2e} (float64 sigma), {err32[~exempt].max():.2e} (float32 sigma)")
    assert err32[~exempt].max() <= 2e-5
    fl, _, _ = UR.floors(dist, rho)
    assert np.array_equal(sigma[floored], fl[floored].astype(np.float32))


def test_generator_matches_the_module():
    for seed, n, e, p in ((0, 0, 0, 0), (7, 199, 123456, 4), (2 ** 63 + 5, 57, 2 ** 33 + 1, 300)):
        assert int(U.counter_word(seed, n, e, p)) == UR.word(seed, n, e, p)
    u = U.jitter(3, 50)
    assert u.dtype == np.float32 and np.array_equal(u, UR.jitter(3, 50)) and (u >= -1).all() and (u < 1).all()
    draws = np.array([UR.R(0, 3, e, p) % 400 for e in range(2000) for p in range(5)])
    assert draws.min() == 0 and draws.max() == 399 and np.bincount(draws, minlength=400).max() < 60


@pytest.mark.parametrize("k", KS)
def test_symmetrize_prune_schedule_on_cpu_tensors(graphs, k):
    idx, dist = graphs[k]
    rho, sigma, _, _ = UR.smooth(dist)
    a = UR.membership(idx, dist, rho, sigma).astype(np.float32)
    a[7, 1] = 0.0                                                        # a zero that is dropped from the pattern
    indptr, cols, w = U.symmetrize(torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(a))
    UR.check_structure(indptr.numpy(), cols.numpy(), w.numpy(), idx, a)
    for n_epochs in (200, 500):
        p_indptr, p_cols, p_w = U.prune(indptr, cols, w, n_epochs)
        keep, eps_ref, neg_ref = UR.schedule(w.numpy(), n_epochs, 5)
        rows = np.repeat(np.arange(len(idx)), np.diff(indptr.numpy()))
        assert np.array_equal(p_cols.numpy(), cols.numpy()[keep]) and np.array_equal(p_w.numpy(), w.numpy()[keep])
        assert np.array_equal(np.diff(p_indptr.numpy()), np.bincount(rows[keep], minlength=len(idx)))
        assert (p_w.numpy() >= w.numpy().max() / np.float32(n_epochs)).all()
        eps, eps_neg = U.schedule(p_w, 5)
        assert np.array_equal(eps.numpy().view(np.uint32), eps_ref.view(np.uint32))
        assert np.array_equal(eps_neg.numpy().view(np.uint32), neg_ref.view(np.uint32))
        assert eps.numpy().min() == 1.0
    if k >= 15:
        assert keep.sum() < len(keep)                                    # the pruning is exercised


def test_symmetrize_refuses_a_repeated_column():
    idx = torch.tensor([[0, 1, 1], [1, 0, 2], [2, 0, 1]], dtype=torch.int32)
    with pytest.raises(ValueError, match="twice"):
        U.symmetrize(idx, torch.ones((3, 3)))


def test_init_layout_matches_the_restatement():
    y = np.random.default_rng(2).standard_normal((40, 2)).astype(np.float32) * [3.0, 0.5]
    y[:, 1] = 2.0                                                        # a constant dimension: only the jitter is left
    got = U.init_layout(torch.from_numpy(y.astype(np.float32)), 11).numpy()
    want = UR.init_layout(y.astype(np.float32), 11)
    assert np.array_equal(got, want)
    assert got[:, 0].min() >= -1e-4 and got[:, 0].max() <= 10 + 1e-4 and np.abs(got[:, 1]).max() <= 1e-4


def test_refused_arguments_raise_before_any_device_call(monkeypatch, graphs):
    from dynamorph_amd import knn, ops

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    for name in ("umap_smooth", "umap_membership", "umap_epoch", "knn", "pca_colsum", "pca_gram", "pca_transform"):
        monkeypatch.setattr(ops, name, no_device)
    monkeypatch.setattr(knn, "knn_graph", no_device)
    idx, dist = graphs[15]
    y0 = np.zeros((300, 2), np.float32)
    emb = U.UMAPEmbedding()
    with pytest.raises(ValueError, match="outside 2"):
        emb.fit_graph(idx[:, :1], dist[:, :1], y0)
    wide = np.tile(idx, (1, 18))[:, :257]
    with pytest.raises(ValueError, match="outside 2"):
        emb.fit_graph(wide, np.zeros(wide.shape, np.float32), y0)
    with pytest.raises(ValueError, match="exceeds"):
        emb.fit_graph(idx[:10], dist[:10], y0[:10])
    bad = idx.copy()
    bad[3, 4] = 300
    with pytest.raises(ValueError, match="outside 0"):
        emb.fit_graph(bad, dist, y0)
    bad[3, 4] = -1
    with pytest.raises(ValueError, match="outside 0"):
        U.fuzzy_graph(bad, dist)
    bad = idx.copy()
    bad[9, 0] = 8
    with pytest.raises(ValueError, match="column 0"):
        emb.fit_graph(bad, dist, y0)
    with pytest.raises(ValueError, match="column 0"):
        U.fuzzy_graph(bad, dist)
    with pytest.raises(ValueError, match="two output dimensions"):
        emb.fit_graph(idx, dist, np.zeros((300, 3), np.float32))
    with pytest.raises(ValueError, match="two output dimensions"):
        U.UMAPEmbedding(init=np.zeros((300, 3), np.float32))
    with pytest.raises(ValueError, match="two output dimensions"):
        U.UMAPEmbedding(n_components=3)
    with pytest.raises(ValueError, match="rows"):
        emb.fit_graph(idx, dist, y0[:299])
    with pytest.raises(ValueError, match="pca"):
        emb.fit_graph(idx, dist)                                         # no data to take the PCA of
    with pytest.raises(ValueError, match="spectral"):
        U.UMAPEmbedding(init="spectral")
    with pytest.raises(ValueError, match="n_neighbors"):
        U.UMAPEmbedding(n_neighbors=257)
    with pytest.raises(ValueError, match="exceeds"):
        U.UMAPEmbedding(n_neighbors=15).fit_transform(np.zeros((10, 4), np.float32))
    with pytest.raises(ValueError, match="shape"):
        emb.fit_graph(idx, dist[:, :14], y0)


def test_cabi_umap_argument_errors_are_reported_before_any_launch():
    import ctypes
    import subprocess
    from conftest import ROOT
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host checks
    assert lib.dm_umap_smooth(None, 10, 5, fake, fake, fake, fake, None) == -1 and b"NULL" in lib.dm_last_error()
    assert lib.dm_umap_smooth(fake, 10, 1, fake, fake, fake, fake, None) == -1 and b"k outside" in lib.dm_last_error()
    assert lib.dm_umap_smooth(fake, 300, 257, fake, fake, fake, fake, None) == -1
    assert lib.dm_umap_smooth(fake, 10, 11, fake, fake, fake, fake, None) == -1 and b"exceeds" in lib.dm_last_error()
    assert lib.dm_umap_membership(fake, fake, 10, 5, fake, None, fake, None) == -1 and b"NULL" in lib.dm_last_error()
    assert lib.dm_umap_membership(fake, fake, 0, 5, fake, fake, fake, None) == -1

    def epoch(**kw):
        args = dict(indptr=fake, cols=fake, N=10, nnz=20, eps=fake, eps_neg=fake, nxt=fake, nxt_neg=fake, y_in=fake,
                    y_out=ctypes.c_void_p(8192), epoch=0, n_epochs=10, a=1.58, b=0.9, gamma=1.0, seed=0, group=0)
        args.update(kw)
        return lib.dm_umap_epoch(*args.values(), None)
    assert epoch(y_out=fake) == -1 and b"same buffer" in lib.dm_last_error()
    assert epoch(epoch=10) == -1 and b"epoch" in lib.dm_last_error()
    assert epoch(group=16) == -1 and b"group" in lib.dm_last_error()
    assert epoch(a=0.0) == -1 and b"positive" in lib.dm_last_error()
    assert epoch(cols=None) == -1 and b"NULL" in lib.dm_last_error()
    assert epoch(N=0) == -1


def test_pipeline_file_names(monkeypatch, tmp_path):
    """fit_umap_embedding writes knn_nbr<n>.pkl and embedding_umap_nbr<n>_a<a>_b<b>.pkl, none of which the reference's
    umap_transform (which lists umap*.pkl) would pick up.  The device stages are replaced; the wrapper is what runs."""
    from dynamorph_amd import dim_reduction as DR
    from dynamorph_amd import knn
    X = UR.fixture(60, 8)
    monkeypatch.setattr(knn, "_resident", lambda x, device=None: x)
    monkeypatch.setattr(knn, "knn_graph", lambda x, k, include_self=True, **kw: UR.knn_float64(x, k))
    monkeypatch.setattr(U, "pca_coordinates", lambda x, device=None: torch.from_numpy(np.asarray(x)[:, :2].copy()))
    seen = []

    def fit_graph(self, idx, dist, init=None):
        seen.append((self.n_neighbors, self.a, self.b, idx.shape, init.shape))
        self.embedding_ = np.full((idx.shape[0], 2), self.n_neighbors, np.float32)
        return self
    monkeypatch.setattr(U.UMAPEmbedding, "fit_graph", fit_graph)
    labels = list(range(60))
    out = DR.fit_umap_embedding(X, str(tmp_path), labels=labels, n_nbrs=(5, 20), a_s=(1.58, 1.0), b_s=(0.9,), seed=3)
    names = sorted(os.listdir(tmp_path))
    assert names == ["embedding_umap_nbr20_a1.0_b0.9.pkl", "embedding_umap_nbr20_a1.58_b0.9.pkl",
                     "embedding_umap_nbr5_a1.0_b0.9.pkl", "embedding_umap_nbr5_a1.58_b0.9.pkl", "knn_nbr20.pkl", "knn_nbr5.pkl"]
    assert not any(n.startswith("umap") for n in names)
    assert sorted(out) == [(5, 1.0, 0.9), (5, 1.58, 0.9), (20, 1.0, 0.9), (20, 1.58, 0.9)]
    assert sorted(s[:3] for s in seen) == sorted(out) and all(s[3] == (60, s[0]) and s[4] == (60, 2) for s in seen)
    with open(tmp_path / "embedding_umap_nbr5_a1.58_b0.9.pkl", "rb") as f:
        emb, lab = pickle.load(f)
    assert emb.shape == (60, 2) and emb.dtype == np.float32 and (emb == 5).all() and lab == labels


def test_trustworthiness_equals_scikit_learn():
    sk = pytest.importorskip("sklearn.manifold")
    rng = np.random.default_rng(8)
    X = rng.standard_normal((120, 10))
    for Y in (X[:, :2], rng.standard_normal((120, 2)), X[:, :2] + 0.3 * rng.standard_normal((120, 2))):
        for k in (5, 15):
            assert abs(UR.trustworthiness(X, Y, k) - sk.trustworthiness(X, Y, n_neighbors=k)) <= 1e-12
    assert UR.trustworthiness(X, X, 15) == 1.0
