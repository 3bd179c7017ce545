"""`not gpu`: the host half of the sample-space ("wide") latent PCA (dynamorph_amd/pca.py: finalize_samples,
orient_components, WidePCA) -- finalisation from a float64 row Gram matrix, limit and rank errors before any device call, the C
ABI's argument errors and the choice of class by width -- against tests/golden/g17_pca_wide.npz (PCA(0.5) of
run_dim_reduction.py:33 on planted-spectrum latents of 16385 and 65536 features)."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from pca_fixture import checksum, make_x  # noqa: E402

from dynamorph_amd import pca as P  # noqa: E402


@pytest.fixture(scope="module")
def g17():
    return load_golden("g17_pca_wide.npz")


def _x(g, tag):
    rec = {k[len(tag) + 8:]: g[k] for k in g if k.startswith(tag + "_recipe_")}
    X = make_x(rec)
    assert checksum(X) == str(g[tag + "_sha256"])
    return X


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


@pytest.mark.parametrize("tag", ["f16385", "f65536"])
def test_finalize_samples_reproduces_scikit_learn(g17, tag):
    X = _x(g17, tag)
    N, F = X.shape
    s = X.mean(0).astype(np.float32).astype(np.float64)          # the shift the fit uses; the centring removes its rounding
    Xs = X - s
    fit = P.finalize_samples(torch.from_numpy(Xs @ Xs.T), N, F, 0.5)
    assert str(g17[f"{tag}_f64_solver"]) == "full" and str(g17[f"{tag}_f32_solver"]) == "full"
    k = int(g17[f"{tag}_f64_n_components_"])
    assert fit["n_components_"] == k == int(g17[f"{tag}_f32_n_components_"])
    np.testing.assert_allclose(fit["explained_variance_ratio_"], g17[f"{tag}_f64_explained_variance_ratio_"], rtol=1e-5)
    np.testing.assert_allclose(fit["explained_variance_"], g17[f"{tag}_f64_explained_variance_"], rtol=1e-5)
    np.testing.assert_allclose(fit["singular_values_"], g17[f"{tag}_f64_singular_values_"], rtol=1e-5)
    np.testing.assert_allclose(fit["noise_variance_"], float(g17[f"{tag}_f64_noise_variance_"]), rtol=1e-5)
    assert fit["n_samples_"] == N and fit["n_features_in_"] == F and "components_" not in fit
    W = fit["W"]
    assert tuple(W.shape) == (k, N) and W.dtype == torch.float64
    if tag == "f16385":
        V = P.orient_components(torch.from_numpy(W.numpy().astype(np.float32).astype(np.float64) @ Xs)).numpy()
        np.testing.assert_allclose(np.linalg.norm(V, axis=1), 1.0, rtol=1e-12)
        c = _cos(V, g17[f"{tag}_f64_components_"])
        assert c.min() >= 1 - 1e-6, c                     # >= 1 - tol: the same sign as well


def test_finalize_samples_does_not_depend_on_the_shift():
    rng = np.random.default_rng(4)
    X = rng.standard_normal((40, 300)) * rng.uniform(0.5, 2, 300) + 30.0
    Xc = X - X.mean(0)
    a = P.finalize_samples(torch.from_numpy(Xc @ Xc.T), 40, 300, 5)
    b = P.finalize_samples(torch.from_numpy((X - 29.0) @ (X - 29.0).T), 40, 300, 5)
    np.testing.assert_allclose(b["explained_variance_"], a["explained_variance_"], rtol=1e-9)
    w, _ = np.linalg.eigh(Xc.T @ Xc / 39)
    np.testing.assert_allclose(a["explained_variance_"], w[::-1][:5], rtol=1e-9)
    np.testing.assert_allclose(a["noise_variance_"], w[::-1][5:40].clip(0).mean(), rtol=1e-9)


def test_limit_and_rank_errors_raise_before_any_device_call(monkeypatch):
    from dynamorph_amd import ops

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    for name in ("pca_colsum", "pca_gram", "pca_transform", "pca_rowgram", "pca_components"):
        monkeypatch.setattr(ops, name, no_device)
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    with pytest.raises(ValueError, match="whiten"):
        P.WidePCA(0.5, whiten=True)
    with pytest.raises(ValueError, match="at least 2 samples"):
        P.WidePCA(0.5).fit(np.zeros((1, 20000), np.float32))
    big = torch.zeros(1, dtype=torch.float32).expand(24577, 16385)         # no memory behind it
    with pytest.raises(ValueError, match="16384.*24576"):
        P.WidePCA(0.5).fit(big)
    with pytest.raises(ValueError, match="16384.*24576"):
        P.WidePCA(0.5).fit_transform(big)
    with pytest.raises(ValueError, match=str(1 << 20)):
        P.WidePCA(0.5).fit(torch.zeros(1).expand(2, (1 << 20) + 1))
    with pytest.raises(ValueError, match="not fitted"):
        P.WidePCA(0.5).transform(np.zeros((2, 20000), np.float32))
    # PCA itself keeps its cap and its message
    with pytest.raises(ValueError, match="VQ_VAE_z32.*65536"):
        P.PCA(0.5).fit(np.zeros((2, 65536), np.float32))
    # rank: centred data of N samples have rank <= N - 1; duplicates lower it further
    rng = np.random.default_rng(6)
    X = rng.standard_normal((12, 50))
    X[7:] = X[:5]                                                           # 7 distinct rows: rank 6 after centring
    K = (X - X.mean(0)) @ (X - X.mean(0)).T
    with pytest.raises(ValueError, match="at most 6 components are defined"):
        P.finalize_samples(torch.from_numpy(K.copy()), 12, 50, None)
    with pytest.raises(ValueError, match="at most 6 components are defined"):
        P.finalize_samples(torch.from_numpy(K.copy()), 12, 50, 7)
    fit = P.finalize_samples(torch.from_numpy(K.copy()), 12, 50, 6)
    assert fit["n_components_"] == 6 and np.isfinite(fit["W"].numpy()).all()
    with pytest.raises(ValueError, match="between 0 and min"):
        P.finalize_samples(torch.from_numpy(K.copy()), 12, 50, 13)
    with pytest.raises(ValueError, match="float64"):
        P.finalize_samples(torch.zeros((12, 12)), 12, 50, 0.5)


def test_cabi_pca_wide_argument_errors_are_reported_before_any_launch():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host checks
    big = 1 << 40
    assert lib.dm_pca_rowgram(None, 10, 4, 4, None, fake, 0, fake, big, None) == -1 and b"X is NULL" in lib.dm_last_error()
    assert lib.dm_pca_rowgram(fake, 10, 4, 4, None, None, 0, fake, big, None) == -1 and b"K is NULL" in lib.dm_last_error()
    assert lib.dm_pca_rowgram(fake, 0, 4, 4, None, fake, 0, fake, big, None) == -1 and b"rows" in lib.dm_last_error()
    assert lib.dm_pca_rowgram(fake, 24577, 4, 4, None, fake, 0, fake, big, None) == -1 and b"24576" in lib.dm_last_error()
    assert lib.dm_pca_rowgram(fake, 10, 0, 4, None, fake, 0, fake, big, None) == -1 and b"features" in lib.dm_last_error()
    assert lib.dm_pca_rowgram(fake, 10, (1 << 20) + 1, 1 << 21, None, fake, 0, fake, big, None) == -1
    assert b"features" in lib.dm_last_error()
    assert lib.dm_pca_rowgram(fake, 10, 8, 4, None, fake, 0, fake, big, None) == -1
    assert b"leading dimension" in lib.dm_last_error()
    # 2000 x 65536: 136 tile pairs, split over the features -> a workspace is needed
    need = lib.dm_pca_rowgram_workspace_bytes(2000, 65536)
    assert need > 0 and need % (128 * 128 * 8 * 136) == 0 and need <= 2 << 30
    assert lib.dm_pca_rowgram(fake, 2000, 65536, 65536, None, fake, 0, None, big, None) == -1
    assert b"workspace is NULL" in lib.dm_last_error()
    assert lib.dm_pca_rowgram(fake, 2000, 65536, 65536, None, fake, 0, fake, need - 8, None) == -1
    assert b"workspace of" in lib.dm_last_error()
    # the plan is a function of (N, F) alone: one feature slab, or tile pairs enough for the part -> no split, no workspace
    assert lib.dm_pca_rowgram_workspace_bytes(2, 1) == 0 and lib.dm_pca_rowgram_workspace_bytes(2000, 256) == 0
    assert lib.dm_pca_rowgram_workspace_bytes(24576, 65536) == 0 and lib.dm_pca_rowgram_workspace_bytes(8192, 65536) == 0
    for n in (2, 129, 257, 1000, 2000, 5000):
        for f in (255, 1000, 16385, 65536, 1 << 20):
            assert 0 <= lib.dm_pca_rowgram_workspace_bytes(n, f) <= 2 << 30, (n, f)
    assert lib.dm_pca_rowgram_workspace_bytes(0, 4) == -1 and lib.dm_pca_rowgram_workspace_bytes(24577, 4) == -1
    assert lib.dm_pca_rowgram_workspace_bytes(4, 0) == -1 and lib.dm_pca_rowgram_workspace_bytes(4, (1 << 20) + 1) == -1

    assert lib.dm_pca_components(None, 10, 8, 8, None, fake, 4, fake, None) == -1 and b"X is NULL" in lib.dm_last_error()
    assert lib.dm_pca_components(fake, 10, 8, 8, None, None, 4, fake, None) == -1 and b"NULL" in lib.dm_last_error()
    assert lib.dm_pca_components(fake, 10, 8, 8, None, fake, 4, None, None) == -1 and b"NULL" in lib.dm_last_error()
    assert lib.dm_pca_components(fake, 10, 8, 8, None, fake, 0, fake, None) == -1 and b"components" in lib.dm_last_error()
    assert lib.dm_pca_components(fake, 10, 8, 8, None, fake, 513, fake, None) == -1 and b"components" in lib.dm_last_error()
    assert lib.dm_pca_components(fake, 24577, 8, 8, None, fake, 4, fake, None) == -1 and b"rows" in lib.dm_last_error()
    assert lib.dm_pca_components(fake, 10, 0, 8, None, fake, 4, fake, None) == -1 and b"features" in lib.dm_last_error()
    assert lib.dm_pca_components(fake, 10, 8, 7, None, fake, 4, fake, None) == -1
    assert b"leading dimension" in lib.dm_last_error()


def _attrs(F, k=3, N=40):
    rng = np.random.default_rng(F)
    V = np.linalg.qr(rng.standard_normal((F, k)))[0].T
    ev = np.array([3.0, 2.0, 1.0])[:k]
    return {"mean_": rng.standard_normal(F) + 30, "components_": V, "explained_variance_": ev,
            "explained_variance_ratio_": ev / 10, "singular_values_": np.sqrt(ev * (N - 1)), "noise_variance_": 0.1,
            "n_components_": k, "n_samples_": N, "n_features_in_": F}


def test_fit_and_load_choose_the_class_by_width(monkeypatch, tmp_path):
    from dynamorph_amd import dim_reduction as D
    made = []

    def fake_fit_transform(self, X, chunk_rows=None):
        made.append(type(self))
        self._set(_attrs(np.shape(X)[1]))
        return torch.zeros((np.shape(X)[0], 3))
    monkeypatch.setattr(P.PCA, "fit_transform", fake_fit_transform)
    monkeypatch.setattr(P.WidePCA, "fit_transform", fake_fit_transform)
    monkeypatch.setattr(D, "_scatter", lambda *a, **k: None)
    for F, cls in ((16384, P.PCA), (16385, P.WidePCA)):
        w = tmp_path / str(F)
        p = D.fit_PCA(np.zeros((40, F), np.float32), str(w))
        assert made[-1] is cls and type(p) is cls and isinstance(p, P.PCA)
        back = D.load_model(str(w))
        assert type(back) is cls
        for a in P._ATTRS:
            np.testing.assert_allclose(np.asarray(getattr(back, a), np.float64), np.asarray(getattr(p, a), np.float64),
                                       rtol=1e-6, err_msg=a)
        # this package's own pickle (what is written where scikit-learn does not import) keeps its class
        (w / "pca_model.pkl").write_bytes(pickle.dumps(p, protocol=4))
        assert type(D.load_model(str(w))) is cls
    # PCA.from_sklearn keeps refusing what it cannot apply
    wide = P.WidePCA(0.5)
    wide._set(_attrs(16385))
    with pytest.raises(ValueError, match="VQ_VAE_z32"):
        P.PCA.from_sklearn(wide)
    assert P.WidePCA.from_sklearn(wide).n_features_in_ == 16385
