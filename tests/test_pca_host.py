"""`not gpu`: the host half of the latent PCA (dynamorph_amd/pca.py) -- finalisation from a float64 covariance, the Chan
merge, the component-count rule, argument refusal before any device call, the C ABI's argument errors and the scikit-learn
interchange -- against tests/golden/g13_pca.npz (PCA(0.5) of run_dim_reduction.py:33 on planted-spectrum latents)."""
import ctypes
import os
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
def g13():
    return load_golden("g13_pca.npz")


def _x(g, tag):
    rec = {k[len(tag) + 8:]: g[k] for k in g if k.startswith(tag + "_recipe_")}
    X = make_x(rec)
    assert checksum(X) == str(g[tag + "_sha256"])
    return X


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


@pytest.mark.parametrize("tag", ["f4096", "f1000"])
def test_finalize_reproduces_scikit_learn(g13, tag):
    X = _x(g13, tag)
    mu = X.mean(0)
    Xc = X - mu
    C = torch.from_numpy(Xc.T @ Xc)
    fit = P.finalize(C, torch.from_numpy(mu), X.shape[0], 0.5)
    for prec, ev_tol, cos_tol in (("f64", 1e-9, 1e-12), ("f32", 1e-5, 1e-6)):
        assert str(g13[f"{tag}_{prec}_solver"]) == "full"
        k = int(g13[f"{tag}_{prec}_n_components_"])
        assert fit["n_components_"] == k
        ev = g13[f"{tag}_{prec}_explained_variance_"].astype(np.float64)
        np.testing.assert_allclose(fit["explained_variance_"], ev, rtol=ev_tol)
        np.testing.assert_allclose(fit["explained_variance_ratio_"], g13[f"{tag}_{prec}_explained_variance_ratio_"],
                                   rtol=ev_tol)
        np.testing.assert_allclose(fit["singular_values_"], g13[f"{tag}_{prec}_singular_values_"], rtol=ev_tol)
        np.testing.assert_allclose(fit["noise_variance_"], float(g13[f"{tag}_{prec}_noise_variance_"]), rtol=ev_tol * 100)
        c = _cos(fit["components_"], g13[f"{tag}_{prec}_components_"])
        assert c.min() >= 1 - cos_tol, c                     # >= 1 - tol: the same sign as well
        np.testing.assert_allclose(fit["mean_"], g13[f"{tag}_{prec}_mean_"], rtol=1e-5 if prec == "f32" else 1e-13)
    assert fit["n_samples_"] == X.shape[0] and fit["n_features_in_"] == X.shape[1]


def test_chan_merge_of_uneven_chunks_is_the_one_shot_covariance():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((1001, 37)) * rng.uniform(0.1, 5, 37) + 30.0
    mu = X.mean(0)
    want = (X - mu).T @ (X - mu)
    C = torch.zeros((37, 37), dtype=torch.float64)
    n, mean = 0, None
    for lo, hi in ((0, 1), (1, 400), (400, 401), (401, 1001)):
        x = X[lo:hi]
        mc = x.mean(0)
        C += torch.from_numpy((x - mc).T @ (x - mc))
        n, mean = P.merge_moments(n, mean, C, hi - lo, torch.from_numpy(mc))
    assert n == 1001
    np.testing.assert_allclose(mean.numpy(), mu, rtol=1e-14)
    assert np.abs(C.numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_selection_rule_matches_scikit_learn_at_the_boundaries():
    sk = pytest.importorskip("sklearn.decomposition")
    rng = np.random.default_rng(5)
    X = rng.standard_normal((200, 12)) * np.linspace(4, 0.5, 12)
    full = sk.PCA(None, svd_solver="full").fit(X)
    cum = np.cumsum(full.explained_variance_ratio_)
    for i in range(len(cum) - 1):
        for t in (cum[i], np.nextafter(cum[i], 0), np.nextafter(cum[i], 1), cum[i] - 1e-9, cum[i] + 1e-9):
            if not 0 < t < 1:
                continue
            want = sk.PCA(float(t), svd_solver="full").fit(X).n_components_
            assert P.select_n_components(float(t), full.explained_variance_ratio_, 200, 12) == want, (i, t)
    assert P.select_n_components(None, full.explained_variance_ratio_, 200, 12) == 12
    assert P.select_n_components(3, full.explained_variance_ratio_, 200, 12) == 3


def test_refused_arguments_raise_before_any_device_call(monkeypatch):
    from dynamorph_amd import ops

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    for name in ("pca_colsum", "pca_gram", "pca_transform"):
        monkeypatch.setattr(ops, name, no_device)
    with pytest.raises(ValueError, match="whiten"):
        P.PCA(0.5, whiten=True)
    with pytest.raises(ValueError, match="mle"):
        P.PCA("mle")
    with pytest.raises(ValueError, match="at least 2 samples"):
        P.PCA(0.5).fit(np.zeros((1, 8), np.float32))
    with pytest.raises(ValueError, match="VQ_VAE_z32.*65536"):
        P.PCA(0.5).fit(np.zeros((2, 65536), np.float32))
    with pytest.raises(ValueError):
        P.PCA(1.5)
    with pytest.raises(ValueError):
        P.PCA(0)
    with pytest.raises(ValueError, match="VQ_VAE_z32"):
        P.finalize(torch.zeros((16385, 1), dtype=torch.float64), torch.zeros(16385), 4)


def test_cabi_pca_argument_errors_are_reported_before_any_launch():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    lib = _lib.load()
    assert lib.dm_pca_colsum(None, 10, 4, 4, None, None, 0, None) == -1 and b"NULL" in lib.dm_last_error()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host checks
    assert lib.dm_pca_colsum(fake, 10, 0, 4, fake, fake, 1 << 20, None) == -1 and b"features" in lib.dm_last_error()
    assert lib.dm_pca_colsum(fake, 10, 16385, 16385, fake, fake, 1 << 30, None) == -1
    assert lib.dm_pca_colsum(fake, 10, 8, 4, fake, fake, 1 << 20, None) == -1 and b"leading dimension" in lib.dm_last_error()
    assert lib.dm_pca_colsum(fake, 10, 8, 8, fake, fake, 8, None) == -1 and b"workspace" in lib.dm_last_error()
    assert lib.dm_pca_gram(fake, 0, 8, 8, None, fake, 0, fake, 1 << 30, None) == -1 and b"rows" in lib.dm_last_error()
    assert lib.dm_pca_gram(fake, 10, 8, 8, None, None, 0, fake, 1 << 30, None) == -1 and b"NULL" in lib.dm_last_error()
    assert lib.dm_pca_gram(fake, 10, 8, 8, None, fake, 0, fake, 16, None) == -1 and b"workspace" in lib.dm_last_error()
    assert lib.dm_pca_transform(fake, 10, 8, 8, None, fake, 0, fake, None) == -1 and b"components" in lib.dm_last_error()
    assert lib.dm_pca_transform(fake, 10, 8, 8, None, fake, 513, fake, None) == -1
    assert lib.dm_pca_transform(fake, 10, 8, 8, None, None, 4, fake, None) == -1 and b"NULL" in lib.dm_last_error()
    assert lib.dm_pca_gram_workspace_bytes(1, 1) == 128 * 128 * 8
    assert lib.dm_pca_gram_workspace_bytes(1, 16385) == -1 and lib.dm_pca_colsum_workspace_bytes(0, 4) == -1


def _fitted(g, tag="f1000"):
    p = P.PCA(0.5)
    p._set({"mean_": g[f"{tag}_f64_mean_"], "components_": g[f"{tag}_f64_components_"],
            "explained_variance_": g[f"{tag}_f64_explained_variance_"],
            "explained_variance_ratio_": g[f"{tag}_f64_explained_variance_ratio_"],
            "singular_values_": g[f"{tag}_f64_singular_values_"],
            "noise_variance_": float(g[f"{tag}_f64_noise_variance_"]), "n_components_": int(g[f"{tag}_f64_n_components_"]),
            "n_samples_": 3000, "n_features_in_": 1000})
    return p


def test_sklearn_round_trip_keeps_every_attribute(g13, tmp_path):
    pytest.importorskip("sklearn.decomposition")
    import pickle
    p = _fitted(g13)
    for dtype, rtol in ((np.float64, 0), (np.float32, 1e-7)):
        sk = p.to_sklearn(dtype=dtype)
        assert sk.n_components == 0.5 and sk.svd_solver == "auto" and sk.whiten is False
        path = tmp_path / "pca_model.pkl"
        path.write_bytes(pickle.dumps(sk, protocol=4))
        back = P.PCA.from_sklearn(pickle.loads(path.read_bytes()))
        for a in P._ATTRS:
            np.testing.assert_allclose(np.asarray(getattr(back, a), np.float64), np.asarray(getattr(p, a), np.float64),
                                       rtol=rtol, err_msg=a)
        X = _x(g13, "f1000")[:64]
        # the transform gate per row; scikit-learn's own float32 transform (X @ V^T - mean @ V^T) cancels at |x|
        bound = (1e-5 * np.linalg.norm(X - p.mean_, axis=1) if dtype is np.float64 else 1e-6 * np.linalg.norm(X, axis=1))
        err = np.abs(sk.transform(X.astype(dtype)) - g13["f1000_f64_transform64"]).max(1)
        assert (err <= bound).all(), (err / bound).max()
    # this package's PCA pickles with its state on the host
    q = pickle.loads(pickle.dumps(p, protocol=4))
    for a in P._ATTRS:
        np.testing.assert_array_equal(np.asarray(getattr(q, a)), np.asarray(getattr(p, a)))
