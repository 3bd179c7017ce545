"""GPU: the latent PCA kernels (csrc/pca.hip) and dynamorph_amd.pca / dim_reduction against float64 computed here and
against tests/golden/g13_pca.npz (scikit-learn's PCA(0.5) of run_dim_reduction.py:33)."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from pca_fixture import checksum, make_x  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g13():
    return load_golden("g13_pca.npz")


def _x(g, tag):
    rec = {k[len(tag) + 8:]: g[k] for k in g if k.startswith(tag + "_recipe_")}
    X = make_x(rec)
    assert checksum(X) == str(g[tag + "_sha256"])
    return X


def _data(N, F, seed):
    """fp32 data with a few strong directions, column scales 0.5 .. 2 and a 30-sigma offset."""
    g = torch.Generator().manual_seed(seed)
    r = min(8, F)
    X = torch.randn(N, r, generator=g) @ torch.randn(r, F, generator=g) + torch.randn(N, F, generator=g)
    X = X * torch.linspace(0.5, 2.0, F) + 30.0 * X.std().clamp_min(1.0)
    return X.float().to(DEV)


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


SHAPES = [(N, F) for F in (1, 15, 256, 1000, 4096) for N in (2, 777, 70001)] + [(2, 16384), (777, 16384), (5000, 16384)]


@pytest.mark.parametrize("N,F", SHAPES)
def test_colsum_and_gram_against_float64(N, F):
    from dynamorph_amd import ops
    X = _data(N, F, N * 7 + F)
    X64 = X.double()
    sums = ops.pca_colsum(X)
    want = X64.sum(0)
    assert (sums - want).abs().max().item() <= 1e-12 * X64.abs().sum(0).max().item()
    s = (sums / N).float()
    G = ops.pca_gram(X, s)
    Xc = X64 - s.double()
    G64 = Xc.T @ Xc
    gate = 1e-5 * G64.diagonal().max().item()
    assert (G - G64).abs().max().item() <= gate
    assert torch.equal(G, G.T)
    assert torch.equal(ops.pca_colsum(X), sums) and torch.equal(ops.pca_gram(X, s), G)       # bit-identical relaunches


def test_gram_strided_rows_and_accumulate():
    from dynamorph_amd import ops
    big = _data(3001, 1003, 5)
    X = big[:, 1:1001]                                  # leading dimension 1003, rows not 16-byte aligned
    s = X.double().mean(0).float()
    Xc = X.double() - s.double()
    G = ops.pca_gram(X, s)
    G64 = Xc.T @ Xc
    assert (G - G64).abs().max().item() <= 1e-5 * G64.diagonal().max().item()
    G2 = ops.pca_gram(X, s, G=G.clone(), accumulate=True)
    assert (G2 - 2 * G64).abs().max().item() <= 2e-5 * G64.diagonal().max().item()
    Y = ops.pca_transform(X, torch.eye(1000, device=DEV)[:7].contiguous(), s)
    assert (Y.double() - Xc[:, :7]).abs().max().item() <= 1e-5 * Xc.norm(dim=1).max().item()


@pytest.mark.parametrize("k", [1, 7, 64, 512])
@pytest.mark.parametrize("F", [1000, 4096])
def test_transform_against_float64(k, F):
    from dynamorph_amd import ops
    N = 1237
    X = _data(N, F, k + F)
    s = X.double().mean(0).float()
    V = torch.linalg.qr(torch.randn(F, k, dtype=torch.float64))[0].T.contiguous().float().to(DEV)
    Y = ops.pca_transform(X, V, s)
    Xc = X.double() - s.double()
    Y64 = Xc @ V.double().T
    bound = 1e-5 * Xc.norm(dim=1, keepdim=True)
    assert Y.shape == (N, k) and Y.dtype == torch.float32
    assert ((Y.double() - Y64).abs() <= bound).all()
    assert torch.equal(ops.pca_transform(X, V, s), Y)


def _check_fit(p, ref_ratio, ref_comp, n_ref):
    assert p.n_components_ == n_ref
    np.testing.assert_allclose(p.explained_variance_ratio_, ref_ratio, rtol=1e-5)
    c = _cos(p.components_, ref_comp)
    assert c.min() >= 1 - 1e-6, c


@pytest.mark.parametrize("tag", ["f4096", "f1000"])
def test_fit_and_transform_against_the_fixture(g13, tag):
    from dynamorph_amd.pca import PCA
    X = _x(g13, tag)
    Xd = torch.from_numpy(X.astype(np.float32)).to(DEV)
    p = PCA(0.5).fit(Xd)
    assert int(g13[f"{tag}_f32_n_components_"]) == int(g13[f"{tag}_f64_n_components_"])
    _check_fit(p, g13[f"{tag}_f64_explained_variance_ratio_"], g13[f"{tag}_f64_components_"],
               int(g13[f"{tag}_f64_n_components_"]))
    Y = p.transform(Xd[:64])
    assert Y.is_cuda and Y.dtype == torch.float32
    bound = 1e-5 * np.linalg.norm(X[:64] - X.mean(0), axis=1, keepdims=True)
    assert (np.abs(Y.cpu().numpy() - g13[f"{tag}_f64_transform64"]) <= bound).all()


def test_streamed_host_fit_matches_the_resident_fit(g13):
    from dynamorph_amd.pca import PCA
    X = _x(g13, "f1000").astype(np.float32)
    res = PCA(0.5).fit(torch.from_numpy(X).to(DEV))
    p = PCA(0.5, chunk_rows=1000)
    st = p.fit(X)
    _check_fit(st, res.explained_variance_ratio_, res.components_, res.n_components_)
    n1, m1, C1 = p.moments(X)
    n2, m2, C2 = p.moments(X)
    assert n1 == n2 == 3000 and torch.equal(m1, m2) and torch.equal(C1, C2)
    bound = 1e-5 * np.linalg.norm(X[:300] - X.mean(0), axis=1, keepdims=True)
    assert (np.abs(st.transform(X[:300]).cpu().numpy() - res.transform(X[:300]).cpu().numpy()) <= bound).all()


def test_fit_on_real_latents():
    from dynamorph_amd import VQ_VAE
    from dynamorph_amd.patch_vae import encode_patches
    from dynamorph_amd.pca import PCA
    g1 = load_golden("g1_state_dict.npz")
    model = VQ_VAE().to(DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in g1.items()})
    torch.manual_seed(21)
    _, z = encode_patches(model, torch.randn(4096, 2, 128, 128), device=DEV)
    Z = z.astype(np.float64)
    mu = Z.mean(0)
    C = (Z - mu).T @ (Z - mu) / (Z.shape[0] - 1)
    w, v = np.linalg.eigh(C)
    w, v = np.clip(w[::-1], 0, None), v[:, ::-1].T
    ratio = w / w.sum()
    k = int(np.searchsorted(np.cumsum(ratio), 0.5, side="right") + 1)
    p = PCA(0.5).fit(torch.from_numpy(z).to(DEV))
    assert p.n_components_ == k
    np.testing.assert_allclose(p.explained_variance_ratio_, ratio[:k], rtol=1e-5)
    # components are determined up to sign where the spectrum is separated; compare those
    gap = np.minimum(np.abs(w[:k] - w[1:k + 1]), np.abs(w[:k] - np.r_[np.inf, w[:k - 1]])) / w[:k]
    sel = gap > 1e-3
    assert sel.any()
    c = np.abs(_cos(p.components_[sel], v[:k][sel]))
    assert c.min() >= 1 - 1e-6, c


def test_pipeline_fit_and_process(tmp_path):
    from dynamorph_amd import dim_reduction as D
    rng = np.random.default_rng(9)
    dirs = [tmp_path / "A", tmp_path / "B"]
    data = {}
    for i, d in enumerate(dirs):
        d.mkdir()
        for pre in ("C5", "C6"):
            z = (rng.standard_normal((300 + 50 * i, 12)) @ rng.standard_normal((12, 256)) + 30).astype(np.float32)
            data[(d, pre)] = z
            for suffix in ("", "_after"):
                with open(d / f"{pre}_latent_space{suffix}.pkl", "wb") as f:
                    pickle.dump(z, f, protocol=4)
    weights = tmp_path / "w"
    pca = D.dim_reduction_pca([str(d) for d in dirs], None, str(weights), ["C5", "C6"], fit_model=True)
    assert (weights / "pca_model.pkl").exists()
    assert pca.n_samples_ == sum(z.shape[0] for z in data.values())
    outs = D.dim_reduction_pca([str(d) for d in dirs], [str(tmp_path / "out" / d.name) for d in dirs], str(weights),
                               ["C5", "C6"], fit_model=False)
    assert len(outs) == 4
    for d in dirs:
        for pre in ("C5", "C6"):
            path = tmp_path / "out" / d.name / f"{pre}_latent_space_after_PCAed.pkl"
            raw = path.read_bytes()
            assert raw[:2] == b"\x80\x04"
            y = pickle.loads(raw)
            z = data[(d, pre)]
            assert y.dtype == np.float32 and y.shape == (z.shape[0], pca.n_components_)
            bound = 1e-5 * np.linalg.norm(z - pca.mean_, axis=1, keepdims=True)
            assert (np.abs(y - pca.transform(z).cpu().numpy()) <= bound).all()
            try:
                import sklearn  # noqa: F401
            except ImportError:
                continue
            with open(weights / "pca_model.pkl", "rb") as f:
                sk = pickle.load(f)
            assert type(sk).__module__.startswith("sklearn")
            assert (np.abs(sk.transform(z).astype(np.float64) - y) <= 1e-5 * np.linalg.norm(z, axis=1, keepdims=True)).all()
