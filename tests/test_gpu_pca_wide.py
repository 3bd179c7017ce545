"""GPU: the sample-space ("wide") latent PCA -- dm_pca_rowgram / dm_pca_components (csrc/pca.hip) and dynamorph_amd.pca.WidePCA
/ dim_reduction -- against float64 computed here and against tests/golden/g17_pca_wide.npz (scikit-learn's PCA(0.5) of
run_dim_reduction.py:33 on latents of 16385 and 65536 features)."""
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
def g17():
    return load_golden("g17_pca_wide.npz")


def _x(g, tag):
    rec = {k[len(tag) + 8:]: g[k] for k in g if k.startswith(tag + "_recipe_")}
    X = make_x(rec)
    assert checksum(X) == str(g[tag + "_sha256"])
    return X


def _data(N, F, seed):
    """fp32 data with a few strong directions, column scales 0.5 .. 2 and a 30-sigma offset (test_gpu_pca._data, made on
    the device: the widest case here has 65 M entries)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = min(8, F)
    X = (torch.randn(N, r, generator=g, device=DEV) @ torch.randn(r, F, generator=g, device=DEV)
         + torch.randn(N, F, generator=g, device=DEV))
    X = X * torch.linspace(0.5, 2.0, F, device=DEV) + 30.0 * X.std().clamp_min(1.0)
    return X.float()


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


# The plan of dm_pca_rowgram (rowgram_plan, csrc/pca.hip) per shape; T = ceil(N / 128) row tiles, T (T + 1) / 2 tile pairs,
# ceil(F / 256) feature slabs, S feature ranges:
#   one tile pair             N = 2                                several: N = 129 (3), 257 (6), 1000 (36), 256 (3)
#   S = 1, stored directly    F = 1, 255 (one slab); (5633, 1000): 1035 tile pairs fill the part, 4 slabs in one range
#   S > 1, workspace + reduce F = 1000 (S = 4), 16385 (65 slabs: S = 33 at N = 2, ...), 65536 (256 slabs)
#   scalar loads (ld % 4)     F = 1, 255, 16385                    vector loads: F = 1000, 512, 65536
#   F no multiple of the slab 1, 255, 1000, 16385                  a multiple: 512, 65536
#   N no multiple of 128      every N but 256
# (vector loads on F & ~3 features and the scalar form on the F & 3 left over, F % 4 != 0 at ld % 4 == 0:
# test_rowgram_strided_rows_and_accumulate)
ROWGRAM_SHAPES = ([(N, F) for N in (2, 129, 257, 1000) for F in (1, 255, 1000, 16385)]
                  + [(130, 65536), (1000, 65536), (256, 512), (5633, 1000)])


@pytest.mark.parametrize("N,F", ROWGRAM_SHAPES)
def test_rowgram_against_float64(N, F):
    from dynamorph_amd import ops
    X = _data(N, F, N * 7 + F)
    s = X.double().mean(0).float()
    K = ops.pca_rowgram(X, s)
    Xc = X.double() - s.double()
    K64 = Xc @ Xc.T
    gate = 1e-5 * K64.diagonal().max().item()
    err = (K - K64).abs().max().item()
    print(f"rowgram ({N}, {F}): max error {err / K64.diagonal().max().item():.2e} of max diag")
    assert K.shape == (N, N) and K.dtype == torch.float64
    assert err <= gate
    assert torch.equal(K, K.T)
    assert torch.equal(ops.pca_rowgram(X, s), K)                           # bit-identical relaunch
    if N == 129:                                                           # shift=None: no centring
        K0 = ops.pca_rowgram(X)
        X64 = X.double()
        assert (K0 - X64 @ X64.T).abs().max().item() <= 1e-5 * (X64 * X64).sum(1).max().item()


def test_rowgram_strided_rows_and_accumulate():
    from dynamorph_amd import ops
    big = _data(301, 20004, 5)
    for lo, F in ((1, 20000), (0, 19999)):           # misaligned rows (scalar loads); aligned rows with a tail (two launches)
        X = big[:, lo:lo + F]                        # leading dimension 20004
        s = X.double().mean(0).float()
        Xc = X.double() - s.double()
        K64 = Xc @ Xc.T
        gate = 1e-5 * K64.diagonal().max().item()
        K = ops.pca_rowgram(X, s)
        assert (K - K64).abs().max().item() <= gate
        if F % 4 == 0:                               # the load form does not change the arithmetic (a tail is added last)
            assert torch.equal(K, ops.pca_rowgram(X.contiguous(), s))
        assert torch.equal(K, ops.pca_rowgram(X, s))
        # two column blocks added into one K
        cut = 16384
        K2 = ops.pca_rowgram(X[:, :cut], s[:cut].contiguous())
        K2 = ops.pca_rowgram(X[:, cut:], s[cut:].contiguous(), K=K2, accumulate=True)
        assert (K2 - K64).abs().max().item() <= 2 * gate
        assert torch.equal(K2, K2.T)
    # the direct (single range) form accumulates as well
    X = big[:, 1:201]
    Xc = X.double()
    K = ops.pca_rowgram(X)
    K = ops.pca_rowgram(X, K=K, accumulate=True)
    K64 = Xc @ Xc.T
    assert (K - 2 * K64).abs().max().item() <= 2e-5 * K64.diagonal().max().item()
    assert torch.equal(K, K.T)


@pytest.mark.parametrize("k", [1, 9, 64, 65, 512])
@pytest.mark.parametrize("F", [1000, 16385])
def test_components_against_float64(k, F):
    from dynamorph_amd import ops
    N = 1237
    X = _data(N, F, k + F)
    s = X.double().mean(0).float()
    g = torch.Generator().manual_seed(k)
    W = (torch.randn(k, N, generator=g) / N ** 0.5).to(DEV)
    V = ops.pca_components(X, W, s)
    Xc = X.double() - s.double()
    V64 = W.double() @ Xc
    bound = 1e-5 * W.double().norm(dim=1, keepdim=True) * Xc.norm(dim=0, keepdim=True)      # Cauchy-Schwarz scale per entry
    assert V.shape == (k, F) and V.dtype == torch.float64
    print(f"components k={k} F={F}: max error / bound {((V - V64).abs() / bound).max().item():.2e}")
    assert ((V - V64).abs() <= bound).all()
    assert torch.equal(ops.pca_components(X, W, s), V)
    if k == 9:                                       # misaligned, strided rows: the scalar-load form
        Xs = X[:, 1:F - 2]
        Vs = ops.pca_components(Xs, W, s[1:F - 2].contiguous())
        assert ((Vs - V64[:, 1:F - 2]).abs() <= bound[:, 1:F - 2]).all()


def _check_fit(p, g, tag):
    assert p.n_components_ == int(g[f"{tag}_f64_n_components_"]) == int(g[f"{tag}_f32_n_components_"])
    np.testing.assert_allclose(p.explained_variance_ratio_, g[f"{tag}_f64_explained_variance_ratio_"], rtol=1e-5)
    np.testing.assert_allclose(p.explained_variance_, g[f"{tag}_f64_explained_variance_"], rtol=1e-5)
    np.testing.assert_allclose(p.singular_values_, g[f"{tag}_f64_singular_values_"], rtol=1e-5)
    np.testing.assert_allclose(p.noise_variance_, float(g[f"{tag}_f64_noise_variance_"]), rtol=1e-5)
    np.testing.assert_allclose(p.mean_, g[f"{tag}_f64_mean_"], rtol=1e-12)
    V = np.asarray(p.components_, np.float64)
    gram = V @ V.T
    assert np.abs(np.diag(gram) - 1).max() <= 1e-6
    assert np.abs(gram - np.diag(np.diag(gram))).max() <= 1e-5
    if f"{tag}_f64_components_" in g:
        c = _cos(V, g[f"{tag}_f64_components_"])
        assert c.min() >= 1 - 1e-6, c


@pytest.fixture(scope="module")
def fitted(g17):
    """The resident fit of each tag, made once: (X float64, X on the device, the fitted WidePCA)."""
    from dynamorph_amd.pca import WidePCA
    out = {}
    for tag in ("f16385", "f65536"):
        X = _x(g17, tag)
        Xd = torch.from_numpy(X.astype(np.float32)).to(DEV)
        out[tag] = (X, Xd, WidePCA(0.5).fit(Xd))
    return out


@pytest.mark.parametrize("tag", ["f16385", "f65536"])
def test_fit_and_transform_against_the_fixture(g17, fitted, tag):
    X, Xd, p = fitted[tag]
    _check_fit(p, g17, tag)
    assert p.n_samples_ == X.shape[0] and p.n_features_in_ == X.shape[1]
    Y = p.transform(Xd[:64])
    assert Y.is_cuda and Y.dtype == torch.float32 and tuple(Y.shape) == (64, p.n_components_)
    bound = 1e-5 * np.linalg.norm(X[:64] - X.mean(0), axis=1, keepdims=True)
    err = np.abs(Y.cpu().numpy() - g17[f"{tag}_f64_transform64"])
    print(f"{tag}: transform error / bound {(err / bound).max():.2e}")
    assert (err <= bound).all()
    assert torch.equal(p.transform(X[:64]), Y)                              # host rows: the same kernels on the same numbers


def test_host_array_fit_equals_the_resident_fit(g17, fitted):
    from dynamorph_amd.pca import WidePCA
    X, Xd, res = fitted["f16385"]
    for host in (X.astype(np.float32), X, torch.from_numpy(X.astype(np.float32)).pin_memory()):
        p = WidePCA(0.5, chunk_rows=100)
        Y = p.fit_transform(host)
        assert np.array_equal(p.explained_variance_, res.explained_variance_)
        assert np.array_equal(p.components_, res.components_)
        assert np.array_equal(p.mean_, res.mean_)
        assert torch.equal(Y, res.transform(Xd))


def test_wide_route_against_the_covariance_route():
    from dynamorph_amd.pca import PCA, WidePCA
    g13 = load_golden("g13_pca.npz")
    X = _x(g13, "f4096")
    assert X.shape == (3000, 4096)
    Xd = torch.from_numpy(X.astype(np.float32)).to(DEV)
    cov = PCA(0.5).fit(Xd)
    wide = WidePCA(0.5).fit(Xd)
    assert wide.n_components_ == cov.n_components_ == int(g13["f4096_f64_n_components_"])
    np.testing.assert_allclose(wide.explained_variance_ratio_, cov.explained_variance_ratio_, rtol=1e-5)
    np.testing.assert_allclose(wide.noise_variance_, cov.noise_variance_, rtol=1e-5)
    c = _cos(wide.components_, cov.components_)
    assert c.min() >= 1 - 1e-6, c
    bound = 1e-5 * np.linalg.norm(X[:64] - X.mean(0), axis=1, keepdims=True)
    assert (np.abs(wide.transform(Xd[:64]).cpu().numpy() - g13["f4096_f64_transform64"]) <= bound).all()


def test_fit_on_real_z32_latents():
    import dynamorph_amd
    from dynamorph_amd.patch_vae import encode_patches
    from dynamorph_amd.pca import WidePCA
    torch.manual_seed(21)
    model = dynamorph_amd.VQ_VAE_z32(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512).to(DEV)
    _, z = encode_patches(model, torch.randn(96, 2, 128, 128), device=DEV)
    assert z.shape == (96, 65536) and z.dtype == np.float32
    Z = z.astype(np.float64)
    Zc = Z - Z.mean(0)
    w, u = np.linalg.eigh(Zc @ Zc.T)
    w, u = np.clip(w[::-1], 0, None), u[:, ::-1]
    ratio = w / w.sum()
    k = int(np.searchsorted(np.cumsum(ratio), 0.5, side="right") + 1)
    p = WidePCA(0.5).fit(torch.from_numpy(z).to(DEV))
    assert p.n_components_ == k
    np.testing.assert_allclose(p.explained_variance_ratio_, ratio[:k], rtol=1e-5)
    np.testing.assert_allclose(p.explained_variance_, w[:k] / 95, rtol=1e-5)
    v = (u[:, :k] / np.sqrt(w[:k])).T @ Zc
    # components are determined up to sign where the spectrum is separated; compare those
    gap = np.minimum(np.abs(w[:k] - w[1:k + 1]), np.abs(w[:k] - np.r_[np.inf, w[:k - 1]])) / w[:k]
    sel = gap > 1e-3
    assert sel.any()
    c = np.abs(_cos(p.components_[sel], v[sel]))
    assert c.min() >= 1 - 1e-6, c
    Y = p.transform(z[:16]).cpu().numpy()
    want = Zc[:16] @ p.components_.T
    assert (np.abs(Y - want) <= 1e-5 * np.linalg.norm(Zc[:16], axis=1, keepdims=True)).all()


def test_pipeline_fit_and_process(tmp_path):
    from dynamorph_amd import dim_reduction as D
    from dynamorph_amd.pca import WidePCA
    rng = np.random.default_rng(9)
    dirs = [tmp_path / "A", tmp_path / "B"]
    data = {}
    for i, d in enumerate(dirs):
        d.mkdir()
        for pre in ("C5", "C6"):
            z = (rng.standard_normal((120 + 10 * i, 12)) @ rng.standard_normal((12, 16400)) + 30).astype(np.float32)
            data[(d, pre)] = z
            for suffix in ("", "_after"):
                with open(d / f"{pre}_latent_space{suffix}.pkl", "wb") as f:
                    pickle.dump(z, f, protocol=4)
    weights = tmp_path / "w"
    pca = D.dim_reduction_pca([str(d) for d in dirs], None, str(weights), ["C5", "C6"], fit_model=True)
    assert type(pca) is WidePCA and (weights / "pca_model.pkl").exists()
    assert pca.n_samples_ == sum(z.shape[0] for z in data.values()) == 500 and pca.n_features_in_ == 16400
    assert type(D.load_model(str(weights))) is WidePCA
    outs = D.dim_reduction_pca([str(d) for d in dirs], [str(tmp_path / "out" / d.name) for d in dirs], str(weights),
                               ["C5", "C6"], fit_model=False)
    assert len(outs) == 4
    try:
        import sklearn  # noqa: F401
        with open(weights / "pca_model.pkl", "rb") as f:
            sk = pickle.load(f)
        assert type(sk).__module__.startswith("sklearn")
    except ImportError:
        sk = None
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
            if sk is not None:
                assert (np.abs(sk.transform(z).astype(np.float64) - y) <= 1e-5 * np.linalg.norm(z, axis=1, keepdims=True)).all()


def test_duplicate_rows_give_a_finite_fit_with_the_float64_count():
    from dynamorph_amd.pca import WidePCA
    X = _data(60, 16400, 3)
    X[30:] = X[:30]                                     # rank <= 29 after centring
    Z = X.double().cpu().numpy()
    Zc = Z - Z.mean(0)
    w = np.clip(np.linalg.eigvalsh(Zc @ Zc.T)[::-1], 0, None)
    k = int(np.searchsorted(np.cumsum(w / w.sum()), 0.5, side="right") + 1)
    p = WidePCA(0.5).fit(X)
    assert p.n_components_ == k
    for a in ("components_", "explained_variance_", "explained_variance_ratio_", "singular_values_", "mean_"):
        assert np.isfinite(getattr(p, a)).all(), a
    assert np.isfinite(p.noise_variance_) and torch.isfinite(p.transform(X)).all()
    np.testing.assert_allclose(p.explained_variance_, w[:k] / 59, rtol=1e-5)
    with pytest.raises(ValueError, match="components are defined"):
        WidePCA(None).fit(X)
