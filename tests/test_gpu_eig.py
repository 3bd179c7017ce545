"""GPU: dm_eig_apply (csrc/eig.hip) against exact integer arithmetic, the partial eigensolver dynamorph_amd.eig on the device
against numpy.linalg.eigh (gates: tests/helpers/eig_cases.py), and the PCA fits with eigensolver="partial" against the
committed scikit-learn fixtures."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import eig_cases as EC  # noqa: E402
from pca_fixture import checksum, make_x  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _views(A, Q, aligned):
    """The operands as row views of larger NaN-filled buffers: lda > n, ldq > b, ldy > b.  aligned: A's rows start on 16
    bytes and lda is even (the kernel's paired loads); otherwise lda = n + 3 from an odd element offset (single loads)."""
    n, b = Q.shape
    lda, off = (n + n % 2 + 2, 0) if aligned else (n + 3, 1)
    bufa = torch.full((n, lda), float("nan"), dtype=torch.float64, device=DEV)
    bufq = torch.full((n, b + 5), float("nan"), dtype=torch.float64, device=DEV)
    bufy = torch.full((n + 2, b + 7), float("nan"), dtype=torch.float64, device=DEV)
    av, qv, yv = bufa[:, off:off + n], bufq[:, 2:2 + b], bufy[1:n + 1, 3:3 + b]
    av.copy_(A)
    qv.copy_(Q)
    return av, qv, yv, bufy


def _untouched(bufy, n, b):
    mask = torch.ones_like(bufy, dtype=torch.bool)
    mask[1:n + 1, 3:3 + b] = False
    return bool(torch.isnan(bufy[mask]).all())


# ------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("n", EC.APPLY_N)
def test_apply_is_exact_on_integers(n):
    """A (integers in [-8, 8], NOT symmetric: a transposed index shows) times Q (integers in [-4, 4]): every partial sum is
    an integer below 2^53, so Y must equal the int64 product in every bit, whatever the order of the sums."""
    from dynamorph_amd import ops
    g = torch.Generator().manual_seed(1000 + n)
    A = torch.randint(-8, 9, (n, n), generator=g)
    assert n < 4 or not torch.equal(A, A.T)
    for b in EC.APPLY_B:
        Q = torch.randint(-4, 5, (n, b), generator=g)
        want = (A @ Q).double()
        tiles, splits, rows, stage = ops.eig_plan(n, b)
        assert tiles == -(-n // rows) and stage == (32 if b <= 64 else 16)
        assert (splits > 1) == (n >= 257), (n, b, splits)            # both paths are among the shapes (257, 512, 1030)
        for aligned in (True, False):
            av, qv, yv, bufy = _views(A.double().to(DEV), Q.double().to(DEV), aligned)
            out = ops.eig_apply(av, qv, out=yv)
            assert out.data_ptr() == yv.data_ptr()
            assert torch.equal(yv.cpu(), want), (n, b, aligned, (yv.cpu() - want).abs().max().item())
            assert _untouched(bufy, n, b), (n, b, aligned)
        assert torch.equal(ops.eig_apply(A.double().to(DEV), Q.double().to(DEV)).cpu(), want)


def _full_mantissa(rng, shape):
    """(float64 array, the same numbers as Python integers scaled by 2^8): 53-bit mantissas, either sign, exponents -8 .. 8."""
    m = rng.integers(1 << 52, 1 << 53, size=shape, dtype=np.int64) * rng.choice(np.array([-1, 1], dtype=np.int64), size=shape)
    e = rng.integers(-8, 9, size=shape)
    val = np.ldexp(m.astype(np.float64), e)
    ints = np.empty(shape, dtype=object)
    for idx in np.ndindex(*shape):
        ints[idx] = int(m[idx]) << int(e[idx] + 8)
    return val, ints


@pytest.mark.parametrize("n", [17, 129, 257])
@pytest.mark.parametrize("b", [16, 48])
def test_apply_rounding_against_exact_integers(n, b):
    """Full-mantissa operands of mixed magnitude.  The reference is exact: Python integers on the values scaled by 2^8 (the
    products by 2^16).  Gate: |Y - Y_ref| <= (n + 1) 2^-53 (|A| |Q|) elementwise -- n float64 products summed in any order
    -- evaluated in integers as well."""
    from dynamorph_amd import ops
    rng = np.random.default_rng(n * 100 + b)
    A, Ai = _full_mantissa(rng, (n, n))
    Q, Qi = _full_mantissa(rng, (n, b))
    ref = Ai.dot(Qi)                                            # exact, scaled by 2^16
    mag = np.abs(Ai).dot(np.abs(Qi))
    Y = ops.eig_apply(torch.from_numpy(A).to(DEV), torch.from_numpy(Q).to(DEV)).cpu().numpy()
    worst = 0.0
    for idx in np.ndindex(n, b):
        y = math.ldexp(float(Y[idx]), 16)
        assert y == int(y)                                      # (every partial sum is a multiple of 2^-16)
        err = abs(int(y) - ref[idx])
        assert (err << 53) <= (n + 1) * mag[idx], (idx, err, mag[idx])
        worst = max(worst, err * 2.0 ** 53 / mag[idx])
    print(f"n = {n}, b = {b}: worst error {worst:.2f} of the bound's {n + 1} units")


@pytest.mark.parametrize("n,b", [(129, 48), (1030, 16), (1030, 256), (600, 32)])
def test_apply_relaunch_and_layout_do_not_change_a_bit(n, b):
    from dynamorph_amd import ops
    g = torch.Generator().manual_seed(n + b)
    A = torch.randn(n, n, generator=g, dtype=torch.float64).to(DEV)
    Q = torch.randn(n, b, generator=g, dtype=torch.float64).to(DEV)
    Y = ops.eig_apply(A, Q)
    ws = ops.eig_workspace(n, b, A)
    for _ in range(3):
        assert torch.equal(ops.eig_apply(A, Q, workspace=ws), Y)
    for aligned in (True, False):
        av, qv, yv, bufy = _views(A, Q, aligned)
        assert torch.equal(ops.eig_apply(av, qv, out=yv), Y) and _untouched(bufy, n, b)
    ref = A @ Q
    assert ((Y - ref).abs() <= (n + 1) * 2.0 ** -52 * (A.abs() @ Q.abs())).all()


def test_apply_refuses_bad_operands():
    from dynamorph_amd import ops
    A = torch.zeros((40, 40), dtype=torch.float64, device=DEV)
    Q = torch.zeros((40, 32), dtype=torch.float64, device=DEV)
    for bad in ((A, Q[:, :24]), (A, Q[:39]), (A[:, :39], Q), (A.float(), Q), (A, Q.T.contiguous().T), (A.cpu(), Q)):
        with pytest.raises(ValueError):
            ops.eig_apply(*bad)
    with pytest.raises(ValueError):
        ops.eig_apply(A, Q, out=torch.zeros((40, 16), dtype=torch.float64, device=DEV))


# ---------------------------------------------------------------------------------------------- the solver on the device
@pytest.mark.parametrize("name,block,groups", [("a", 64, ()), ("b", 64, ()), ("c", 32, ((8, 9),)), ("d", 256, ())])
def test_spectra_on_the_device(name, block, groups):
    from dynamorph_amd import eig
    lam, kw, k = EC.spectrum(name)
    A = EC.planted(lam)
    theta, V, info = eig.top_eigenpairs(torch.from_numpy(A).to(DEV), **kw)
    print(f"({name}): k {len(theta)}, block {info['block']}, applies {info['applies']}, "
          f"max residual {info['residual'].max() / float(theta[0]):.2e} theta_1")
    assert theta.is_cuda and V.is_cuda and len(theta) == k and info["block"] == block and info["applies"] <= 400
    EC.check_pairs(A, theta.cpu().numpy(), V.cpu().numpy(), info, groups)


def test_block_grown_to_the_whole_matrix_on_the_device():
    """n = 100: the block grows 32 -> 64 -> 100, which the kernel takes as 112 columns with twelve of zeros; the
    Rayleigh-Ritz step of a block of n columns is the exact decomposition."""
    from dynamorph_amd import eig
    A = EC.planted(1.0 / np.arange(1, 101))
    theta, V, info = eig.top_eigenpairs(torch.from_numpy(A).to(DEV), fraction=0.9)
    w = np.linalg.eigvalsh(A)[::-1]
    k = int(np.searchsorted(np.cumsum(w) / np.trace(A), 0.9, side="right") + 1)
    assert info["block"] == 100 and len(theta) == k
    EC.check_pairs(A, theta.cpu().numpy(), V.cpu().numpy(), info, angles=False)


# ------------------------------------------------------------------------------------------------------- the fits
def _x(g, tag):
    rec = {k[len(tag) + 8:]: g[k] for k in g if k.startswith(tag + "_recipe_")}
    X = make_x(rec)
    assert checksum(X) == str(g[tag + "_sha256"])
    return X


def _cos(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


def _check_fit(p, g, tag, X, Xd):
    """The gates of tests/test_gpu_pca.py and tests/test_gpu_pca_wide.py, and the route taken."""
    assert p.eigensolver_ == "partial" and p.eig_info_["applies"] <= 400
    assert p.n_components_ == int(g[f"{tag}_f64_n_components_"])
    np.testing.assert_allclose(p.explained_variance_ratio_, g[f"{tag}_f64_explained_variance_ratio_"], rtol=1e-5)
    np.testing.assert_allclose(p.explained_variance_, g[f"{tag}_f64_explained_variance_"], rtol=1e-5)
    np.testing.assert_allclose(p.singular_values_, g[f"{tag}_f64_singular_values_"], rtol=1e-5)
    np.testing.assert_allclose(p.noise_variance_, float(g[f"{tag}_f64_noise_variance_"]), rtol=1e-5)
    np.testing.assert_allclose(p.mean_, g[f"{tag}_f64_mean_"], rtol=1e-12)
    V = np.asarray(p.components_, np.float64)
    gram = V @ V.T
    assert np.abs(np.diag(gram) - 1).max() <= 1e-6 and np.abs(gram - np.diag(np.diag(gram))).max() <= 1e-5
    if f"{tag}_f64_components_" in g:
        assert _cos(V, g[f"{tag}_f64_components_"]).min() >= 1 - 1e-6
    Y = p.transform(Xd[:64])
    bound = 1e-5 * np.linalg.norm(X[:64] - X.mean(0), axis=1, keepdims=True)
    assert (np.abs(Y.cpu().numpy() - g[f"{tag}_f64_transform64"]) <= bound).all()


@pytest.mark.parametrize("tag", ["f4096", "f1000"])
def test_pca_fit_with_the_partial_solver(tag):
    from dynamorph_amd.pca import PCA
    g = load_golden("g13_pca.npz")
    X = _x(g, tag)
    Xd = torch.from_numpy(X.astype(np.float32)).to(DEV)
    _check_fit(PCA(0.5, eigensolver="partial").fit(Xd), g, tag, X, Xd)
    assert PCA(0.5).fit(Xd).eigensolver_ == "full"


@pytest.mark.parametrize("tag", ["f16385", "f65536"])
def test_wide_pca_fit_with_the_partial_solver(tag):
    from dynamorph_amd.pca import WidePCA
    g = load_golden("g17_pca_wide.npz")
    X = _x(g, tag)
    Xd = torch.from_numpy(X.astype(np.float32)).to(DEV)
    _check_fit(WidePCA(0.5, eigensolver="partial").fit(Xd), g, tag, X, Xd)


@pytest.mark.parametrize("N,F,route", [(500, 64, "full"), (300, 16385, "partial")])
def test_pca_init_with_the_partial_solver(N, F, route):
    """The two scores of init="pca" against a float64 host SVD of the centred data, signed by svd_flip(u_based_decision=False).
    (N = 500, F = 64: a covariance of order 64 = 2 x block takes the full route, as documented.)"""
    from dynamorph_amd import pca as P
    from dynamorph_amd.umap_layout import pca_init
    rng = np.random.default_rng(N + F)
    X = (rng.standard_normal((N, 4)) * np.array([9.0, 6.0, 3.0, 2.0])) @ rng.standard_normal((4, F)) / np.sqrt(F)
    X = (X + 0.1 * rng.standard_normal((N, F)) + 5.0).astype(np.float32)
    Xd = torch.from_numpy(X).to(DEV)
    Y = pca_init(Xd, eigensolver="partial")
    assert Y.is_cuda and Y.dtype == torch.float32 and tuple(Y.shape) == (N, 2)
    X64 = X.astype(np.float64)
    Xc = X64 - X64.mean(0)
    Vt = np.linalg.svd(Xc, full_matrices=False)[2][:2]
    Vt *= np.sign(Vt[np.arange(2), np.abs(Vt).argmax(1)])[:, None]
    bound = 1e-5 * np.linalg.norm(Xc, axis=1, keepdims=True)
    assert (np.abs(Y.cpu().numpy() - Xc @ Vt.T) <= bound).all()
    p = (P.WidePCA if F > P.MAX_FEATURES else P.PCA)(2, eigensolver="partial").fit(Xd)
    assert p.eigensolver_ == route
