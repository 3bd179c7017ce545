"""`not gpu`: the host half of the partial eigensolver -- dm_eig_apply's argument errors before any launch, its plan, the
deterministic start block, the driver dynamorph_amd.eig.top_eigenpairs on CPU tensors against numpy.linalg.eigh (gates:
tests/helpers/eig_cases.py), and pca.finalize / finalize_samples with eigensolver="partial" against the scikit-learn fixture."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import eig_cases as EC  # noqa: E402
from pca_fixture import checksum, make_x  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    return _lib.load()


def _plan(lib, n, b):
    out = [ctypes.c_int(-1) for _ in range(4)]
    assert lib.dm_eig_apply_plan(n, b, *[ctypes.addressof(o) for o in out]) == 0, lib.dm_last_error()
    return tuple(o.value for o in out)          # row_tiles, splits, tile_rows, stage


# ------------------------------------------------------------------------------------------------ the C entry points
def test_dm_eig_apply_argument_errors_before_any_launch(lib):
    """Every refusal is made on the host (-1, dm_last_error text); the pointers are never dereferenced."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255        # a 256-byte aligned host address standing in for device memory
    need = lib.dm_eig_apply_workspace_bytes(100, 32)
    assert need > 0

    def apply(A=p, n=100, lda=100, Q=p, b=32, ldq=32, Y=p, ldy=32, ws=p, ws_bytes=need):
        return lib.dm_eig_apply(A, n, lda, Q, b, ldq, Y, ldy, ws, ws_bytes, None)

    cases = [(dict(A=None), b"NULL"), (dict(Q=None), b"NULL"), (dict(Y=None), b"NULL"), (dict(ws=None), b"NULL"),
             (dict(n=0, lda=1), b"n outside"), (dict(lda=99), b"leading dimension of A"),
             (dict(ldq=31), b"leading dimension of Q"), (dict(ldy=31), b"leading dimension of Y"),
             (dict(ws_bytes=need - 1), b"workspace of"), (dict(ws=p + 8), b"aligned")]
    cases += [(dict(b=b, ldq=512, ldy=512), b"multiple of 16") for b in (0, 8, 24, 272)]
    for kw, text in cases:
        rc = apply(**kw)
        assert rc == -1 and b"dm_eig_apply" in lib.dm_last_error() and text in lib.dm_last_error(), (kw, rc, lib.dm_last_error())
    from dynamorph_amd import _lib
    with pytest.raises(ValueError, match="dm_eig_apply"):
        _lib.check(apply(b=24), "dm_eig_apply")


def test_dm_eig_apply_workspace_bytes(lib):
    for n in (1, 17, 24576):
        w = lib.dm_eig_apply_workspace_bytes(n, 256)
        assert w > 0 and w % 256 == 0, (n, w)
    for bad in ((0, 32), (-3, 32), (1 << 31, 32), (100, 0), (100, 8), (100, 24), (100, 272), (100, -16)):
        assert lib.dm_eig_apply_workspace_bytes(*bad) == -1, bad
        assert lib.dm_eig_apply_plan(*bad, None, None, None, None) == -1 and b"dm_eig_apply_plan" in lib.dm_last_error()


def test_plan_depends_on_the_shape_alone(lib):
    seen = set()
    for n in EC.APPLY_N + (4096, 8192, 20000, 24576):
        for b in EC.APPLY_B + (32, 64, 80):
            tiles, splits, rows, stage = _plan(lib, n, b)
            assert _plan(lib, n, b) == (tiles, splits, rows, stage)
            assert tiles * rows >= n > (tiles - 1) * rows and splits >= 1
            assert stage in (16, 32) and rows % 16 == 0
            ws = lib.dm_eig_apply_workspace_bytes(n, b)
            assert ws >= (splits * n * b * 8 if splits > 1 else 1)
            if n in EC.APPLY_N:
                seen.add(splits > 1)
            if n >= 4096:                           # enough workgroups for a 256-CU part, never more ranges than that needs
                assert 256 <= tiles * splits <= 1024, (n, b, tiles, splits)
    assert seen == {False, True}                    # the GPU test's shapes take both paths
    assert _plan(lib, 64, 16)[1] == 1 and _plan(lib, 257, 16)[1] > 1 and _plan(lib, 1030, 256)[1] > 1


# --------------------------------------------------------------------------------------------------- the start block
def test_start_block():
    from dynamorph_amd import eig
    from dynamorph_amd.umap_layout import counter_word
    a = eig.start_block(300, 32, seed=5)
    assert a.dtype == np.float64 and a.shape == (300, 32)
    assert np.array_equal(a, eig.start_block(300, 32, seed=5))
    assert a.min() >= -1.0 and a.max() < 1.0 and not np.array_equal(a, eig.start_block(300, 32, seed=6))
    big = eig.start_block(300, 64, seed=5)
    assert np.array_equal(big[:, :32], a)
    assert np.array_equal(eig.start_block(300, 32, seed=5, first=32), big[:, 32:])
    assert a[7, 3] == float(int(counter_word(5, 3, 7, 0)) >> 11) / 2.0 ** 52 - 1.0
    assert abs(a.mean()) < 0.02 and abs(a.std() - 3 ** -0.5) < 0.02      # uniform on [-1, 1)


# --------------------------------------------------------------------------------------- the driver on CPU tensors
@pytest.mark.parametrize("name,block,groups", [("a", 64, ()), ("b", 64, ()), ("c", 32, ((8, 9),)), ("d", 256, ())])
def test_driver_against_numpy_eigh(name, block, groups):
    from dynamorph_amd import eig
    lam, kw, k = EC.spectrum(name)
    A = EC.planted(lam)
    theta, V, info = eig.top_eigenpairs(torch.from_numpy(A), **kw)
    print(f"({name}): k {len(theta)}, block {info['block']}, applies {info['applies']}, steps {info['steps']}, "
          f"max residual {info['residual'].max() / float(theta[0]):.2e} theta_1")
    assert theta.dtype == torch.float64 and V.dtype == torch.float64
    assert len(theta) == k and info["block"] == block and info["applies"] <= 400
    EC.check_pairs(A, theta.numpy(), V.numpy(), info, groups)
    again = eig.top_eigenpairs(torch.from_numpy(A), **kw)
    assert torch.equal(again[0], theta) and torch.equal(again[1], V)


def test_driver_gives_up_as_documented():
    from dynamorph_amd import eig
    lam, kw, _ = EC.spectrum("e")
    with pytest.raises(eig.NotApplicable):
        eig.top_eigenpairs(torch.from_numpy(EC.planted(lam)), **kw)
    lam, kw, _ = EC.spectrum("d")
    A = torch.from_numpy(EC.planted(lam))
    with pytest.raises(eig.NotConverged):
        eig.top_eigenpairs(A, max_applies=4, **kw)
    with pytest.raises(eig.NotApplicable):
        eig.top_eigenpairs(A, k=250)                # k + guard > max_block < n
    for bad in (dict(), dict(k=3, fraction=0.5), dict(k=0), dict(k=601), dict(fraction=1.0), dict(fraction=0.0)):
        with pytest.raises(ValueError):
            eig.top_eigenpairs(A, **bad)
    with pytest.raises(ValueError):
        eig.top_eigenpairs(A.float(), k=3)
    nan = A.clone()
    nan[5, 5] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        eig.top_eigenpairs(nan, k=3)
    with pytest.raises(ValueError, match="finite"):
        eig.top_eigenpairs(nan, k=3, trace=1.0)


def test_driver_small_matrix_is_the_exact_decomposition():
    from dynamorph_amd import eig
    A = EC.planted(1.0 / np.arange(1, 41))
    calls = []

    def apply(Q):
        calls.append(Q.shape[1])
        return torch.from_numpy(A) @ Q
    theta, V, info = eig.top_eigenpairs(torch.from_numpy(A), fraction=0.9, apply=apply)
    assert info["block"] == 40 and calls[0] == 32 and calls[-1] == 40 and len(calls) == info["applies"]     # grown to n
    EC.check_pairs(A, theta.numpy(), V.numpy(), info, angles=False)


# ------------------------------------------------------------------------------------------ the PCA finalisations
def test_rank_deficient_request_is_refused_on_both_routes():
    """(f): centred data of rank 5, 8 components asked for."""
    from dynamorph_amd import pca as P
    rng = np.random.default_rng(3)
    X = rng.standard_normal((100, 5)) @ rng.standard_normal((5, 300))
    Xc = X - X.mean(0)
    for solver in ("partial", "full"):
        with pytest.raises(ValueError, match="at most 5 components are defined"):
            P.finalize_samples(torch.from_numpy(Xc @ Xc.T), 100, 300, 8, eigensolver=solver)
    fit = P.finalize_samples(torch.from_numpy(Xc @ Xc.T), 100, 300, 5, eigensolver="partial")
    assert fit["eigensolver_"] == "partial" and fit["n_components_"] == 5 and fit["W"].shape == (5, 100)


def test_routes_taken():
    from dynamorph_amd import pca as P
    rng = np.random.default_rng(4)
    X = rng.standard_normal((200, 90)) * np.linspace(3.0, 0.1, 90)
    mu = X.mean(0)
    C = torch.from_numpy((X - mu).T @ (X - mu))
    assert P.finalize(C, mu, 200, 0.5)["eigensolver_"] == "full"
    assert P.finalize(C, mu, 200, 0.5, eigensolver="partial")["eigensolver_"] == "partial"
    assert P.finalize(C, mu, 200, None, eigensolver="partial")["eigensolver_"] == "full"        # every component
    assert P.finalize(C[:64, :64], mu[:64], 200, 3, eigensolver="partial")["eigensolver_"] == "full"    # order <= 2 block
    flat = torch.eye(300, dtype=torch.float64) * (1.0 + 1e-3 * torch.arange(300) / 300)
    fit = P.finalize(flat, np.zeros(300), 400, 0.5, eigensolver="partial")                      # NotApplicable inside
    assert fit["eigensolver_"] == "full" and fit["eig_info_"] is None and fit["n_components_"] == 150
    with pytest.raises(ValueError, match="eigensolver"):
        P.finalize(C, mu, 200, 0.5, eigensolver="lanczos")
    with pytest.raises(ValueError, match="eigensolver"):
        P.PCA(0.5, eigensolver="lanczos")
    with pytest.raises(ValueError, match="between 0 and"):
        P.finalize(C, mu, 200, 91, eigensolver="partial")
    a, b = P.finalize(C, mu, 200, 7), P.finalize(C, mu, 200, 7, eigensolver="partial")
    for key in ("explained_variance_", "explained_variance_ratio_", "singular_values_", "noise_variance_"):
        np.testing.assert_allclose(b[key], a[key], rtol=1e-9)
    assert ((a["components_"] * b["components_"]).sum(1) >= 1 - 1e-9).all()          # the same directions AND signs
    assert P.PCA().eigensolver == "full" and P.WidePCA(eigensolver="partial").eigensolver == "partial"


def _cos(a, b):
    return (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)


def test_fixture_on_the_cpu():
    """g13's f1000 matrix in float64 through both finalisations with eigensolver="partial", against scikit-learn's float64
    attributes at the gates of tests/test_gpu_pca.py::_check_fit."""
    from dynamorph_amd import pca as P
    g = load_golden("g13_pca.npz")
    tag = "f1000"
    X = make_x({k[len(tag) + 8:]: g[k] for k in g if k.startswith(tag + "_recipe_")})
    assert checksum(X) == str(g[tag + "_sha256"])
    N, F = X.shape
    mu = X.mean(0)
    Xc = X - mu
    ref = {a: g[f"{tag}_f64_{a}"] for a in ("components_", "explained_variance_", "explained_variance_ratio_",
                                            "singular_values_", "noise_variance_", "n_components_")}
    full = P.finalize(torch.from_numpy(Xc.T @ Xc), mu, N, 0.5)
    assert full["eigensolver_"] == "full"
    fit = P.finalize(torch.from_numpy(Xc.T @ Xc), mu, N, 0.5, eigensolver="partial")
    s = X[0]                                        # any shift: the finalisation centres K itself
    wide = P.finalize_samples(torch.from_numpy((X - s) @ (X - s).T), N, F, 0.5, eigensolver="partial")
    comps = P.orient_components(wide.pop("W") @ torch.from_numpy(Xc)).numpy()
    for got, c in ((fit, fit["components_"]), (wide, comps)):
        assert got["eigensolver_"] == "partial" and got["eig_info_"]["applies"] <= 400
        print(got["eig_info_"]["block"], got["eig_info_"]["applies"], got["eig_info_"]["residual"].max())
        assert got["n_components_"] == int(ref["n_components_"])
        np.testing.assert_allclose(got["explained_variance_ratio_"], ref["explained_variance_ratio_"], rtol=1e-5)
        assert _cos(c, ref["components_"]).min() >= 1 - 1e-6
        for a in ("explained_variance_", "singular_values_", "noise_variance_"):
            np.testing.assert_allclose(got[a], ref[a], rtol=1e-5)
