"""`not gpu`: the host half of the k-nearest-neighbour graph -- the acceptance criterion itself (tests/helpers/knn_reference.py)
on two CPU emulations, dm_knn's argument errors before any launch, and fit_knn / dim_reduction_knn with knn_graph replaced by
the float64 helper."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import knn_reference as KR  # noqa: E402


# ------------------------------------------------------------------------------------------------ the criterion
@pytest.mark.parametrize("name", sorted(KR.FIXTURES))
def test_difference_form_passes_every_row(name):
    X = KR.fixture(name)
    d2 = KR.d2_float64(X, X, self_r0=0)
    idx, dist = KR.emulate_difference(X, X, 15, self_r0=0)
    print(f"{name}: {KR.clear_share(d2, 15):.3f} of the rows have gaps above 1e-5 (index equality binds them)")
    KR.assert_passes(idx, dist, d2, 15, name, self_r0=0)


@pytest.mark.parametrize("name", ["offset_257x64", "offset_130x4096"])
def test_gram_form_alone_fails(name):
    """The fp32 Gram form has cancelled the bits that order near neighbours on data with an offset: a filter without a working
    re-check cannot pass the GPU test."""
    X = KR.fixture(name)
    d2 = KR.d2_float64(X, X, self_r0=0)
    idx, dist = KR.emulate_gram(X, X, 15, self_r0=0)
    bad = KR.failing_rows(idx, dist, d2, 15, self_r0=0)
    print(f"{name}: the Gram form fails {len(bad)} of {X.shape[0]} rows")
    assert len(bad) >= 0.9 * X.shape[0]


def test_criterion_catches_each_defect():
    X = KR.fixture("plain_257x40")
    d2 = KR.d2_float64(X, X, self_r0=0)
    idx, dist = KR.emulate_difference(X, X, 15, self_r0=0)
    assert not KR.failing_rows(idx, dist, d2, 15, self_r0=0)
    far = np.argmax(np.where(np.isinf(d2[3]), -1.0, d2[3]))
    i2, d_2 = idx.copy(), dist.copy()
    i2[3, 14] = far                                                  # a far row in the list, a near one missing
    assert 3 in KR.failing_rows(i2, d_2, d2, 15, self_r0=0)
    i2 = idx.copy()
    i2[5, [2, 3]] = i2[5, [3, 2]]                                    # order
    assert 5 in KR.failing_rows(i2, dist, d2, 15, self_r0=0)
    d_2 = dist.copy()
    d_2[7, 4] *= np.float32(1 + 1e-5)                                # a distance that is not the pair's
    assert 7 in KR.failing_rows(idx, d_2, d2, 15, self_r0=0)
    i2 = idx.copy()
    i2[9, 0] = 9                                                     # the self row
    assert 9 in KR.failing_rows(i2, dist, d2, 15, self_r0=0)
    i2 = idx.copy()
    i2[11, 1] = i2[11, 0]                                            # a duplicate
    assert 11 in KR.failing_rows(i2, dist, d2, 15, self_r0=0)
    gi, gd = KR.knn_graph_float64(X, 16, include_self=True)
    assert not KR.failing_rows(gi, gd, d2, 16, self_r0=0, include_self=True)
    gi[4, 0] = 5
    assert 4 in KR.failing_rows(gi, gd, d2, 16, self_r0=0, include_self=True)


# ------------------------------------------------------------------------------------- the C ABI, without a device
@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    return _lib.load()


def test_dm_knn_argument_errors_before_any_launch(lib):
    """Every refusal is made on the host (negative return, dm_last_error text); the pointers are never dereferenced."""
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    p = (p + 255) & ~255                    # a 256-byte aligned host address standing in for device memory
    big = 1 << 40

    def call(X=p, M=100, F=64, ldx=64, Q=None, R=100, ldq=0, r0=0, k=15, slack=64, include_self=0, idx=p, dist=p, nfb=p,
             ws=p, ws_bytes=big):
        return lib.dm_knn(X, M, F, ldx, Q, R, ldq, r0, k, slack, include_self, None, idx, dist, nfb, ws, ws_bytes, None)

    for kw, text in (
        (dict(X=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(dist=None), b"NULL"), (dict(nfb=None), b"NULL"),
        (dict(ws=None), b"NULL"),
        (dict(k=0), b"k outside"), (dict(k=257, M=1000, R=1000), b"k outside"),
        (dict(k=100), b"eligible"),                                   # self form: k > M - 1
        (dict(k=100, include_self=1, slack=0), None),                 # ... but M - 1 others and the row itself are fine
        (dict(F=0), b"F outside"), (dict(F=16385, ldx=16385), b"F outside"),
        (dict(ldx=63), b"leading dimension"),
        (dict(Q=p, ldq=63, k=100), b"leading dimension"),
        (dict(Q=p, ldq=64, k=101), b"eligible"),                      # foreign form: k <= M is allowed, k = M + 1 is not
        (dict(Q=p, ldq=64, include_self=1), b"self form"),
        (dict(r0=1), b"outside X"), (dict(r0=-1), b"outside X"),
        (dict(slack=-1), b"slack"), (dict(slack=257), b"slack"),
        (dict(ws_bytes=lib.dm_knn_workspace_bytes(100, 100, 64, 15, 64) - 1), b"workspace"),
        (dict(ws=p + 4), b"aligned"),
    ):
        if text is None:
            continue
        rc = call(**kw)
        assert rc == -1 and text in lib.dm_last_error(), (kw, rc, lib.dm_last_error())
    from dynamorph_amd import _lib
    with pytest.raises(ValueError, match="dm_knn"):
        _lib.check(call(k=0), "dm_knn")


def test_dm_knn_workspace_bytes(lib):
    w = [lib.dm_knn_workspace_bytes(R, 20000, 4096, 200, 64) for R in (1, 2, 64, 128, 129, 1000, 2048, 4096)]
    assert all(b > 0 for b in w) and all(a <= b for a, b in zip(w, w[1:])) and w[0] < w[-1]
    assert w[-1] >= 4096 * 20000 * 4                                 # the fp32 panel
    assert lib.dm_knn_workspace_bytes(1, 1, 1, 1, 0) > 0
    for bad in ((0, 10, 4, 1, 0), (10, 0, 4, 1, 0), (10, 10, 0, 1, 0), (10, 10, 16385, 1, 0), (10, 10, 4, 0, 0),
                (10, 10, 4, 257, 0), (10, 10, 4, 11, 0), (10, 10, 4, 1, -1), (10, 10, 4, 1, 257)):
        assert lib.dm_knn_workspace_bytes(*bad) == -1, bad


# ------------------------------------------------------------------------------------- fit_knn / dim_reduction_knn
def _write_latents(tmp_path, rng):
    dirs, prefixes = [], ["A", "B"]
    for d, n in (("cond0", (5, 7)), ("cond1", (9, 4))):
        os.makedirs(tmp_path / d)
        dirs.append(str(tmp_path / d))
        for p, rows in zip(prefixes, n):
            with open(tmp_path / d / f"{p}_latent_space_after.pkl", "wb") as f:
                pickle.dump(rng.standard_normal((rows, 12)).astype(np.float32), f, protocol=4)
    return dirs, prefixes


def test_fit_knn_files_are_slices_of_one_graph(tmp_path, monkeypatch):
    from dynamorph_amd import dim_reduction as DR
    calls = []

    def stand_in(X, k, include_self=True, **kw):
        calls.append((k, include_self))
        return KR.knn_graph_float64(X, k, include_self=include_self)

    monkeypatch.setattr(DR._knn, "knn_graph", stand_in)
    X = KR.randn(7, (260, 12))
    out = DR.fit_knn(X, str(tmp_path / "w"), n_nbrs=(15, 50, 200))
    assert calls == [(200, True)]                                    # ONE graph, at the largest n
    assert sorted(os.listdir(tmp_path / "w")) == ["knn_nbr15.pkl", "knn_nbr200.pkl", "knn_nbr50.pkl"]
    got = {}
    for n in (15, 50, 200):
        raw = open(tmp_path / "w" / f"knn_nbr{n}.pkl", "rb").read()
        assert raw[:2] == b"\x80\x04"                                # pickle protocol 4
        obj = pickle.loads(raw)
        assert isinstance(obj, list) and len(obj) == 2
        got[n] = obj
        assert obj[0].dtype == np.int64 and obj[1].dtype == np.float32
        assert obj[0].shape == (260, n) and obj[1].shape == (260, n)
        assert obj[0].flags.c_contiguous and obj[1].flags.c_contiguous
        assert np.array_equal(obj[0], out[n][0]) and np.array_equal(obj[1], out[n][1])
    for n in (15, 50):
        assert np.array_equal(got[n][0], got[200][0][:, :n]) and np.array_equal(got[n][1], got[200][1][:, :n])
    assert np.array_equal(got[200][0][:, 0], np.arange(260)) and not got[200][1][:, 0].any()
    KR.assert_passes(got[15][0], got[15][1], KR.d2_float64(X, X, self_r0=0), 15, "knn_nbr15", self_r0=0, include_self=True)
    with pytest.raises(ValueError):
        DR.fit_knn(X, str(tmp_path / "w"), n_nbrs=())


def test_dim_reduction_knn_pools_like_dim_reduction_pca(tmp_path, monkeypatch):
    from dynamorph_amd import dim_reduction as DR
    dirs, prefixes = _write_latents(tmp_path, np.random.default_rng(5))
    seen = {}

    def stand_in(X, k, include_self=True, **kw):
        seen["knn"] = np.array(X)
        return KR.knn_graph_float64(X, k, include_self=include_self)

    def fit_pca(train_data, weights_dir, labels=None, conditions=None, **kw):
        seen["pca"], seen["labels"] = np.array(train_data), list(labels)

    monkeypatch.setattr(DR._knn, "knn_graph", stand_in)
    monkeypatch.setattr(DR, "fit_PCA", fit_pca)
    DR.dim_reduction_pca(dirs, dirs, str(tmp_path / "w"), prefixes, fit_model=True)
    out = DR.dim_reduction_knn(dirs, str(tmp_path / "w"), prefixes, n_nbrs=(3, 8))
    assert seen["knn"].shape == (25, 12) and np.array_equal(seen["knn"], seen["pca"])
    assert seen["labels"] == [0] * 5 + [1] * 7 + [2] * 9 + [3] * 4
    expect = np.concatenate([pickle.load(open(os.path.join(d, f"{p}_latent_space_after.pkl"), "rb"))
                             for d in dirs for p in prefixes])
    assert np.array_equal(seen["knn"], expect)
    assert sorted(os.listdir(tmp_path / "w")) == ["knn_nbr3.pkl", "knn_nbr8.pkl"] and sorted(out) == [3, 8]
    one = DR.dim_reduction_knn(dirs[:1], str(tmp_path / "w1"), "A", n_nbrs=(3,))       # a single prefix as a string
    assert one[3][0].shape == (5, 3)
    with pytest.raises(ValueError, match="prefix"):
        DR.dim_reduction_knn(dirs, str(tmp_path / "w"), [])


def test_no_umap_import():
    import dynamorph_amd.dim_reduction  # noqa: F401
    import dynamorph_amd.knn  # noqa: F401
    assert "umap" not in sys.modules
    for mod in ("knn.py", "dim_reduction.py"):
        text = open(os.path.join(ROOT, "dynamorph_amd", mod)).read()
        assert "import umap" not in text


def test_knn_graph_refuses_bad_arguments_before_any_device_call(monkeypatch):
    import torch
    from dynamorph_amd import knn as K
    x = torch.zeros((10, 4))
    monkeypatch.setattr(K, "_resident", lambda X, device: X)
    with pytest.raises(ValueError, match="exceeds"):
        K.knn_graph(x, 11, include_self=False)
    with pytest.raises(ValueError, match="exceeds"):
        K.knn_graph(x, 10, include_self=False)
    with pytest.raises(ValueError, match="outside 1"):
        K.knn_graph(x, 0)
    with pytest.raises(ValueError, match="outside 1"):
        K.knn_graph(torch.zeros((1000, 4)), 257)
    with pytest.raises(ValueError, match="rows="):
        K.knn_graph(x, 3, rows=(8, 3))
    with pytest.raises(ValueError, match="features"):
        K.knn_graph(torch.zeros((10, 16385)), 3)
    with pytest.raises(ValueError, match="exceeds"):
        K.knn_query(x, torch.zeros((3, 4)), 11)
    with pytest.raises(ValueError, match="expected"):
        K.knn_query(x, torch.zeros((3, 5)), 2)
