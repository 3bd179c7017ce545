"""`not gpu`: the host half of the k-nearest-neighbour graph of wide latents (more than 16384 features, DESIGN.md section
3.5f) -- the argument errors of dm_knn_wide and dm_knn_wide_self before any launch, their workspace sizes, the refusals of
knn.wide_knn_graph / wide_knn_query before any device call, and fit_knn's choice of route from the column count."""
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

WIDE_F = 1 << 20


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    return _lib.load()


def _aligned():
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 255) & ~255      # a 256-byte aligned host address standing in for device memory


def test_dm_knn_wide_argument_errors_before_any_launch(lib):
    """The foreign form: every refusal is made on the host (negative return, dm_last_error text)."""
    buf, p = _aligned()
    big = 1 << 50

    def call(X=p, M=100, F=65536, ldx=None, Q=p, R=70, ldq=None, k=15, slack=64, idx=p, dist=p, nfb=p, ws=p, ws_bytes=big):
        return lib.dm_knn_wide(X, M, F, F if ldx is None else ldx, Q, R, F if ldq is None else ldq, k, slack, None, idx, dist,
                               nfb, ws, ws_bytes, None)

    for kw, text in (
        (dict(X=None), b"NULL"), (dict(Q=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(dist=None), b"NULL"),
        (dict(nfb=None), b"NULL"), (dict(ws=None), b"NULL"),
        (dict(k=0), b"k outside"), (dict(k=257, M=1000), b"k outside"),
        (dict(k=101), b"eligible"),                                   # k <= M is allowed, k = M + 1 is not
        (dict(slack=-1), b"slack"), (dict(slack=257), b"slack"),
        (dict(F=0), b"F outside"), (dict(F=WIDE_F + 1), b"F outside"),
        (dict(ldx=65535), b"leading dimension"), (dict(ldq=65535), b"leading dimension"),
        (dict(M=24577), b"DM_PCA_WIDE_MAX_SAMPLES"), (dict(M=0), b">= 1"), (dict(R=0), b">= 1"),
        (dict(ws_bytes=lib.dm_knn_wide_workspace_bytes(70, 100, 65536, 15, 64) - 1), b"workspace"),
        (dict(ws=p + 4), b"aligned"),
    ):
        rc = call(**kw)
        assert rc == -1 and text in lib.dm_last_error() and b"dm_knn_wide" in lib.dm_last_error(), (kw, rc, lib.dm_last_error())
    for F in (16385, 65536, WIDE_F):                                  # accepted widths: a size, not a refusal
        assert lib.dm_knn_wide_workspace_bytes(70, 100, F, 15, 64) > 0
    assert lib.dm_knn_workspace_bytes(70, 100, 16385, 15, 64) == -1   # the narrow entry keeps its cap


def test_dm_knn_wide_self_argument_errors_before_any_launch(lib):
    buf, p = _aligned()
    big = 1 << 50

    def call(X=p, N=100, F=65536, ldx=None, K=p, k=15, slack=64, include_self=0, pair_once=1, idx=p, dist=p, nfb=p, npairs=None,
             ws=p, ws_bytes=big):
        return lib.dm_knn_wide_self(X, N, F, F if ldx is None else ldx, None, K, k, slack, include_self, pair_once, idx, dist,
                                    nfb, npairs, ws, ws_bytes, None)

    for kw, text in (
        (dict(X=None), b"X is NULL"), (dict(K=None), b"K is NULL"), (dict(idx=None), b"NULL"), (dict(dist=None), b"NULL"),
        (dict(nfb=None), b"NULL"), (dict(ws=None), b"NULL"),
        (dict(k=0), b"k outside"), (dict(k=257, N=1000), b"k outside"),
        (dict(k=100), b"eligible"),                                   # k > N - 1 without the self column
        (dict(k=101, include_self=1), b"eligible"),
        (dict(slack=-1), b"slack"), (dict(slack=257), b"slack"),
        (dict(F=0), b"F outside"), (dict(F=WIDE_F + 1), b"F outside"),
        (dict(ldx=65535), b"leading dimension"),
        (dict(N=24577), b"DM_PCA_WIDE_MAX_SAMPLES"), (dict(N=0), b">= 1"),
        (dict(K=p + 4), b"8-byte"),
        (dict(ws_bytes=lib.dm_knn_wide_self_workspace_bytes(100, 65536, 15, 64) - 1), b"workspace"),
        (dict(ws=p + 4), b"aligned"),
    ):
        rc = call(**kw)
        assert rc == -1 and text in lib.dm_last_error() and b"dm_knn_wide_self" in lib.dm_last_error(), \
            (kw, rc, lib.dm_last_error())
    for F in (16385, 65536, WIDE_F):
        assert lib.dm_knn_wide_self_workspace_bytes(100, F, 15, 64) > 0
    assert lib.dm_knn_wide_self_workspace_bytes(24576, 65536, 200, 64) > 0
    assert lib.dm_knn_wide_self_workspace_bytes(24577, 65536, 200, 64) == -1
    from dynamorph_amd import _lib
    with pytest.raises(ValueError, match="dm_knn_wide_self"):
        _lib.check(call(k=0), "dm_knn_wide_self")


def test_wide_workspace_bytes(lib):
    """Monotone in the shape, at least the fp32 panel, -1 for a bad shape."""
    w = [lib.dm_knn_wide_self_workspace_bytes(N, 65536, 200, 64) for N in (300, 1000, 2000, 8192, 20000, 24576)]
    assert all(b > 0 for b in w) and all(a < b for a, b in zip(w, w[1:]))
    assert w[-1] >= 24576 * 24576 * 4
    w = [lib.dm_knn_wide_self_workspace_bytes(8192, 65536, k, s) for k, s in ((1, 0), (15, 0), (15, 64), (200, 64), (256, 256))]
    assert all(a <= b for a, b in zip(w, w[1:])) and w[0] < w[-1] and w[0] >= 8192 * 8192 * 4
    w = [lib.dm_knn_wide_workspace_bytes(R, 20000, 65536, 200, 64) for R in (1, 2, 64, 128, 129, 1000, 2048)]
    assert all(b > 0 for b in w) and all(a <= b for a, b in zip(w, w[1:])) and w[0] < w[-1]
    assert w[-1] >= 2048 * 20000 * 4
    assert lib.dm_knn_wide_self_workspace_bytes(2, 1, 1, 0) > 0 and lib.dm_knn_wide_workspace_bytes(1, 1, 1, 1, 0) > 0
    for bad in ((0, 4, 1, 0), (10, 0, 1, 0), (10, WIDE_F + 1, 1, 0), (10, 4, 0, 0), (10, 4, 257, 0), (10, 4, 11, 0),
                (10, 4, 1, -1), (10, 4, 1, 257), (24577, 4, 1, 0)):
        assert lib.dm_knn_wide_self_workspace_bytes(*bad) == -1, bad
    for bad in ((0, 10, 4, 1, 0), (10, 0, 4, 1, 0), (10, 10, WIDE_F + 1, 1, 0), (10, 10, 4, 11, 0), (10, 24577, 4, 1, 0)):
        assert lib.dm_knn_wide_workspace_bytes(*bad) == -1, bad


def test_wide_entries_refuse_bad_arguments_before_any_device_call(monkeypatch):
    import torch
    from dynamorph_amd import knn as K
    monkeypatch.setattr(K, "_resident", lambda X, device: X)
    x = torch.zeros((10, 4))
    with pytest.raises(ValueError, match="exceeds"):
        K.wide_knn_graph(x, 11, include_self=False)
    with pytest.raises(ValueError, match="exceeds"):
        K.wide_knn_graph(x, 10, include_self=False)
    with pytest.raises(ValueError, match="outside 1"):
        K.wide_knn_graph(x, 0)
    with pytest.raises(ValueError, match="outside 1"):
        K.wide_knn_graph(torch.zeros((1000, 4)), 257)
    with pytest.raises(ValueError, match="slack"):
        K.wide_knn_graph(x, 3, slack=257)
    with pytest.raises(ValueError, match="shift="):
        K.wide_knn_graph(x, 3, shift="median")
    with pytest.raises(ValueError, match="gram="):
        K.wide_knn_graph(x, 3, gram=(None, None, torch.zeros((9, 9), dtype=torch.float64)))
    with pytest.raises(ValueError, match="features"):
        K.wide_knn_graph(torch.zeros((3, 0)), 1)
    with pytest.raises(ValueError, match=str(K.WIDE_MAX_ROWS)):      # the cap is named
        K.wide_knn_graph(torch.zeros((24577, 1)), 3)
    with pytest.raises(TypeError):
        K.wide_knn_graph(x, 3, rows=(0, 5))                           # rows= is not offered
    with pytest.raises(ValueError, match="exceeds"):
        K.wide_knn_query(x, torch.zeros((3, 4)), 11)
    with pytest.raises(ValueError, match="expected"):
        K.wide_knn_query(x, torch.zeros((3, 5)), 2)
    with pytest.raises(ValueError, match=str(K.WIDE_MAX_ROWS)):
        K.wide_knn_query(torch.zeros((24577, 1)), torch.zeros((3, 1)), 2)
    with pytest.raises(ValueError, match="features"):                 # the narrow entries keep their cap
        K.knn_graph(torch.zeros((10, 16385)), 3)
    assert K.WIDE_MAX_FEATURES == WIDE_F and K.WIDE_MAX_ROWS == 24576 and K.MAX_FEATURES == 16384


def test_fit_knn_chooses_the_route_from_the_column_count(tmp_path, monkeypatch):
    """Above 16384 columns fit_knn makes ONE wide_knn_graph call at the largest n and never calls knn_graph; the three files are
    slices of that graph.  At 12 columns it calls knn_graph as before."""
    from dynamorph_amd import dim_reduction as DR
    calls = []

    def stand_in(name):
        def f(X, k, include_self=True, **kw):
            calls.append((name, k, include_self, sorted(kw)))
            return KR.knn_graph_float64(X, k, include_self=include_self)
        return f

    monkeypatch.setattr(DR._knn, "wide_knn_graph", stand_in("wide"))
    monkeypatch.setattr(DR._knn, "knn_graph", stand_in("narrow"))
    X = KR.randn(8, (40, 16385))
    out = DR.fit_knn(X, str(tmp_path / "w"), n_nbrs=(5, 15, 30))
    assert calls == [("wide", 30, True, [])]
    assert sorted(os.listdir(tmp_path / "w")) == ["knn_nbr15.pkl", "knn_nbr30.pkl", "knn_nbr5.pkl"]
    got = {}
    for n in (5, 15, 30):
        raw = open(tmp_path / "w" / f"knn_nbr{n}.pkl", "rb").read()
        assert raw[:2] == b"\x80\x04"                                # pickle protocol 4
        got[n] = pickle.loads(raw)
        assert isinstance(got[n], list) and len(got[n]) == 2
        assert got[n][0].dtype == np.int64 and got[n][1].dtype == np.float32 and got[n][0].shape == (40, n)
        assert np.array_equal(got[n][0], out[n][0]) and np.array_equal(got[n][1], out[n][1])
    for n in (5, 15):
        assert np.array_equal(got[n][0], got[30][0][:, :n]) and np.array_equal(got[n][1], got[30][1][:, :n])
    assert np.array_equal(got[30][0][:, 0], np.arange(40)) and not got[30][1][:, 0].any()
    del calls[:]
    DR.fit_knn(X, str(tmp_path / "g"), n_nbrs=(5,), gram="G")          # keywords reach the wide entry
    assert calls == [("wide", 5, True, ["gram"])]
    del calls[:]
    DR.fit_knn(KR.randn(7, (60, 12)), str(tmp_path / "n"), n_nbrs=(5, 15))
    assert calls == [("narrow", 15, True, [])]
    del calls[:]
    DR.fit_knn(KR.randn(7, (20, 16384)), str(tmp_path / "e"), n_nbrs=(3,))      # the threshold itself is narrow
    assert calls == [("narrow", 3, True, [])]
