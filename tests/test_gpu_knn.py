"""`gpu`: the exact k-nearest-neighbour graph (csrc/knn.hip, dynamorph_amd/knn.py) against the float64 truth computed from
the fp32 inputs, by the complete criterion of tests/helpers/knn_reference.py (tau = 1e-6 on d^2, every row) plus index
equality wherever the reference's own gaps exceed 1e-5.  The shapes are the smallest at which each part can go wrong: ragged
tiles and F no multiple of 4 (257, 40), the workload's width (130, 4096), many column tiles per row (5000, 32), the smallest
graph there is (2, 1), and data with an offset, on which the Gram filter alone gets every row wrong (test_knn_host.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import knn_reference as KR  # noqa: E402

pytestmark = pytest.mark.gpu

SELF_CASES = {
    "257x40": lambda: KR.fixture("plain_257x40"),
    "130x4096": lambda: KR.randn(111, (130, 4096)),
    "5000x32": lambda: KR.randn(112, (5000, 32)),
    "offset_257x64": lambda: KR.fixture("offset_257x64"),
    "offset_130x4096": lambda: KR.fixture("offset_130x4096"),
}
_cache = {}


def self_case(name):
    """(X, float64 d^2 with the self pairs at +inf), computed once per session."""
    if name not in _cache:
        X = SELF_CASES[name]()
        _cache[name] = (X, KR.d2_float64(X, X, self_r0=0))
    return _cache[name]


def graph(X, k, **kw):
    from dynamorph_amd import knn as K
    return K.knn_graph(torch.from_numpy(np.array(X)).cuda(), k, return_fallback=True, **kw)


@pytest.mark.parametrize("k", [1, 15, 200])
@pytest.mark.parametrize("name", sorted(SELF_CASES))
def test_self_graph(name, k):
    X, d2 = self_case(name)
    if k > X.shape[0] - 1:
        with pytest.raises(ValueError, match="exceeds"):
            graph(X, k, include_self=False)
        return
    idx, dist, nfb = graph(X, k, include_self=False)
    print(f"{name} k={k}: {nfb} of {X.shape[0]} rows took the fallback; "
          f"{KR.clear_share(d2, k):.3f} of the rows are bound by index equality")
    assert idx.dtype == np.int64 and dist.dtype == np.float32
    KR.assert_passes(idx, dist, d2, k, f"{name} k={k}", self_r0=0)
    idx_s, dist_s, _ = graph(X, k, include_self=True)                # UMAP layout: the row itself, then the first k - 1
    KR.assert_passes(idx_s, dist_s, d2, k, f"{name} k={k} include_self", self_r0=0, include_self=True)
    assert np.array_equal(idx_s[:, 1:], idx[:, :k - 1]) and np.array_equal(dist_s[:, 1:], dist[:, :k - 1])


def test_smallest_graph():
    X = np.array([[0.5], [-2.0]], np.float32)
    idx, dist, _ = graph(X, 1, include_self=False)
    assert idx.tolist() == [[1], [0]] and dist.tolist() == [[2.5], [2.5]]
    idx, dist, _ = graph(X, 2, include_self=True)
    assert idx.tolist() == [[0, 1], [1, 0]] and dist.tolist() == [[0.0, 2.5], [0.0, 2.5]]
    idx, dist, nfb = graph(X, 1, include_self=True)
    assert idx.tolist() == [[0], [1]] and dist.tolist() == [[0.0], [0.0]] and nfb == 0
    with pytest.raises(ValueError):
        graph(X, 2, include_self=False)


def test_duplicates():
    X = KR.randn(113, (200, 64)).copy()
    X[90] = X[7]
    X[150] = X[7]
    X[4] = X[3]
    d2 = KR.d2_float64(X, X, self_r0=0)
    idx, dist, _ = graph(X, 5, include_self=False)
    KR.assert_passes(idx, dist, d2, 5, "duplicates", self_r0=0)
    assert idx[7, :2].tolist() == [90, 150] and idx[90, :2].tolist() == [7, 150] and idx[150, :2].tolist() == [7, 90]
    assert idx[3, 0] == 4 and idx[4, 0] == 3
    for r, n in ((7, 2), (90, 2), (150, 2), (3, 1), (4, 1)):
        assert not dist[r, :n].any() and dist[r, n] > 0               # zero distances exactly, and only those
    idx_s, dist_s, _ = graph(X, 5, include_self=True)
    KR.assert_passes(idx_s, dist_s, d2, 5, "duplicates include_self", self_r0=0, include_self=True)
    assert idx_s[150, :3].tolist() == [150, 7, 90] and idx_s[90, :3].tolist() == [90, 7, 150]     # i itself first
    assert idx_s[4, :2].tolist() == [4, 3] and not dist_s[150, :3].any()
    # a whole block of equal rows, more of them than k + slack: ties at the filter's threshold, in index order
    Y = KR.randn(114, (400, 8)).copy()
    Y[100:300] = Y[100]
    d2y = KR.d2_float64(Y, Y, self_r0=0)
    idx, dist, _ = graph(Y, 15, include_self=False, slack=8)
    KR.assert_passes(idx, dist, d2y, 15, "block of duplicates", self_r0=0)
    assert idx[100].tolist() == list(range(101, 116)) and idx[299].tolist() == list(range(100, 115))


def test_foreign_queries():
    from dynamorph_amd import knn as K
    X, Q = KR.fixture("plain_257x40"), KR.randn(115, (70, 40))
    d2 = KR.d2_float64(Q, X)
    xd = torch.from_numpy(np.array(X)).cuda()
    for k in (1, 15, 256):
        idx, dist = K.knn_query(xd, torch.from_numpy(Q).cuda(), k)
        KR.assert_passes(idx, dist, d2, k, f"foreign k={k}")
    idx, dist = K.knn_query(xd[:100], torch.from_numpy(Q).cuda(), 100)     # no self exclusion: k up to M
    KR.assert_passes(idx, dist, np.ascontiguousarray(d2[:, :100]), 100, "foreign k=M")
    with pytest.raises(ValueError, match="exceeds"):
        K.knn_query(xd[:100], torch.from_numpy(Q).cuda(), 101)
    # a query that IS a row of X is not excluded
    idx, dist = K.knn_query(xd, xd[5:8], 1)
    assert idx[:, 0].tolist() == [5, 6, 7] and not dist.any()


@pytest.mark.parametrize("r0,R", [(0, 64), (100, 157), (256, 1)])
def test_row_range_equals_rows_of_the_whole_graph(r0, R):
    X, _ = self_case("257x40")
    whole = graph(X, 15)
    part = graph(X, 15, rows=(r0, R))
    assert part[0].shape == (R, 15)
    assert np.array_equal(part[0], whole[0][r0:r0 + R])
    assert np.array_equal(part[1].view(np.uint32), whole[1][r0:r0 + R].view(np.uint32))


@pytest.mark.parametrize("name", ["1000x64", "offset_257x64"])
def test_invariance_and_determinism(name):
    """The results depend on the inputs only: not on the query chunking, the slack, the shift, a fallback or the launch."""
    X = KR.randn(116, (1000, 64)) if name == "1000x64" else KR.fixture(name)
    d2 = KR.d2_float64(X, X, self_r0=0)
    base = graph(X, 15)
    KR.assert_passes(base[0], base[1], d2, 15, name, self_r0=0, include_self=True)
    runs = {
        "chunk_rows=64": graph(X, 15, chunk_rows=64),
        "slack=0": graph(X, 15, slack=0),
        "shift=None": graph(X, 15, shift=None),
        "slack=0, shift=None": graph(X, 15, slack=0, shift=None),
        "again": graph(X, 15),
    }
    for what, (idx, dist, nfb) in runs.items():
        print(f"{name} {what}: {nfb} fallback rows (default: {base[2]})")
        assert np.array_equal(idx, base[0]), what
        assert np.array_equal(dist.view(np.uint32), base[1].view(np.uint32)), what
    assert runs["slack=0"][2] > 0                                    # the fallback is known to have run
    assert runs["again"][2] == base[2]
    if name.startswith("offset"):
        assert runs["shift=None"][2] == X.shape[0]                   # uncentred: the bound certifies no row


def test_strided_input():
    from dynamorph_amd import ops
    W = torch.from_numpy(KR.randn(117, (257, 50))).cuda()
    view = W[:, 3:43]                                                # leading dimension 50 > F = 40, unaligned rows
    copy = view.contiguous()
    s = view.mean(0)
    a = ops.knn(view, k=15, shift=s)
    b = ops.knn(copy, k=15, shift=s)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert int(a[2]) == int(b[2])
    d2 = KR.d2_float64(copy.cpu().numpy(), copy.cpu().numpy(), self_r0=0)
    KR.assert_passes(a[0].cpu().numpy(), a[1].cpu().numpy(), d2, 15, "strided", self_r0=0)
    qa = ops.knn(copy, Q=W[10:80, 3:43], k=7)
    qb = ops.knn(copy, Q=W[10:80, 3:43].contiguous(), k=7)
    assert torch.equal(qa[0], qb[0]) and torch.equal(qa[1].view(torch.int32), qb[1].view(torch.int32))
    assert qa[0][:, 0].tolist() == list(range(10, 80))


def test_knn_query_from_pageable_host_memory():
    from dynamorph_amd import knn as K
    X, Q = KR.fixture("plain_257x40"), KR.randn(118, (70, 40))
    xd = torch.from_numpy(np.array(X)).cuda()
    dev = K.knn_query(xd, torch.from_numpy(Q).cuda(), 15)
    host = K.knn_query(xd, Q, 15, chunk_rows=24)                     # three chunks: 24, 24, 22
    f64 = K.knn_query(xd, Q.astype(np.float64), 15, chunk_rows=24)   # converted in the staging copy
    for got in (host, f64):
        assert np.array_equal(got[0], dev[0]) and np.array_equal(got[1].view(np.uint32), dev[1].view(np.uint32))


def test_ops_knn_refuses_bad_arguments():
    from dynamorph_amd import ops
    x = torch.zeros((10, 4), device="cuda")
    with pytest.raises(ValueError, match="eligible"):
        ops.knn(x, k=10)
    with pytest.raises(ValueError, match="k outside"):
        ops.knn(x, k=0)
    with pytest.raises(ValueError, match="self form"):
        ops.knn(x, Q=x, k=2, include_self=True)
    with pytest.raises(ValueError, match="rows="):
        ops.knn(x, k=2, rows=(5, 6))
    with pytest.raises(ValueError):
        ops.knn(x.cpu(), k=2)
