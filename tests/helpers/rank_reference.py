"""Float64 truth for the neighbour ranks behind trustworthiness and continuity (dynamorph_amd/quality.py).

The rank of target j for row i is 1 + #{l != i : (d(i, l), l) < (d(i, j), j)}.  The float64 truth is computed from the fp32
inputs (knn_reference.d2_float64: d^2 from differences, the self pair +inf); the exact form's own error is about 3e-7 on d^2,
so the criterion is an INTERVAL at tau = knn_reference.TAU = 1e-6:
    lo = 1 + #{d2_l < d2_j (1 - tau)},   hi = #{d2_l <= d2_j (1 + tau)}   (the count of hi includes j itself),
every rank lies in [lo, hi], and equals it where lo == hi -- which is nearly everywhere on the random fixtures
(test_quality_host.py asserts the share).  On the lattice the exact form is exact and the ranks are the stable (d^2, index)
ranks, ties included."""
import functools

import numpy as np

import umap_reference as UR
from knn_reference import TAU, d2_float64  # noqa: F401  (TAU: the tests' tolerance)


def _read_only(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _top2(X):
    """The projection onto the top two right singular vectors of the centred X, fp32."""
    Xc = np.asarray(X, np.float64)
    Xc = Xc - Xc.mean(0)
    _, _, vt = np.linalg.svd(Xc, full_matrices=False)
    return (Xc @ vt[:2].T).astype(np.float32)


def _blobs():
    X = np.ascontiguousarray(UR.blobs()[0][:700])
    return X, _top2(X)


def _randn(shape):
    X = np.random.default_rng(3).standard_normal(shape).astype(np.float32)
    return X, _top2(X)


def _lattice():
    rng = np.random.default_rng(4)
    X = rng.integers(-3, 4, (400, 6)).astype(np.float32)
    Y = (X[:, :2] + np.float32(0.01) * rng.standard_normal((400, 2)).astype(np.float32)).astype(np.float32)
    return X, Y


FIXTURES = {
    "blobs_700x64": _blobs,
    "randn_384x4096": lambda: _randn((384, 4096)),
    "randn_300x8": lambda: _randn((300, 8)),
    "lattice_400x6": _lattice,
}
RANDOM = ("blobs_700x64", "randn_384x4096", "randn_300x8")


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(X (N, F) fp32, Y (N, 2) fp32), read-only, made once."""
    return _read_only(*FIXTURES[name]())


@functools.lru_cache(maxsize=None)
def d2_of(name, which="X"):
    """Float64 d^2 of the fixture's X or Y with the self pairs at +inf, read-only, made once."""
    P = fixture(name)[0 if which == "X" else 1]
    return _read_only(d2_float64(P, P, self_r0=0))[0]


def graph_float64(d2, k):
    """The k nearest other rows by stable (d^2, index): (N, k) int64."""
    return np.argsort(d2, axis=1, kind="stable")[:, :k]


def rank_interval(d2, targets, tau=TAU, r0=0):
    """(lo, hi) int64 (R, c) for targets (R, c) of the rows r0 .. r0 + R - 1 whose float64 d^2 to all M rows is d2 (R, M), the
    self pair +inf.  A target equal to its row has lo = hi = 0."""
    targets = np.asarray(targets, np.int64)
    R = d2.shape[0]
    lo, hi = np.empty(targets.shape, np.int64), np.empty(targets.shape, np.int64)
    for i in range(R):
        srt = np.sort(d2[i])
        dj = d2[i, targets[i]]
        fin = np.isfinite(dj)
        lo[i] = np.where(fin, 1 + np.searchsorted(srt, dj * (1 - tau), side="left"), 0)
        hi[i] = np.where(fin, np.searchsorted(srt, dj * (1 + tau), side="right"), 0)
        assert (targets[i][~fin] == r0 + i).all()
    return lo, hi


def rank_stable(d2, targets, r0=0):
    """The ranks by stable (d^2, index) order, exactly: int64 (R, c); 0 for a target equal to its row."""
    targets = np.asarray(targets, np.int64)
    R, M = d2.shape
    order = np.argsort(d2, axis=1, kind="stable")
    rank = np.empty((R, M), np.int64)
    rank[np.arange(R)[:, None], order] = np.arange(1, M + 1)[None, :]
    out = np.take_along_axis(rank, targets, axis=1)
    out[targets == (r0 + np.arange(R))[:, None]] = 0
    return out


def normalisation(N, k):
    return 2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0))


def trustworthiness_from_ranks(ranks, k, N=None):
    """1 - 2 / (N k (2 N - 3 k - 1)) sum max(0, r - k) over the first k columns of ranks (N, >= k), in float64."""
    r = np.asarray(ranks, np.int64)[:, :k]
    N = r.shape[0] if N is None else N
    return 1.0 - float(np.maximum(r - k, 0).sum()) * normalisation(N, k)
