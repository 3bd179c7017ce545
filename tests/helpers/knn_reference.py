"""Float64 truth, the acceptance criterion and two CPU emulations for the k-nearest-neighbour graph (dynamorph_amd/knn.py).

The truth is computed from the fp32 inputs: d^2 = sum (q - x)^2 in float64, stable sort by (d^2, index).  The criterion is
complete (no row is exempt), tau = 1e-6 on d^2: the exact form's own error is about 5 u = 3e-7 (one rounding of the
difference, the square, the fp32 sum of four squares before the float64 sum).  Per row, d64_k the reference's k-th distance:
  1. every returned index j has d64^2(i, j) <= d64_k^2 (1 + tau);
  2. every row with d64^2 < d64_k^2 (1 - tau) is returned;
  3. each reported distance is within tau / 2 relative (plus one fp32 ulp) of d64(i, j), and exactly 0 where d64 is 0;
  4. the reported distances are non-decreasing, equal distances in ascending index order;
  5. indices unique and in range; the self row absent, or in column 0 at 0.0 for include_self.
Index equality on top: wherever every relative gap among the reference's first k + 1 squared distances exceeds 1e-5 the
indices equal the reference's exactly."""
import functools

import numpy as np

TAU = 1e-6
GAP = 1e-5

# name -> (seed, offset, scale, shape): offset + scale * standard_normal(shape), fp32
FIXTURES = {
    "plain_257x40": (101, 0.0, 1.0, (257, 40)),
    "offset_257x64": (102, 10.0, 1e-2, (257, 64)),
    "offset_130x4096": (103, 3.0, 1e-2, (130, 4096)),
}


def randn(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    seed, offset, scale, shape = FIXTURES[name]
    x = (np.float32(offset) + np.float32(scale) * randn(seed, shape)).astype(np.float32)
    x.setflags(write=False)
    return x


def d2_float64(Q, X, self_r0=None):
    """(R, M) float64 squared distances from differences; the self pairs (i, self_r0 + i) are +inf."""
    Q64, X64 = np.asarray(Q, np.float64), np.asarray(X, np.float64)
    R, M, F = Q64.shape[0], X64.shape[0], X64.shape[1]
    out = np.empty((R, M), np.float64)
    step = max(1, (1 << 24) // max(1, M * F))
    for lo in range(0, R, step):
        diff = Q64[lo:lo + step, None, :] - X64[None, :, :]
        out[lo:lo + step] = np.einsum("rmf,rmf->rm", diff, diff)
    if self_r0 is not None:
        out[np.arange(R), self_r0 + np.arange(R)] = np.inf
    return out


_sorted = {}        # id(d2) -> (d2, order, sorted d^2), the first 258 columns: the sort is done once per matrix


def truth(d2, k):
    """Stable sort by (d^2, index): (indices (R, k) int64, d^2 sorted (R, min(k + 1, M)))."""
    hit = _sorted.get(id(d2))
    if hit is None or hit[0] is not d2:
        order = np.argsort(d2, axis=1, kind="stable")[:, :258]
        hit = _sorted[id(d2)] = (d2, order, np.take_along_axis(d2, order, axis=1))
    assert k <= 257
    return hit[1][:, :k], hit[2][:, :k + 1]


def knn_graph_float64(X, k, include_self=True, rows=None, **_):
    """The float64 stand-in of knn.knn_graph: numpy (indices int64, distances float32)."""
    X = np.asarray(X, np.float32)
    r0, R = (0, X.shape[0]) if rows is None else rows
    d2 = d2_float64(X[r0:r0 + R], X, self_r0=r0)
    kk = k - 1 if include_self else k
    idx, srt = truth(d2, kk)
    dist = np.sqrt(srt[:, :kk]).astype(np.float32)
    if include_self:
        idx = np.concatenate([(r0 + np.arange(R))[:, None], idx], axis=1)
        dist = np.concatenate([np.zeros((R, 1), np.float32), dist], axis=1)
    return idx.astype(np.int64), dist


def emulate_difference(Q, X, k, self_r0=None):
    """The exact form on the CPU: differences and squares in fp32, sums in float64; sorted by (distance, index)."""
    Q, X = np.asarray(Q, np.float32), np.asarray(X, np.float32)
    R, M, F = Q.shape[0], X.shape[0], X.shape[1]
    d2 = np.empty((R, M), np.float64)
    step = max(1, (1 << 24) // max(1, M * F))
    for lo in range(0, R, step):
        diff = Q[lo:lo + step, None, :] - X[None, :, :]
        d2[lo:lo + step] = (diff * diff).astype(np.float64).sum(axis=2)
    if self_r0 is not None:
        d2[np.arange(R), self_r0 + np.arange(R)] = np.inf
    dist = np.sqrt(d2).astype(np.float32)
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    return order, np.take_along_axis(dist, order, axis=1)


def emulate_gram(Q, X, k, self_r0=None):
    """The fp32 Gram form |q|^2 + |x|^2 - 2 q.x WITHOUT a re-check: what a filter alone would report."""
    Q, X = np.asarray(Q, np.float32), np.asarray(X, np.float32)
    R = Q.shape[0]
    g = (Q * Q).sum(1, dtype=np.float32)[:, None] + (X * X).sum(1, dtype=np.float32)[None, :] - np.float32(2) * (Q @ X.T)
    g = np.maximum(g, np.float32(0)).astype(np.float32)
    if self_r0 is not None:
        g[np.arange(R), self_r0 + np.arange(R)] = np.inf
    order = np.argsort(g, axis=1, kind="stable")[:, :k]
    return order, np.sqrt(np.take_along_axis(g, order, axis=1)).astype(np.float32)


def failing_rows(idx, dist, d2, k, self_r0=None, include_self=False):
    """Rows that miss the criterion or the index equality: {row: reason} (empty = pass).  d2: d2_float64 of the same queries
    (self pairs +inf); idx (R, k), dist (R, k) as returned."""
    idx, dist = np.asarray(idx).astype(np.int64), np.asarray(dist)
    R, M = d2.shape
    bad = {}

    def fail(rows, why):
        for r in np.flatnonzero(rows):
            bad.setdefault(int(r), why)

    assert idx.shape == (R, k) and dist.shape == (R, k) and dist.dtype == np.float32, (idx.shape, dist.shape, dist.dtype)
    if include_self:
        me = self_r0 + np.arange(R)
        fail(idx[:, 0] != me, "5: column 0 is not the row itself")
        fail(dist[:, 0] != 0.0, "5: the self distance is not 0.0")
        idx, dist, k = idx[:, 1:], dist[:, 1:], k - 1
        if k == 0:
            return bad
    ref_idx, srt = truth(d2, k)
    d2k = srt[:, k - 1]
    fail(((idx < 0) | (idx >= M)).any(1), "5: index out of range")
    idx_c = np.clip(idx, 0, M - 1)
    got = np.take_along_axis(d2, idx_c, axis=1)                     # float64 d^2 of the returned pairs
    fail(np.isinf(got).any(1), "5: the self row is in the list")
    fail(np.array([len(set(r)) != k for r in idx_c.tolist()]), "5: indices are not unique")
    fail((got > d2k[:, None] * (1 + TAU)).any(1), "1: a returned row lies beyond the k-th distance")
    member = np.zeros((R, M), bool)
    np.put_along_axis(member, idx_c, True, axis=1)
    fail(((d2 < d2k[:, None] * (1 - TAU)) & ~member).any(1), "2: a row inside the k-th distance is missing")
    d64 = np.sqrt(got)
    tol = TAU / 2 * d64 + np.spacing(d64.astype(np.float32)).astype(np.float64)
    fail((np.abs(dist.astype(np.float64) - d64) > tol).any(1), "3: a reported distance is off")
    fail(((got == 0) & (dist != 0)).any(1), "3: a zero distance is not reported as 0")
    if k > 1:
        fail((dist[:, 1:] < dist[:, :-1]).any(1), "4: distances decrease")
        fail(((dist[:, 1:] == dist[:, :-1]) & (idx[:, 1:] <= idx[:, :-1])).any(1), "4: a tie is not in index order")
    if srt.shape[1] > 1:
        lo, hi = srt[:, :-1], srt[:, 1:]
        with np.errstate(invalid="ignore"):
            clear = ((hi - lo) > GAP * hi) | np.isinf(hi)
        clear = clear.all(1)
    else:
        clear = np.ones(R, bool)
    fail(clear & (idx != ref_idx).any(1), "indices differ from the reference although its gaps exceed 1e-5")
    return bad


def clear_share(d2, k):
    """Share of rows whose first k + 1 reference distances have relative gaps above 1e-5 (the rows index equality binds)."""
    _, srt = truth(d2, k)
    lo, hi = srt[:, :-1], srt[:, 1:]
    return float((((hi - lo) > GAP * hi) | np.isinf(hi)).all(1).mean())


def assert_passes(idx, dist, d2, k, what, **kw):
    bad = failing_rows(idx, dist, d2, k, **kw)
    assert not bad, f"{what}: {len(bad)} of {d2.shape[0]} rows fail, e.g. {sorted(bad.items())[:5]}"
