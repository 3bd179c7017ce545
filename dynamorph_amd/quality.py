"""How faithful an embedding is to the latents, on the GPU: trustworthiness, continuity and neighbour recall (DESIGN.md
section 3.5i).  fit_umap_embedding writes one embedding per (n_neighbors, a, b); the reference chooses among them from
UMAP.png by eye.  These are the standard numbers for that choice (Venna & Kaski; sklearn.manifold.trustworthiness), at sizes
where the N x N distance matrix and its argsort do not fit anywhere: what they need per row is the RANK, among the row's
neighbours in one space, of its k nearest neighbours in the other.

neighbor_ranks (dm_knn_ranks, csrc/knn.hip) computes exactly that: one pass over all pairs with knn_graph's Gram panel as a
filter, its proven error bound on both sides of every threshold, the exact-form distance as the arbiter of what the filter
cannot decide.  The rank of target j for row i is 1 + #{l != i : (d(i, l), l) < (d(i, j), j)}, d the fp32 distance knn_graph
reports: the rank of knn_graph(X, k, include_self=False)'s column c is c + 1, and the results depend on the inputs only."""
import numpy as np
import torch

from . import ops
from .knn import DEFAULT_CHUNK_ROWS, MAX_FEATURES, MAX_K, _resident, column_shift, is_wide, knn_graph
from .rows import shape_of


def _check_points(X, what):
    shape = shape_of(X)
    if len(shape) != 2:
        raise ValueError(f"{what} has shape {shape}, expected (samples, features)")
    if is_wide(X):
        raise ValueError(f"{what} has {shape[1]} features: more than {MAX_FEATURES} (knn.is_wide) take the wide route, which "
                         "the quality scores do not have")
    if shape[1] < 1 or shape[0] < 2:
        raise ValueError(f"{what} has shape {shape}: at least two rows of at least one feature")
    return shape


def _check_targets(targets, R, M):
    t = np.asarray(targets)
    if t.ndim != 2 or t.shape[0] != R or t.dtype.kind not in "iu":
        raise ValueError(f"targets has shape {t.shape} and dtype {t.dtype}, expected integers of shape ({R}, c)")
    c = t.shape[1]
    if c < 1 or c > MAX_K:
        raise ValueError(f"targets has {c} columns: 1 .. {MAX_K} per pass")
    if t.min() < 0 or t.max() >= M:
        raise ValueError(f"targets lie outside 0 .. {M - 1} (min {t.min()}, max {t.max()})")
    return np.ascontiguousarray(t, dtype=np.int32)


def neighbor_ranks(X, targets, rows=None, chunk_rows=DEFAULT_CHUNK_ROWS, device=None, shift="mean", cap=None,
                   return_counts=False):
    """Ranks of targets (R, c) -- row indices of X, 1 <= c <= 256, repeats allowed -- among the neighbours of the rows of X
    (M, F): int32 (R, c) numpy, 1 for the nearest other row, 0 for the row itself.  rows=(r0, R): targets belong to those rows
    (a data-parallel caller passes its dist.shard_range).  X: a CUDA tensor (used in place) or host data, moved to the device
    once.  shift: "mean", None or an (F,) fp32 device tensor; cap: entries of a row's list of columns the filter cannot
    decide (default ops.knn_ranks_default_cap).  Neither changes a result.  return_counts: also (columns decided one by one
    by the exact form, rows redone from exact distances to all M rows)."""
    M, F = _check_points(X, "X")
    r0, R = (0, M) if rows is None else (int(rows[0]), int(rows[1]))
    if r0 < 0 or R < 1 or r0 + R > M:
        raise ValueError(f"rows=({r0}, {R}) lie outside X with {M} rows")
    t = _check_targets(targets, R, M)
    c = t.shape[1]
    if cap is not None and int(cap) < 1:
        raise ValueError(f"cap = {cap}: at least one entry")
    x = _resident(X, device)
    cr = max(1, min(int(chunk_rows), R))
    with torch.no_grad(), torch.cuda.device(x.device):
        s = column_shift(x) if isinstance(shift, str) else shift
        cp = ops.knn_ranks_default_cap(c, M) if cap is None else int(cap)
        nbytes = ops.L.load().dm_knn_ranks_workspace_bytes(cr, M, F, c, cp)
        if nbytes < 0:
            raise ValueError(f"dm_knn_ranks: bad shape R = {cr}, M = {M}, F = {F}, c = {c}, cap = {cp}")
        ws = torch.empty(int(nbytes), device=x.device, dtype=torch.uint8)
        tg = torch.from_numpy(t).to(x.device)
        ranks = torch.empty((R, c), dtype=torch.int32, device=x.device)
        counts = []
        for lo in range(0, R, cr):
            m = min(cr, R - lo)
            _, na, nr = ops.knn_ranks(x, tg[lo:lo + m], rows=(r0 + lo, m), shift=s, cap=cp, out=ranks[lo:lo + m], workspace=ws)
            counts.append(torch.cat([na, nr]))
        res = ranks.cpu().numpy()
        if not return_counts:
            return res
        tot = torch.stack(counts).sum(0, dtype=torch.int64).cpu().numpy()
        return res, int(tot[0]), int(tot[1])


# ------------------------------------------------------------------------------------------------ the host formula
def _ks(n_neighbors, N):
    ks = (int(n_neighbors),) if np.isscalar(n_neighbors) else tuple(int(k) for k in n_neighbors)
    if not ks:
        raise ValueError("n_neighbors is empty")
    for k in ks:
        if k < 1:
            raise ValueError(f"n_neighbors = {k}: at least 1")
        if N is not None and k >= N / 2:
            raise ValueError(f"n_neighbors ({k}) should be less than n_samples / 2 ({N / 2})")
        if k > MAX_K:
            raise ValueError(f"n_neighbors = {k}: at most {MAX_K}")
    return ks, np.isscalar(n_neighbors)


def score_from_ranks(ranks, n_neighbors, n_samples=None):
    """T(k) = 1 - 2 / (N k (2 N - 3 k - 1)) sum_i sum_{c < k} max(0, r_ic - k) from ranks (R, >= max k): column c holds the
    rank, in the one space, of the row's (c + 1)-th neighbour in the other.  The sum is an integer; float64 out, one per k
    (a float for an int k).  n_samples: N where the ranks are a shard of the rows (the shards' penalties add up)."""
    r = np.asarray(ranks)
    N = r.shape[0] if n_samples is None else int(n_samples)
    ks, scalar = _ks(n_neighbors, N)
    if r.ndim != 2 or r.shape[1] < max(ks):
        raise ValueError(f"ranks has shape {r.shape}, need (rows, >= {max(ks)})")
    out = []
    for k in ks:
        penalty = int(np.maximum(r[:, :k].astype(np.int64) - k, 0).sum())
        out.append(1.0 - penalty * (2.0 / (N * k * (2.0 * N - 3.0 * k - 1.0))))
    return out[0] if scalar else tuple(out)


def recall_from_ranks(ranks, n_neighbors):
    """Share of the k nearest neighbours in the one space that are among the k nearest in the other: ranks 1 .. k."""
    r = np.asarray(ranks)
    ks, scalar = _ks(n_neighbors, None)
    out = [float(((r[:, :k] <= k) & (r[:, :k] >= 1)).mean()) for k in ks]
    return out[0] if scalar else tuple(out)


def _pair_shapes(X, Y, n_neighbors):
    sx, sy = _check_points(X, "X"), _check_points(Y, "Y")
    if sx[0] != sy[0]:
        raise ValueError(f"X has {sx[0]} rows and Y {sy[0]}: an embedding has one row per sample")
    return sx[0], _ks(n_neighbors, sx[0])[0]


def _graph_targets(graph, N, kmax, what):
    idx = np.asarray(graph[0] if isinstance(graph, (tuple, list)) else graph)
    if idx.ndim != 2 or idx.shape[0] != N or idx.shape[1] < kmax:
        raise ValueError(f"{what} has indices of shape {idx.shape}, need ({N}, >= {kmax}) without a self column")
    return idx[:, :kmax]


def trustworthiness(X, Y, n_neighbors=15, chunk_rows=DEFAULT_CHUNK_ROWS, device=None, shift="mean", cap=None, y_graph=None):
    """sklearn.manifold.trustworthiness(X, Y, n_neighbors) at any N: how far the k nearest neighbours of a row in the
    embedding Y (N, d) are from being its neighbours in X (N, F); 1.0 = no intruders.  n_neighbors: an int (a float64 comes
    back) or a tuple (a tuple does): ONE graph of Y at max(n_neighbors), ONE rank pass in X.  y_graph: an existing
    (knn_indices, knn_dists) of Y without the self column."""
    N, ks = _pair_shapes(X, Y, n_neighbors)
    kmax = max(ks)
    tg = _graph_targets(y_graph, N, kmax, "y_graph") if y_graph is not None else \
        knn_graph(Y, kmax, include_self=False, chunk_rows=chunk_rows, device=device)[0]
    ranks = neighbor_ranks(X, tg, chunk_rows=chunk_rows, device=device, shift=shift, cap=cap)
    return score_from_ranks(ranks, n_neighbors)


def continuity(X, Y, n_neighbors=15, chunk_rows=DEFAULT_CHUNK_ROWS, device=None, shift="mean", cap=None, x_graph=None):
    """The other direction (Venna & Kaski): how far the k nearest neighbours of a row in X are from being its neighbours in
    the embedding Y; 1.0 = nothing torn apart.  The roles of X and Y swap: the targets come from the graph of X, the ranks
    are taken in Y (the same kernels at F = d).  x_graph: an existing (knn_indices, knn_dists) of X without the self column
    -- fit_knn's output without its column 0."""
    N, ks = _pair_shapes(X, Y, n_neighbors)
    kmax = max(ks)
    tg = _graph_targets(x_graph, N, kmax, "x_graph") if x_graph is not None else \
        knn_graph(X, kmax, include_self=False, chunk_rows=chunk_rows, device=device, shift=shift)[0]
    ranks = neighbor_ranks(Y, tg, chunk_rows=chunk_rows, device=device, cap=cap)
    return score_from_ranks(ranks, n_neighbors)


def embedding_quality(X, embeddings, n_neighbors=15, chunk_rows=DEFAULT_CHUNK_ROWS, device=None, shift="mean", cap=None,
                      x_graph=None):
    """{name: {"trustworthiness", "continuity", "neighbor_recall"}} for embeddings = {name: (N, d) array} of the same X.
    The neighbour lists of all embeddings are concatenated, up to 256 columns per pass, so X's Gram panel is computed once
    for all of them (once per 256 // max k embeddings); the graph of X behind the continuity is built once.  neighbor_recall:
    the share of an embedding's k nearest neighbours that are among the k nearest in X.  n_neighbors: an int or a tuple."""
    if not embeddings:
        raise ValueError("embeddings is empty")
    names = list(embeddings)
    for name in names:
        N, ks = _pair_shapes(X, embeddings[name], n_neighbors)
    kmax = max(ks)
    x = _resident(X, device)
    xg = _graph_targets(x_graph, N, kmax, "x_graph") if x_graph is not None else \
        knn_graph(x, kmax, include_self=False, chunk_rows=chunk_rows, shift=shift)[0]
    out = {}
    per = max(1, MAX_K // kmax)
    for g0 in range(0, len(names), per):
        group = names[g0:g0 + per]
        ys = [_resident(embeddings[name], x.device) for name in group]
        tg = np.concatenate([knn_graph(y, kmax, include_self=False, chunk_rows=chunk_rows)[0] for y in ys], axis=1)
        ranks = neighbor_ranks(x, tg, chunk_rows=chunk_rows, shift=shift, cap=cap)
        for e, (name, y) in enumerate(zip(group, ys)):
            r = ranks[:, e * kmax:(e + 1) * kmax]
            out[name] = {"trustworthiness": score_from_ranks(r, n_neighbors),
                         "continuity": score_from_ranks(neighbor_ranks(y, xg, chunk_rows=chunk_rows, cap=cap), n_neighbors),
                         "neighbor_recall": recall_from_ranks(r, n_neighbors)}
    return out
