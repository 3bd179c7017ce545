"""The exact k-nearest-neighbour graph of the latents on the GPU: what umap.UMAP(n_neighbors=n) computes first, and takes
ready-made as precomputed_knn=(knn_indices, knn_dists) (run_dim_reduction.py:143-207 fit_umap fits three of them, n = 15, 50,
200, on the pooled (N, 4096) latents; one sorted exact graph at k = 200 holds all three as its first columns).

dm_knn (csrc/knn.hip) works on one panel of query rows against all of X; this module keeps X resident, computes the shift
(the fp32 column mean: distances are translation invariant, the filter's error bound is not), walks the panels and returns
numpy (indices int64, distances float32).  The distance matrix is never formed.

Latents wider than MAX_FEATURES (VQ_VAE_z32: 65536 features) take wide_knn_graph / wide_knn_query:
the whole graph of at most WIDE_MAX_ROWS rows in one call, its filter panel made from the row Gram matrix that WidePCA needs
as well (dm_pca_rowgram), each candidate pair evaluated once; the same distances, the same certificate, the same bits."""
import numpy as np
import torch

from . import ops
from .pca import column_mean
from .rows import chunk_size, device_chunks, device_of, host_rows, shape_of

MAX_FEATURES = 16384           # DM_KNN_MAX_FEATURES
MAX_K = ops.KNN_MAX_K
DEFAULT_CHUNK_ROWS = 2048
WIDE_MAX_FEATURES = ops.KNN_WIDE_MAX_FEATURES      # DM_KNN_WIDE_MAX_FEATURES
WIDE_MAX_ROWS = ops.KNN_WIDE_MAX_ROWS              # DM_PCA_WIDE_MAX_SAMPLES
WIDE_STAGE_BYTES = 1 << 28                         # a chunk of wide queries is at most this large


def _resident(X, device):
    """X as a 2-D fp32 device matrix with unit column stride: a CUDA tensor is used in place, host data move there once."""
    x = host_rows(X, "knn").to(device_of(X, device), dtype=torch.float32)
    if x.shape[1] > 1 and x.stride(1) != 1:
        x = x.contiguous()
    return x


def _check_k(M, k, eligible):
    if k < 1 or k > MAX_K:
        raise ValueError(f"k = {k} is outside 1 .. {MAX_K}")
    if k > eligible:
        raise ValueError(f"k = {k} exceeds the {eligible} rows a query can have as neighbours (M = {M})")


def _check(M, F, k, eligible):
    if F < 1 or F > MAX_FEATURES:
        raise ValueError(f"knn on the GPU supports 1 .. {MAX_FEATURES} features, got {F}")
    _check_k(M, k, eligible)


def is_wide(X):
    """More columns than knn_graph / knn_query / PCA take: the wide route, decided from the shape alone, before any device
    call."""
    shape = shape_of(X)
    return len(shape) == 2 and shape[1] > MAX_FEATURES


def _check_wide(M, F, k, eligible):
    if F < 1 or F > WIDE_MAX_FEATURES:
        raise ValueError(f"wide knn on the GPU supports 1 .. {WIDE_MAX_FEATURES} features, got {F}")
    if M > WIDE_MAX_ROWS:
        raise ValueError(f"wide knn of {M} rows of {F} features: more than {MAX_FEATURES} features need all rows resident "
                         f"(and, for the graph, their {M} x {M} float64 Gram matrix) and support up to {WIDE_MAX_ROWS} rows")
    _check_k(M, k, eligible)


def column_shift(x):
    """fp32 column mean of a device matrix of any width (dm_pca_colsum per block of pca.MAX_FEATURES columns: float64 sums
    in a fixed order), as WidePCA.gram forms its shift."""
    return column_mean(x).float()


def _panel_state(x, R, k, cr, slack, shift, wide=False):
    """What every panel of a call shares: the shift, the slack, one workspace for panels of cr rows, the outputs."""
    s = column_shift(x) if isinstance(shift, str) else shift
    sl = ops.KNN_DEFAULT_SLACK if slack is None else int(slack)
    if wide:
        nbytes = ops.L.load().dm_knn_wide_workspace_bytes(cr, x.shape[0], x.shape[1], k, sl)
        if nbytes < 0:
            raise ValueError(f"dm_knn_wide: bad shape R = {cr}, M = {x.shape[0]}, F = {x.shape[1]}, k = {k}, slack = {sl}")
        ws = torch.empty(int(nbytes), device=x.device, dtype=torch.uint8)
    else:
        ws = ops.knn_workspace(cr, x.shape[0], x.shape[1], k, sl, x)
    idx = torch.empty((R, k), dtype=torch.int32, device=x.device)
    dist = torch.empty((R, k), dtype=torch.float32, device=x.device)
    return s, sl, ws, idx, dist, []


def _result(idx, dist, counts, return_fallback):
    """numpy (indices int64, distances float32[, rows redone exactly]): the dtypes umap-learn's precomputed_knn takes."""
    res = idx.cpu().numpy().astype(np.int64), dist.cpu().numpy()
    return res + (int(torch.cat(counts).sum().item()),) if return_fallback else res


def knn_graph(X, k, include_self=True, rows=None, chunk_rows=DEFAULT_CHUNK_ROWS, device=None, slack=None, shift="mean",
              return_fallback=False):
    """The k-NN graph of the rows of X (M, F): numpy (indices (R, k) int64, distances (R, k) float32), sorted by (distance,
    index).  include_self=True: column 0 is the row itself at 0.0 and k - 1 other rows follow (umap-learn's layout).
    rows=(r0, R): only those rows of the graph (a data-parallel caller passes its dist.shard_range).  X: a CUDA tensor (used
    in place) or host data, moved to the device once.  shift: "mean" (computed here), None, or an (F,) fp32 device tensor.
    return_fallback: also the number of rows that were redone exactly."""
    x = _resident(X, device)
    M, F = x.shape
    k = int(k)
    _check(M, F, k, M - 1 + (1 if include_self else 0))
    r0, R = (0, M) if rows is None else (int(rows[0]), int(rows[1]))
    if r0 < 0 or R < 1 or r0 + R > M:
        raise ValueError(f"rows=({r0}, {R}) lie outside X with {M} rows")
    cr = max(1, min(int(chunk_rows), R))
    with torch.no_grad(), torch.cuda.device(x.device):
        s, sl, ws, idx, dist, counts = _panel_state(x, R, k, cr, slack, shift)
        for lo in range(0, R, cr):
            m = min(cr, R - lo)
            _, _, c = ops.knn(x, k=k, rows=(r0 + lo, m), shift=s, slack=sl, include_self=include_self,
                              out=(idx[lo:lo + m], dist[lo:lo + m]), workspace=ws)
            counts.append(c)
        return _result(idx, dist, counts, return_fallback)


def knn_query(X, Q, k, chunk_rows=DEFAULT_CHUNK_ROWS, device=None, slack=None, shift="mean", return_fallback=False):
    """The k nearest rows of X for every row of Q (no row is excluded; k <= M).  Q on the device is used in place; host Q is
    streamed in chunks of chunk_rows rows through pinned staging, the next chunk's copy overlapping the current chunk's
    kernels.  Returns numpy (indices (R, k) int64, distances (R, k) float32)."""
    return _query(X, Q, k, chunk_rows, device, slack, shift, return_fallback, wide=False)


def _query(X, Q, k, chunk_rows, device, slack, shift, return_fallback, wide):
    """knn_query (dm_knn) and wide_knn_query (dm_knn_wide): one body."""
    x = _resident(X, device)
    M, F = x.shape
    k = int(k)
    (_check_wide if wide else _check)(M, F, k, M)
    call = ops.knn_wide if wide else ops.knn
    shape = shape_of(Q)
    if len(shape) != 2 or shape[1] != F:
        raise ValueError(f"Q has shape {shape}, expected (n, {F})")
    R = shape[0]
    if R < 1:
        raise ValueError("Q has no rows")
    cr = chunk_size(chunk_rows, R, F, WIDE_STAGE_BYTES if wide else None)
    with torch.no_grad(), torch.cuda.device(x.device):
        s, sl, ws, idx, dist, counts = _panel_state(x, R, k, cr, slack, shift, wide)
        for lo, q in device_chunks(Q, cr, x.device):
            m = q.shape[0]
            counts.append(call(x, q, k=k, shift=s, slack=sl, out=(idx[lo:lo + m], dist[lo:lo + m]), workspace=ws)[2])
        return _result(idx, dist, counts, return_fallback)


# ------------------------------------------------------------------------ more than MAX_FEATURES features (section 3.5f)
def _check_wide_memory(dev, N, F, k, slack, have_gram):
    """K (8 N^2) and the row Gram's workspace unless K is given, and the graph's workspace (the fp32 panel, 4 N^2, and the
    candidate lists) against the free memory of the device, before anything is allocated."""
    lib = ops.L.load()
    need_k = 0 if have_gram else 8 * N * N + max(int(lib.dm_pca_rowgram_workspace_bytes(N, F)), 0)
    need_ws = max(int(lib.dm_knn_wide_self_workspace_bytes(N, F, k, slack)), 0)
    free, _ = torch.cuda.mem_get_info(dev)
    if need_k + need_ws > free:
        raise ValueError(f"wide knn of {N} rows of {F} features needs {(need_k + need_ws) / 2**30:.1f} GiB on the device (row "
                         f"Gram matrix and its workspace {need_k / 2**30:.1f}, panel and lists {need_ws / 2**30:.1f} GiB), "
                         f"{free / 2**30:.1f} GiB are free")


def wide_knn_graph(X, k, include_self=True, device=None, slack=None, shift="mean", gram=None, return_fallback=False,
                   return_pairs=False, pair_once=True):
    """knn_graph for 1 .. WIDE_MAX_FEATURES features and at most WIDE_MAX_ROWS rows, in one call (dm_knn_wide_self): the same
    dtypes, ordering and bits as knn_graph.  The filter panel comes from the row Gram matrix K = (X - s)(X - s)^T
    (dm_pca_rowgram), the matrix WidePCA decomposes: gram=(mean, s, K) as WidePCA.gram(x) returned it is used as it is (and
    left unchanged), otherwise K is computed here for shift "mean" (the fp32 column mean, dm_pca_colsum per block of
    MAX_FEATURES columns), None or an (F,) fp32 device tensor.  return_fallback: also the rows redone exactly;
    return_pairs: also the exact pair evaluations made before the fallback (a pair on both rows' lists counts once).
    pair_once=False: knn_graph's refine kernel on the same candidate lists -- the same results, for comparison."""
    x = _resident(X, device)
    N, F = x.shape
    k = int(k)
    _check_wide(N, F, k, N - 1 + (1 if include_self else 0))
    sl = ops.KNN_DEFAULT_SLACK if slack is None else int(slack)
    if sl < 0 or sl > ops.KNN_MAX_SLACK:
        raise ValueError(f"slack = {sl} is outside 0 .. {ops.KNN_MAX_SLACK}")
    if gram is not None:
        _, s, K = gram
        if not torch.is_tensor(K) or tuple(K.shape) != (N, N) or K.dtype != torch.float64:
            raise ValueError(f"gram=(mean, s, K): K must be a float64 ({N}, {N}) device tensor")
        if s is not None and s.numel() != F:
            raise ValueError(f"gram=(mean, s, K): s has {s.numel()} entries, F = {F}")
    elif isinstance(shift, str) and shift != "mean":
        raise ValueError(f"shift={shift!r}: 'mean', None or an (F,) fp32 device tensor")
    with torch.no_grad(), torch.cuda.device(x.device):
        _check_wide_memory(x.device, N, F, k, sl, gram is not None)
        if gram is None:
            s = column_shift(x) if isinstance(shift, str) else shift
            K = ops.pca_rowgram(x, s)
        idx, dist, nfb, npairs = ops.knn_wide_self(x, K, k=k, shift=s, slack=sl, include_self=include_self,
                                                   pair_once=pair_once)
        res = _result(idx, dist, [nfb], return_fallback)
        return res + (int(npairs.item()),) if return_pairs else res


def wide_knn_query(X, Q, k, chunk_rows=DEFAULT_CHUNK_ROWS, device=None, slack=None, shift="mean", return_fallback=False):
    """knn_query for 1 .. WIDE_MAX_FEATURES features against at most WIDE_MAX_ROWS rows of X (dm_knn_wide: knn_query's
    kernels, the wide feature cap); Q has any number of rows, a chunk of them at most WIDE_STAGE_BYTES."""
    return _query(X, Q, k, chunk_rows, device, slack, shift, return_fallback, wide=True)
