"""The UMAP embedding behind the exact k-NN graph (run_dim_reduction.py:143-207 fit_umap: umap.UMAP(a=1.58, b=0.9,
n_neighbors=n) for n = 15, 50, 200): smooth distances, the fuzzy simplicial set, the sampling schedule, the initialisation and
a deterministic layout, as DESIGN.md section 3.5c defines them (McInnes, Healy, Melville 2018).

dm_umap_smooth, dm_umap_membership and dm_umap_epoch (csrc/umap.hip) are the device kernels; the symmetrisation, the pruning
and the schedule arrays are sorting and merging of integer keys in torch and run on CPU tensors as well.  The layout keeps
two position buffers and gives every vertex its row, its position and its entries' schedule state, so a fit is a function of
its inputs and the seed alone.  Two output dimensions, the Euclidean k-NN graph, a and b given (no fit from min_dist).

A fitted model that kept its training matrix places new rows into the embedding (transform): the
query graph (knn.knn_query), dm_umap_transform_prepare and ONE launch of dm_umap_transform_layout for all epochs -- the
training positions are fixed, so a new row reads nothing that another new row writes.

Latents of more than knn.MAX_FEATURES columns (VQ_VAE_z32: 65536) take the wide route, chosen from
the column count alone: knn.wide_knn_graph / knn.wide_knn_query and WidePCA(n_components=2), the fit computing ONE row Gram
matrix for both the graph and the PCA initialisation.  Such a model keeps (and pickles) its N x F x 4-byte training matrix."""
import numpy as np
import torch

from . import knn as _knn
from . import ops
from .rows import device_of, shape_of

MAX_K = ops.UMAP_MAX_K
_M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------------------------------- the generator
def mix64(z):
    """The finaliser of splitmix64 on numpy uint64 (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def counter_word(seed, epoch, entry, p):
    """The 64-bit word of the counter (seed, epoch, entry, p): mix64(mix64(mix64(seed + G (epoch + 1)) ^ entry) + G (p + 1)),
    G = 0x9E3779B97F4A7C15.  R = its upper 32 bits; the jitter uses epoch = -1, entry = the row, p = the dimension."""
    with np.errstate(over="ignore"):
        key = mix64(np.uint64((int(seed) + GOLDEN * (int(epoch) + 1)) & _M64))
        ke = mix64(key ^ np.asarray(entry, dtype=np.uint64))
        return mix64(ke + np.uint64(GOLDEN) * (np.asarray(p, dtype=np.uint64) + np.uint64(1)))


def jitter(seed, N):
    """u (N, 2) float32 in [-1, 1): the upper 24 bits of counter_word(seed, -1, i, d) / 2^23 - 1 (exact in float32)."""
    w = counter_word(seed, -1, np.arange(N, dtype=np.uint64)[:, None], np.arange(2, dtype=np.uint64)[None, :])
    return ((w >> np.uint64(40)).astype(np.float32) / np.float32(2 ** 23) - np.float32(1)).astype(np.float32)


# --------------------------------------------------------------------------------------------------- argument checking
def default_n_epochs(N):
    return 500 if N <= 10000 else 200


def check_graph(knn_indices, knn_dists):
    """The host copies (indices (N, k) int64, distances (N, k) float32) of a graph the kernels accept, or ValueError: 2 <= k
    <= 256, k <= N, every index in [0, N), column 0 the row itself.  No device call is made on host input."""
    idx = knn_indices.cpu().numpy() if torch.is_tensor(knn_indices) else np.asarray(knn_indices)
    dist = knn_dists.cpu().numpy() if torch.is_tensor(knn_dists) else np.asarray(knn_dists)
    if idx.ndim != 2 or idx.shape != dist.shape:
        raise ValueError(f"knn_indices {idx.shape} and knn_dists {dist.shape} must be two (N, k) arrays of one shape")
    if not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"knn_indices must be integers, got {idx.dtype}")
    N, k = idx.shape
    if k < 2 or k > MAX_K:
        raise ValueError(f"k = {k} is outside 2 .. {MAX_K}")
    if k > N:
        raise ValueError(f"k = {k} exceeds the {N} rows of the graph")
    if N > 0x7fffffff:
        raise ValueError(f"N = {N} does not fit 31 bits")
    if idx.min() < 0 or idx.max() >= N:
        raise ValueError(f"knn_indices lie outside 0 .. {N - 1}")
    if not np.array_equal(idx[:, 0], np.arange(N)):
        raise ValueError("column 0 of knn_indices must be the row itself (knn_graph(include_self=True))")
    return np.ascontiguousarray(idx, dtype=np.int64), np.ascontiguousarray(dist, dtype=np.float32)


def check_query_graph(knn_indices, knn_dists, M):
    """The host copies (indices (R, k) int64, distances (R, k) float32) of a query graph against M training rows that the
    transform kernels accept, or ValueError: R >= 1, 2 <= k <= 256, k <= M, every index in [0, M).  There is no self column.
    No device call is made on host input."""
    idx = knn_indices.cpu().numpy() if torch.is_tensor(knn_indices) else np.asarray(knn_indices)
    dist = knn_dists.cpu().numpy() if torch.is_tensor(knn_dists) else np.asarray(knn_dists)
    if idx.ndim != 2 or idx.shape != dist.shape:
        raise ValueError(f"knn_indices {idx.shape} and knn_dists {dist.shape} must be two (R, k) arrays of one shape")
    if not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"knn_indices must be integers, got {idx.dtype}")
    R, k = idx.shape
    if R < 1:
        raise ValueError("the query graph has no rows")
    if k < 2 or k > MAX_K:
        raise ValueError(f"k = {k} is outside 2 .. {MAX_K}")
    if k > M:
        raise ValueError(f"k = {k} exceeds the {M} training rows")
    if M > 0x7fffffff or R > 0x7fffffff:
        raise ValueError(f"M = {M} or R = {R} does not fit 31 bits")
    if idx.min() < 0 or idx.max() >= M:
        raise ValueError(f"knn_indices lie outside 0 .. {M - 1}")
    return np.ascontiguousarray(idx, dtype=np.int64), np.ascontiguousarray(dist, dtype=np.float32)


def _check_init(init, N):
    if isinstance(init, str):
        if init != "pca":
            raise ValueError(f"init={init!r}: 'pca' or an (N, 2) array (spectral initialisation is not built)")
        return None
    y = init.detach().cpu().numpy() if torch.is_tensor(init) else np.asarray(init)
    if y.ndim != 2 or y.shape[1] != 2:
        raise ValueError(f"the layout has two output dimensions; init has shape {y.shape}")
    if y.shape[0] != N:
        raise ValueError(f"init has {y.shape[0]} rows, the graph has {N}")
    return np.ascontiguousarray(y, dtype=np.float32)


# ------------------------------------------------------------------------------------------- plumbing (any torch device)
def symmetrize(knn_indices, membership):
    """W = A + A^T - A o A^T of the directed memberships A (N, k) at columns knn_indices (N, k), zeros dropped, on the union
    pattern, evaluated as (a + b) - a * b in float32 (so w_ij and w_ji are the same bits).  CSR: (indptr (N + 1) int64,
    indices int32 ascending within a row, data float32), on the tensors' device.  A row must not name a column twice."""
    N, k = membership.shape
    dev = membership.device
    rows = torch.arange(N, device=dev, dtype=torch.int64).repeat_interleave(k)
    cols = knn_indices.reshape(-1).to(torch.int64)
    a = membership.reshape(-1).to(torch.float32)
    keep = a != 0
    rows, cols, a = rows[keep], cols[keep], a[keep]
    kf, of = torch.sort(rows * N + cols)
    if kf.numel() > 1 and bool((kf[1:] == kf[:-1]).any()):
        raise ValueError("a row of knn_indices names a column twice")
    kt, ot = torch.sort(cols * N + rows)
    union = torch.unique(torch.cat([kf, kt]), sorted=True)
    A = torch.zeros(union.numel(), dtype=torch.float32, device=dev)
    B = torch.zeros_like(A)
    A[torch.searchsorted(union, kf)] = a[of]
    B[torch.searchsorted(union, kt)] = a[ot]
    w = (A + B) - A * B
    nz = w != 0
    union, w = union[nz], w[nz]
    return _csr(union // N, N), (union % N).to(torch.int32), w


def _csr(rows, N):
    indptr = torch.zeros(N + 1, dtype=torch.int64, device=rows.device)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    return indptr


def prune(indptr, indices, data, n_epochs):
    """The entries the layout samples: w >= w_max / n_epochs (float32), as CSR again."""
    if data.numel() == 0:
        return indptr, indices, data
    keep = data >= data.max() / torch.tensor(float(n_epochs), dtype=torch.float32, device=data.device)
    N = indptr.numel() - 1
    rows = torch.repeat_interleave(torch.arange(N, device=data.device, dtype=torch.int64), indptr[1:] - indptr[:-1])
    return _csr(rows[keep], N), indices[keep], data[keep]


def schedule(data, negative_sample_rate=5):
    """(eps = w_max / w, eps_neg = eps / negative_sample_rate), float32, per stored entry."""
    if data.numel() == 0:
        return data.clone(), data.clone()
    eps = data.max() / data
    return eps, eps / torch.tensor(float(negative_sample_rate), dtype=torch.float32, device=data.device)


def init_layout(y, seed):
    """Each dimension of y (N, 2) rescaled to [0, 10] as 10 (y - min) / (max - min) (0 where max = min) plus the jitter
    1e-4 u(seed, i, d), float32 throughout, on y's device."""
    y = y.to(torch.float32)
    lo, hi = y.min(0).values, y.max(0).values
    span = hi - lo
    t = torch.where(span > 0, (y - lo) / torch.where(span > 0, span, torch.ones_like(span)), torch.zeros_like(y))
    u = torch.from_numpy(jitter(seed, y.shape[0])).to(y.device)
    return (t * 10.0 + u * 1e-4).contiguous()


def wide_gram(x, eigensolver="full"):
    """(mean, s, K) of a resident wide matrix, as WidePCA.gram forms it: what wide_knn_graph and WidePCA both start from.  The
    free memory of the device is checked first, as for a WidePCA(eigensolver=eigensolver) fit (K, and eigh's 3 N^2 float64,
    which exceed the graph's fp32 panel)."""
    from .pca import WidePCA
    WidePCA._check_memory(x.device, x.shape[0], x.shape[1], resident=True, eigensolver=eigensolver)
    return WidePCA().gram(x)


def pca_coordinates(X, device=None, gram=None, consume_gram=False, eigensolver="full"):
    """The first two principal-component scores of X from this package's PCA(n_components=2): init="pca" before rescaling.
    More than knn.MAX_FEATURES columns: WidePCA(n_components=2), from gram=(mean, s, K) = wide_gram(x) when it is given (K is
    left unchanged unless consume_gram).  eigensolver: "full" or "partial", handed to the PCA."""
    if _knn.is_wide(X):
        from .pca import WidePCA
        return WidePCA(n_components=2, device=device, eigensolver=eigensolver).fit_transform(X, gram=gram,
                                                                                             consume_gram=consume_gram)
    from .pca import PCA
    return PCA(n_components=2, device=device, eigensolver=eigensolver).fit_transform(X)


pca_init = pca_coordinates      # init="pca"


# ---------------------------------------------------------------------------------------------------------- the device
def fuzzy_graph(knn_indices, knn_dists, device=None):
    """The fuzzy simplicial set of a k-NN graph as fit_knn / knn_graph(include_self=True) return it: (indptr int64, indices
    int32, data float32, rho float32, sigma float32) on the device."""
    idx, dist = check_graph(knn_indices, knn_dists)
    dev = device_of(knn_dists, device)
    with torch.no_grad(), torch.cuda.device(dev):
        i32 = torch.from_numpy(idx.astype(np.int32)).to(dev)
        d = torch.from_numpy(dist).to(dev)
        rho, sigma, _, _ = ops.umap_smooth(d)
        a = ops.umap_membership(i32, d, rho, sigma)
        indptr, cols, w = symmetrize(i32, a)
    return indptr, cols, w, rho, sigma


DEFAULT_TRANSFORM_CHUNK_ROWS = 16384


class UMAPEmbedding:
    """fit_transform(X) / fit_graph(knn_indices, knn_dists, init) leave embedding_ (N, 2) float32 numpy; graph() is the fuzzy
    set as a scipy CSR matrix.  a, b: the curve parameters as given (the reference's 1.58, 0.9).  A model fitted by
    fit_transform, or by fit_graph(..., X=X), also keeps its training matrix and places new rows into the embedding with
    transform(Q); it pickles with its state on the host."""

    def __init__(self, n_neighbors=15, a=1.58, b=0.9, n_epochs=None, negative_sample_rate=5, gamma=1.0, init="pca", seed=0,
                 n_components=2, device=None, init_eigensolver="full"):
        if int(n_components) != 2:
            raise ValueError(f"the layout has two output dimensions, got n_components={n_components}")
        if int(n_neighbors) < 2 or int(n_neighbors) > MAX_K:
            raise ValueError(f"n_neighbors = {n_neighbors} is outside 2 .. {MAX_K}")
        if not (a > 0 and b > 0):
            raise ValueError(f"a = {a} and b = {b} must be positive")
        if n_epochs is not None and int(n_epochs) < 1:
            raise ValueError(f"n_epochs = {n_epochs} must be at least 1")
        if int(negative_sample_rate) < 1 or int(negative_sample_rate) > 1000:
            raise ValueError(f"negative_sample_rate = {negative_sample_rate} is outside 1 .. 1000")
        if not isinstance(init, str) and np.ndim(init) == 2 and np.shape(init)[1] != 2:
            raise ValueError(f"the layout has two output dimensions; init has shape {np.shape(init)}")
        if isinstance(init, str) and init != "pca":
            raise ValueError(f"init={init!r}: 'pca' or an (N, 2) array (spectral initialisation is not built)")
        self.n_neighbors, self.a, self.b = int(n_neighbors), float(a), float(b)
        self.n_epochs = None if n_epochs is None else int(n_epochs)
        self.negative_sample_rate, self.gamma, self.init, self.seed = int(negative_sample_rate), float(gamma), init, int(seed)
        self.device = device
        self.init_eigensolver = init_eigensolver    # the eigensolver of init="pca": "full" or "partial" (pca.PCA's)
        self.group = 0              # lanes per vertex of dm_umap_epoch (0: chosen by the library; no effect on the result)
        self.transform_group = 0    # the same for dm_umap_transform_layout
        self._X = None              # the training matrix (M, F) fp32: the resident device tensor of the fit, or host numpy

    def fit_transform(self, X):
        """The exact k-NN graph of X at n_neighbors (knn.knn_graph; knn.wide_knn_graph above knn.MAX_FEATURES columns), then
        fit_graph; returns embedding_."""
        N = X.shape[0]
        if self.n_neighbors > N:
            raise ValueError(f"n_neighbors = {self.n_neighbors} exceeds the {N} rows of X")
        init = self.init
        if not isinstance(init, str):
            init = _check_init(init, N)
        wide = _knn.is_wide(X)
        if wide:
            _knn._check_wide(N, X.shape[1], self.n_neighbors, N)
        x = _knn._resident(X, self.device)
        if not wide:
            idx, dist = _knn.knn_graph(x, self.n_neighbors, include_self=True)
            if isinstance(init, str):
                init = pca_coordinates(x, eigensolver=self.init_eigensolver)
        elif isinstance(init, str):                 # one row Gram matrix: the graph's filter first, then the PCA uses it up
            with torch.no_grad(), torch.cuda.device(x.device):
                g = wide_gram(x, eigensolver=self.init_eigensolver)
            idx, dist = _knn.wide_knn_graph(x, self.n_neighbors, include_self=True, gram=g)
            init = pca_coordinates(x, gram=g, consume_gram=True, eigensolver=self.init_eigensolver)
            del g
        else:
            idx, dist = _knn.wide_knn_graph(x, self.n_neighbors, include_self=True)
        self.fit_graph(idx, dist, init)
        self._X = x
        return self.embedding_

    def fit_graph(self, knn_indices, knn_dists, init=None, X=None):
        """Fit from a k-NN graph (column 0 the row itself); init: an (N, 2) array of coordinates before rescaling (the PCA
        scores of pca_coordinates(X) for init="pca").  X: the (N, F) matrix the graph was computed from, kept (a device tensor
        as it is) so that transform can place new rows; without it the model has an embedding only.  Returns self."""
        idx, dist = check_graph(knn_indices, knn_dists)
        N = idx.shape[0]
        if X is not None and (len(X.shape) != 2 or X.shape[0] != N):
            raise ValueError(f"X has shape {tuple(X.shape)}, the graph has {N} rows")
        init = self.init if init is None else init
        if isinstance(init, str):
            _check_init(init, N)
            raise ValueError("fit_graph has no data to compute init='pca' from: pass init=pca_coordinates(X) or use fit_transform")
        y0 = _check_init(init, N)
        n_epochs = default_n_epochs(N) if self.n_epochs is None else self.n_epochs
        dev = device_of(None, self.device)
        with torch.no_grad(), torch.cuda.device(dev):
            indptr, cols, w, rho, sigma = fuzzy_graph(idx, dist, device=dev)
            self._graph = (indptr.cpu().numpy(), cols.cpu().numpy(), w.cpu().numpy(), N)
            self.rho_, self.sigma_ = rho.cpu().numpy(), sigma.cpu().numpy()
            p_indptr, p_cols, p_w = prune(indptr, cols, w, n_epochs)
            eps, eps_neg = schedule(p_w, self.negative_sample_rate)
            nxt, nxt_neg = eps.clone(), eps_neg.clone()
            y = init_layout(torch.from_numpy(y0).to(dev), self.seed)
            self.init_ = y.cpu().numpy()
            other = torch.empty_like(y)
            for n in range(n_epochs):
                ops.umap_epoch(p_indptr, p_cols, eps, eps_neg, nxt, nxt_neg, y, other, n, n_epochs, self.a, self.b, self.gamma,
                               self.seed, self.group)
                y, other = other, y
            self.embedding_ = y.cpu().numpy()
        self.n_epochs_ = n_epochs
        self._X = X
        return self

    # ------------------------------------------------------------------------------------- transform (section 3.5d)
    def _fitted(self, need_data):
        if getattr(self, "embedding_", None) is None or getattr(self, "n_epochs_", None) is None:
            raise ValueError("the model has no embedding: fit it first")
        if need_data and self._X is None:
            raise ValueError("the model has no training data: fit it with fit_transform or fit_graph(..., X=X)")
        return self.embedding_.shape[0]

    def _transform_args(self, n_epochs, seed, row_offset):
        n_epochs = max(1, self.n_epochs_ // 3) if n_epochs is None else int(n_epochs)
        if n_epochs < 1:
            raise ValueError(f"n_epochs = {n_epochs} must be at least 1")
        if int(row_offset) < 0:
            raise ValueError(f"row_offset = {row_offset} is negative")
        return n_epochs, self.seed if seed is None else int(seed), int(row_offset)

    def _place(self, idx, dist, y_train, n_epochs, seed, row_offset):
        """prepare and one layout launch for a checked host graph: device (y (R, 2), sigma (R,), y0 (R, 2))."""
        dev = y_train.device
        i32 = torch.from_numpy(idx.astype(np.int32)).to(dev)
        d = torch.from_numpy(dist).to(dev)
        sigma, _, eps, eps_neg, nxt, nxt_neg, y0 = ops.umap_transform_prepare(i32, d, y_train, n_epochs, self.negative_sample_rate)
        y = y0.clone()
        ops.umap_transform_layout(i32, eps, eps_neg, nxt, nxt_neg, y_train, y, 0, n_epochs, n_epochs, row_offset, seed, self.a,
                                  self.b, self.gamma, self.transform_group)
        return y, sigma, y0

    def transform_graph(self, knn_indices, knn_dists, n_epochs=None, seed=None, row_offset=0):
        """(R, 2) float32 numpy: the rows of a query graph -- the k = n_neighbors nearest training rows of every query and
        their distances, sorted, as knn.knn_query returns them -- placed into the fitted embedding.  n_epochs: default
        max(1, n_epochs_ // 3); seed: default the model's; row_offset: the global number of row 0 (a row's result depends
        on its number, not on the other rows of the call).  Leaves sigma_t_ (R,) and init_t_ (R, 2)."""
        M = self._fitted(need_data=False)
        idx, dist = check_query_graph(knn_indices, knn_dists, M)
        n_epochs, seed, row_offset = self._transform_args(n_epochs, seed, row_offset)
        dev = device_of(None, self.device)
        with torch.no_grad(), torch.cuda.device(dev):
            y, sigma, y0 = self._place(idx, dist, torch.from_numpy(self.embedding_).to(dev), n_epochs, seed, row_offset)
            self.sigma_t_, self.init_t_ = sigma.cpu().numpy(), y0.cpu().numpy()
            return y.cpu().numpy()

    def transform(self, Q, n_epochs=None, seed=None, row_offset=0, chunk_rows=DEFAULT_TRANSFORM_CHUNK_ROWS):
        """(R, 2) float32 numpy: the rows of Q (R, F) placed into the fitted embedding -- the exact query graph against the
        training matrix (knn.knn_query), then transform_graph's steps, chunk_rows rows at a time, so that Q may be larger
        than the device holds.  The result of a row depends on the row, its global number row_offset + i, the seed and the
        model alone: not on chunk_rows and not on the other rows."""
        M = self._fitted(need_data=True)
        F = self._X.shape[1]
        shape = shape_of(Q)
        if len(shape) != 2 or shape[1] != F:
            raise ValueError(f"Q has shape {shape}, expected (n, {F})")
        if shape[0] < 1:
            raise ValueError("Q has no rows")
        if self.n_neighbors > M:
            raise ValueError(f"n_neighbors = {self.n_neighbors} exceeds the {M} training rows")
        if self._X.shape[0] != M:
            raise ValueError(f"the training matrix has {self._X.shape[0]} rows, the embedding {M}")
        n_epochs, seed, row_offset = self._transform_args(n_epochs, seed, row_offset)
        cr = max(1, int(chunk_rows))
        if not torch.is_tensor(Q):
            Q = np.asarray(Q)
        x = self._X = _knn._resident(self._X, self.device)
        wide = F > _knn.MAX_FEATURES
        with torch.no_grad(), torch.cuda.device(x.device):
            shift = _knn.column_shift(x)
            y_train = torch.from_numpy(self.embedding_).to(x.device)
            ys, sigmas, inits = [], [], []
            for lo in range(0, shape[0], cr):
                if wide:
                    idx, dist = _knn.wide_knn_query(x, Q[lo:lo + cr], self.n_neighbors, shift=shift)
                else:
                    idx, dist = _knn.knn_query(x, Q[lo:lo + cr], self.n_neighbors, shift=shift)
                idx, dist = check_query_graph(idx, dist, M)
                y, sigma, y0 = self._place(idx, dist, y_train, n_epochs, seed, row_offset + lo)
                ys.append(y.cpu().numpy())
                sigmas.append(sigma.cpu().numpy())
                inits.append(y0.cpu().numpy())
        self.sigma_t_, self.init_t_ = np.concatenate(sigmas), np.concatenate(inits)
        return np.concatenate(ys)

    # ------------------------------------------------------------------------------------------------------ pickling
    def __getstate__(self):
        """Host state only: the training matrix as fp32 numpy (N x F x 4 bytes: 5.2 GB for 20 000 rows of 65536 features), the
        embedding, the parameters and the fitted graph."""
        state = dict(self.__dict__)
        X = state.get("_X")
        if torch.is_tensor(X):
            state["_X"] = X.detach().cpu().numpy().astype(np.float32, copy=False)
        elif X is not None:
            state["_X"] = np.ascontiguousarray(X, dtype=np.float32)
        if torch.is_tensor(state.get("init")):
            state["init"] = state["init"].detach().cpu().numpy()
        state["device"] = None if state.get("device") is None else str(state["device"])
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        self.__dict__.setdefault("_X", None)
        self.__dict__.setdefault("transform_group", 0)
        self.__dict__.setdefault("init_eigensolver", "full")

    def graph(self):
        """The fuzzy simplicial set W (N, N) as scipy.sparse.csr_matrix (float32)."""
        import scipy.sparse as sp
        indptr, cols, w, N = self._graph
        return sp.csr_matrix((w, cols, indptr), shape=(N, N))
