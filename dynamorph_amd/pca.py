"""Latent PCA on the GPU: a drop-in for the sklearn.decomposition.PCA(0.5) of run_dim_reduction.py (fit_PCA, lines 14-50;
process_PCA, lines 52-92).

The fit follows scikit-learn's covariance route (sklearn/decomposition/_pca.py::_fit_full) with the covariance formed on the
device: fp64 column sums (dm_pca_colsum), then the centred Gram matrix (X - s)^T (X - s) for the fp32 shift s = fp32(mean)
(dm_pca_gram), corrected in float64 for the rounding of s.  Host data are streamed in chunks through pinned staging and the
chunks merged with the pairwise (Chan) update, so the data cross PCIe once.  Finalisation -- eigendecomposition, component
count, signs -- is plain float64 torch and runs on a CPU tensor as well.  Every fitted attribute follows scikit-learn's names
and conventions, so PCA(0.5) here chooses the components and signs the reference's call chooses.

Latents wider than MAX_FEATURES (VQ_VAE_z32: 65536 features) take the sample-space route of WidePCA: the N x N matrix
K = (X - s)(X - s)^T (dm_pca_rowgram) has the covariance's non-zero spectrum, and its eigenvectors U give the components as
Lambda^(-1/2) U^T (X - s) (dm_pca_components).  finalize_samples / orient_components are its float64 finalisation.
"""
import numpy as np
import torch

from . import ops
from .rows import device_chunks, device_of, host_rows

MAX_FEATURES = 16384           # DM_PCA_MAX_FEATURES
MAX_COMPONENTS = 512           # DM_PCA_MAX_COMPONENTS (one transform launch; more are done in blocks of this many)
WIDE_MAX_SAMPLES = 24576       # DM_PCA_WIDE_MAX_SAMPLES
WIDE_MAX_FEATURES = 1 << 20    # DM_PCA_WIDE_MAX_FEATURES
_ATTRS = ("mean_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_",
          "noise_variance_", "n_components_", "n_samples_", "n_features_in_")


def _check_n_components(n_components):
    if isinstance(n_components, str):
        raise ValueError(f"n_components={n_components!r} is not supported (only a fraction in (0, 1), an int or None)")
    if n_components is None:
        return
    if isinstance(n_components, (bool, np.bool_)):
        raise ValueError(f"n_components={n_components!r} is not a number")
    if isinstance(n_components, (int, np.integer)):
        if n_components < 1:
            raise ValueError(f"n_components={n_components} must be >= 1")
        return
    if isinstance(n_components, (float, np.floating)):
        if not 0.0 < float(n_components) < 1.0:
            raise ValueError(f"n_components={n_components} as a float must lie in (0, 1)")
        return
    raise ValueError(f"n_components={n_components!r} is not supported")


def _check_shape(N, F):
    if N < 2:
        raise ValueError(f"PCA needs at least 2 samples, got {N}")
    if F < 1:
        raise ValueError("PCA needs at least 1 feature")
    if F > MAX_FEATURES:
        raise ValueError(f"PCA on the GPU supports up to {MAX_FEATURES} features, got {F}: this covers the VQ_VAE / VQ_VAE_z16 "
                         f"latents up to embedding_dim 64, not the VQ_VAE_z32 latents of 65536 features (their float64 "
                         f"covariance alone is 34 GB)")


def _int_components(n_components, N, F):
    """An integer n_components as it is: at most min(N, F)."""
    m = min(N, F)
    if n_components > m:
        raise ValueError(f"n_components={n_components} must be between 0 and min(n_samples, n_features)={m}")
    return int(n_components)


def select_n_components(n_components, ratio, N, F):
    """_fit_full's rule: a fraction -> searchsorted(cumsum(ratio), frac, side='right') + 1; an int as it is (<= min(N, F));
    None -> min(N, F).  `ratio`: explained_variance_ratio_ of all components, float64 numpy."""
    _check_n_components(n_components)
    if n_components is None:
        return min(N, F)
    if isinstance(n_components, (int, np.integer)):
        return _int_components(n_components, N, F)
    cum = np.cumsum(np.asarray(ratio, dtype=np.float64))
    return int(np.searchsorted(cum, float(n_components), side="right") + 1)


def merge_moments(n, mean, C, n_c, mean_c):
    """Pairwise (Chan) merge of a chunk into running moments: C already holds sum G + G_c (the chunk's centred Gram matrix
    was accumulated into it); this adds n n_c / (n + n_c) d d^T, d = mean_c - mean, and returns (n + n_c, merged mean).
    float64 tensors on any device."""
    if n == 0:
        return n_c, mean_c.clone()
    tot = n + n_c
    d = mean_c - mean
    C.add_(torch.outer(d, d), alpha=n * n_c / tot)
    return tot, mean + d * (n_c / tot)


EIGENSOLVERS = ("full", "partial")
EIG_BLOCK = 32                 # the partial solver's first block; a matrix of order <= 2 EIG_BLOCK takes the full route


def _check_eigensolver(eigensolver):
    if eigensolver not in EIGENSOLVERS:
        raise ValueError(f"eigensolver={eigensolver!r}: one of {EIGENSOLVERS}")


def _leading_pairs(M, n_components, N, F, eigensolver):
    """The partial route: (theta (k,) descending clipped at 0, V (order, k), trace, info) of the symmetric float64 matrix M
    from eig.top_eigenpairs -- or None where the full route is taken: eigensolver="full", n_components=None, a matrix of
    order <= 2 EIG_BLOCK, or a solve that eig.NotApplicable / eig.NotConverged gave up on."""
    if eigensolver != "partial" or n_components is None or M.shape[0] <= 2 * EIG_BLOCK:
        return None
    from . import eig
    if isinstance(n_components, (int, np.integer)):
        want = {"k": _int_components(n_components, N, F)}
    else:
        want = {"fraction": float(n_components)}
    trace = float(torch.diagonal(M).sum(dtype=torch.float64))
    try:
        theta, V, info = eig.top_eigenpairs(M, trace=trace, block=EIG_BLOCK, **want)
    except (eig.NotApplicable, eig.NotConverged):
        return None
    return theta.clamp_min(0.0), V, trace, info


def _eigenpairs(M, n_components, N, F, eigensolver):
    """(lam descending clipped at 0, V (order, len(lam)), trace, info) of the symmetric float64 matrix M: the partial route's
    leading pairs (_leading_pairs), or from eigh the top min(N, F) pairs -- the spectrum of the full SVD that _fit_full's
    'full' solver computes -- with trace None."""
    part = _leading_pairs(M, n_components, N, F, eigensolver)
    if part is not None:
        return part
    evals, evecs = torch.linalg.eigh(M)
    m = min(N, F)
    return torch.flip(evals, (0,))[:m].clamp_min(0.0), torch.flip(evecs, (1,))[:, :m], None, None


def _attrs(ev, ratio, singular, noise, N, F, route, info=None):
    """The fitted attributes that need no eigenvector, of the ev.shape[0] components kept."""
    return {
        "explained_variance_": ev,
        "explained_variance_ratio_": ratio,
        "singular_values_": singular,
        "noise_variance_": noise,
        "n_components_": int(ev.shape[0]),
        "n_samples_": int(N),
        "n_features_in_": int(F),
        "eigensolver_": route,
        "eig_info_": info,
    }


def _full_attrs(ev, n_components, N, F):
    """The full route: from the explained variances of all min(N, F) components (numpy), by scikit-learn's expressions."""
    ratio = ev / ev.sum() if ev.sum() > 0 else np.zeros_like(ev)
    k = select_n_components(n_components, ratio, N, F)
    noise = float(ev[k:].mean()) if k < min(N, F) else 0.0
    return _attrs(ev[:k].copy(), ratio[:k].copy(), np.sqrt(ev[:k] * (N - 1)), noise, N, F, "full")


def _partial_attrs(theta, trace, N, F, info):
    """The partial route: from the leading eigenvalues theta (numpy, clipped) and the trace, which stands in for the rest."""
    k, m = theta.shape[0], min(N, F)
    noise = max(float(trace - theta.sum()), 0.0) / (N - 1) / (m - k) if k < m else 0.0
    return _attrs(theta / (N - 1), theta / trace if trace > 0 else np.zeros_like(theta), np.sqrt(theta), noise, N, F,
                  "partial", info)


def _svd_flip(V):
    """svd_flip(u_based_decision=False) on the rows of V: the entry of largest magnitude of each row becomes positive.  In
    place; returns V."""
    idx = V.abs().argmax(dim=1)
    signs = torch.sign(V.gather(1, idx[:, None]))
    signs[signs == 0] = 1.0
    V *= signs
    return V


def finalize(C, mean, N, n_components=0.5, eigensolver="full"):
    """From the float64 scatter matrix C = sum (x - mean)(x - mean)^T (F x F, any device) to scikit-learn's fitted attributes
    (a dict of float64 numpy arrays and ints).  eigh in float64 on C's device; eigenvalues clipped at 0; the top min(N, F)
    eigenpairs are kept (_eigenpairs); signs by _svd_flip.

    eigensolver="partial": only the leading pairs, from eig.top_eigenpairs (_leading_pairs); ratios against the trace and
    the noise variance from the trace's remainder.  "eigensolver_" names the route taken, "eig_info_" the solver's record."""
    F = C.shape[0]
    _check_shape(N, F)
    _check_n_components(n_components)
    _check_eigensolver(eigensolver)
    C = C.to(torch.float64)
    mean = mean.to(torch.float64).cpu().numpy() if torch.is_tensor(mean) else np.asarray(mean, np.float64)
    lam, V, trace, info = _eigenpairs(C, n_components, N, F, eigensolver)
    if trace is None:
        attrs = _full_attrs((lam / (N - 1)).cpu().numpy(), n_components, N, F)
    else:
        attrs = _partial_attrs(lam.cpu().numpy(), trace, N, F, info)
    comps = _svd_flip(V.T.contiguous())                                   # rows are components
    attrs.update(mean_=mean, components_=comps[:attrs["n_components_"]].cpu().numpy())
    return attrs


def _check_wide_shape(N, F):
    if N < 2:
        raise ValueError(f"PCA needs at least 2 samples, got {N}")
    if F < 1:
        raise ValueError("PCA needs at least 1 feature")
    if F > WIDE_MAX_FEATURES:
        raise ValueError(f"PCA on the GPU supports up to {WIDE_MAX_FEATURES} features, got {F}")
    if N > WIDE_MAX_SAMPLES:
        raise ValueError(f"PCA of {N} samples of {F} features: more than {MAX_FEATURES} features need the sample-space route, "
                         f"which holds all rows and their {N} x {N} float64 Gram matrix on the device and supports up to "
                         f"{WIDE_MAX_SAMPLES} samples")


def finalize_samples(K, N, F, n_components=0.5, eigensolver="full"):
    """The sample-space finalisation: from the float64 matrix K = (X - s)(X - s)^T (N x N, any device, s any shift) to the
    fitted attributes that do not need X (a dict as finalize returns, without mean_ and components_) and "W": the
    (n_components_, N) float64 tensor (U_k / sqrt(lambda_k))^T on K's device, whose product with X - s is the components.

    K is double-centred in float64 -- K - row means - column means + grand mean = (X - mean)(X - mean)^T whatever s was --
    in place.  eigh in float64 on K's device; eigenvalues clipped at 0; the top min(N, F) are the spectrum of the full SVD
    _fit_full's 'full' solver computes.  A requested component whose eigenvalue is at most N 2^-52 lambda_max is not
    defined (centred data have rank <= N - 1): ValueError.

    eigensolver="partial": the leading pairs only, as in finalize; "eigensolver_" names the route taken."""
    _check_wide_shape(N, F)
    _check_n_components(n_components)
    _check_eigensolver(eigensolver)
    if tuple(K.shape) != (N, N) or K.dtype != torch.float64:
        raise ValueError(f"K has shape {tuple(K.shape)} and dtype {K.dtype}, need a float64 ({N}, {N})")
    rm = K.mean(dim=1)
    cm = K.mean(dim=0)
    gm = rm.mean()
    K -= rm[:, None]
    K -= cm[None, :]
    K += gm
    lam, V, trace, info = _eigenpairs(K, n_components, N, F, eigensolver)
    lam_h = lam.cpu().numpy()
    attrs = _full_attrs(lam_h / (N - 1), n_components, N, F) if trace is None else _partial_attrs(lam_h, trace, N, F, info)
    k = attrs["n_components_"]
    rank = int((lam_h > N * 2.0 ** -52 * lam_h[0]).sum())
    if k > rank:
        raise ValueError(f"n_components={n_components!r} asks for {k} components of {N} samples, but at most {rank} "
                         f"components are defined (the others have zero variance: centred data have rank <= n_samples - 1)")
    attrs["W"] = (V[:, :k] / lam[:k].sqrt()).T.contiguous()
    return attrs


def orient_components(V):
    """Rows of V (k x F float64 tensor) scaled to unit length and signed by _svd_flip, as finalize signs them.  In place;
    returns V."""
    V /= torch.linalg.vector_norm(V, dim=1, keepdim=True)
    return _svd_flip(V)


def column_mean(x):
    """float64 column mean (F,) of a resident fp32 matrix of any width: dm_pca_colsum per block of MAX_FEATURES columns."""
    N, F = x.shape
    sums = [ops.pca_colsum(x[:, lo:min(lo + MAX_FEATURES, F)]) for lo in range(0, F, MAX_FEATURES)]
    return (sums[0] if len(sums) == 1 else torch.cat(sums)) / N


class PCA:
    """PCA(n_components=0.5, whiten=False): fit / transform / fit_transform on the GPU with scikit-learn's attributes.

    X: a CUDA tensor (used in place: fp32, unit column stride) or host data (numpy array / CPU tensor, streamed in chunks of
    `chunk_rows` rows through pinned staging).  transform returns a CUDA fp32 tensor."""

    _check_shape = staticmethod(_check_shape)
    # eigensolver: "full" (eigh of the whole matrix) or "partial" (eig.top_eigenpairs where it applies: _leading_pairs);
    # eigensolver_ / eig_info_: the route the last fit took and the partial solver's record.  Not part of the pickle.
    eigensolver = "full"
    eigensolver_ = None
    eig_info_ = None

    def __init__(self, n_components=0.5, whiten=False, chunk_rows=65536, device=None, eigh_device="cuda", eigensolver="full"):
        if whiten:
            raise ValueError("PCA(whiten=True) is not supported")
        _check_n_components(n_components)
        _check_eigensolver(eigensolver)
        self.eigensolver = eigensolver
        self.n_components = n_components
        self.whiten = False
        self.chunk_rows = int(chunk_rows)
        self.device = device
        self.eigh_device = eigh_device      # 'cuda' (the fit's device) or 'cpu'
        self._dev = {}

    # ------------------------------------------------------------------------------------------------------ fitting
    def moments(self, X, chunk_rows=None):
        """(N, mean (F,) float64, C (F, F) float64 = sum (x - mean)(x - mean)^T) on the device."""
        if torch.is_tensor(X) and X.is_cuda:
            if X.dim() != 2:
                raise ValueError(f"PCA expects a 2-D (samples, features) array, got shape {tuple(X.shape)}")
            N, F = X.shape
            _check_shape(N, F)
            with torch.cuda.device(X.device):
                return (N,) + self._chunk_moments(X)
        X = host_rows(X)
        N, F = X.shape
        _check_shape(N, F)
        return self._stream_moments(X, int(chunk_rows or self.chunk_rows))

    @staticmethod
    def _chunk_moments(x, G=None, accumulate=False, ws=None):
        """mean (fp64) of the chunk and its centred Gram matrix, (+)= into G: shifted by s = fp32(mean) in the kernel, then
        corrected by -n (mean - s)(mean - s)^T in float64."""
        n = x.shape[0]
        mean = ops.pca_colsum(x) / n
        s = mean.float()
        G = ops.pca_gram(x, s, G=G, accumulate=accumulate, workspace=ws)
        d = mean - s.double()
        G.add_(torch.outer(d, d), alpha=-n)
        return mean, G

    def _stream_moments(self, X, chunk_rows):
        N, F = X.shape
        dev = device_of(X, self.device)
        cr = max(2, min(chunk_rows, N))
        with torch.no_grad(), torch.cuda.device(dev):
            ws = torch.empty(max(ops.L.load().dm_pca_gram_workspace_bytes(cr, F), 8) // 8, dtype=torch.float64, device=dev)
            C = torch.zeros((F, F), dtype=torch.float64, device=dev)
            n, mean = 0, None
            for _, x in device_chunks(X, cr, dev):
                m = x.shape[0]
                mean_c, _ = self._chunk_moments(x, G=C, accumulate=True, ws=ws)
                n, mean = merge_moments(n, mean, C, m, mean_c) if mean is not None else (m, mean_c)
            torch.cuda.current_stream().synchronize()
        return n, mean, C

    def fit(self, X, chunk_rows=None):
        N, mean, C = self.moments(X, chunk_rows)
        if self.eigh_device == "cpu":
            C = C.cpu()
        self._set(finalize(C, mean, N, self.n_components, self.eigensolver), device_of(X, self.device))
        return self

    def fit_transform(self, X, chunk_rows=None):
        return self.fit(X, chunk_rows).transform(X)

    # ---------------------------------------------------------------------------------------------------- applying
    def _set(self, attrs, device=None):
        for a in _ATTRS:
            setattr(self, a, attrs[a])
        self.eigensolver_, self.eig_info_ = attrs.get("eigensolver_"), attrs.get("eig_info_")
        self._dev = {}
        self._home = device

    def _operands(self, device):
        key = str(device)
        if key not in self._dev:
            V = torch.as_tensor(np.ascontiguousarray(self.components_, dtype=np.float32)).to(device)
            # the shift is fp32(mean); the projection of (mean - fp32(mean)) is removed in float64 afterwards
            mean = np.asarray(self.mean_, dtype=np.float64)
            s = mean.astype(np.float32)
            corr = (mean - s.astype(np.float64)) @ np.asarray(self.components_, np.float64).T
            corr = torch.as_tensor(corr.astype(np.float32)).to(device) if np.any(corr != 0) else None
            self._dev[key] = (V, torch.as_tensor(s).to(device), corr)
        return self._dev[key]

    def _device_rows(self, X):
        """X as the fp32 device matrix (n, n_features_in_) the kernels read."""
        if not hasattr(self, "components_"):
            raise ValueError("this PCA instance is not fitted yet")
        if torch.is_tensor(X) and X.is_cuda:
            x = X if X.dtype == torch.float32 else X.float()
        else:
            x = host_rows(X)
            dev = self._home if getattr(self, "_home", None) is not None else device_of(x, self.device)
            x = x.to(dev, dtype=torch.float32)
        if x.dim() != 2 or x.shape[1] != self.n_features_in_:
            raise ValueError(f"X has shape {tuple(x.shape)}, expected (n, {self.n_features_in_})")
        return x

    def transform(self, X):
        """(X - mean_) components_^T as a CUDA fp32 tensor (N, n_components_)."""
        x = self._device_rows(X)
        V, s, corr = self._operands(x.device)
        with torch.cuda.device(x.device):
            k = V.shape[0]
            if k <= MAX_COMPONENTS:
                Y = ops.pca_transform(x, V, s)
            else:
                Y = torch.cat([ops.pca_transform(x, V[j:j + MAX_COMPONENTS], s) for j in range(0, k, MAX_COMPONENTS)], 1)
            if corr is not None:
                Y -= corr
        return Y

    # ------------------------------------------------------------------------------------------- scikit-learn interchange
    def to_sklearn(self, dtype=np.float32):
        """A fitted sklearn.decomposition.PCA(n_components, svd_solver='auto', whiten=False) with these attributes (float32
        by default: what a fit on the float32 latents leaves, so its .transform of them is float32 as well)."""
        try:
            from sklearn.decomposition import PCA as SkPCA
        except ImportError as e:
            raise ImportError("to_sklearn needs scikit-learn, which is not importable here") from e
        sk = SkPCA(n_components=self.n_components, svd_solver="auto", whiten=False)
        for a in _ATTRS:
            v = getattr(self, a)
            if isinstance(v, np.ndarray):
                v = v.astype(dtype)
            elif a == "noise_variance_":
                v = dtype(v)
            setattr(sk, a, v)
        sk._fit_svd_solver = "full"
        return sk

    @classmethod
    def from_sklearn(cls, obj, device=None):
        """Apply a fitted sklearn PCA (e.g. the reference's pca_model.pkl) on the GPU."""
        if getattr(obj, "whiten", False):
            raise ValueError("PCA(whiten=True) is not supported")
        self = cls(n_components=obj.n_components if not isinstance(obj.n_components, str) else None, device=device)
        attrs = {}
        for a in _ATTRS:
            v = getattr(obj, a)
            attrs[a] = np.asarray(v, np.float64).copy() if isinstance(v, np.ndarray) else v
        attrs["noise_variance_"] = float(attrs["noise_variance_"])
        for a in ("n_components_", "n_samples_", "n_features_in_"):
            attrs[a] = int(attrs[a])
        cls._check_shape(2, attrs["n_features_in_"])
        self._set(attrs)
        return self

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_dev"] = {}
        st["_home"] = None
        for a in ("eigensolver", "eigensolver_", "eig_info_"):
            st.pop(a, None)
        return st


class WidePCA(PCA):
    """PCA for latents of more than MAX_FEATURES features (the VQ_VAE_z32 latents: 65536) and up to WIDE_MAX_SAMPLES rows,
    by the sample-space route: K = (X - s)(X - s)^T (N x N float64, dm_pca_rowgram), double-centred and decomposed in
    float64, components Lambda^(-1/2) U^T (X - s) (dm_pca_components).  Same constructor, attributes, methods and pickle
    as PCA.  All row pairs are needed, so host data are uploaded (in chunks of rows through pinned staging) into one
    resident fp32 matrix instead of being streamed."""

    _check_shape = staticmethod(_check_wide_shape)
    STAGE_BYTES = 1 << 28               # pinned staging: two buffers of at most this many bytes

    # ------------------------------------------------------------------------------------------------------ fitting
    def _resident(self, X):
        """X as one fp32 matrix on the device: a CUDA tensor as it lies (fp32, unit column stride), host data uploaded."""
        if torch.is_tensor(X) and X.is_cuda:
            if X.dim() != 2:
                raise ValueError(f"PCA expects a 2-D (samples, features) array, got shape {tuple(X.shape)}")
            _check_wide_shape(*X.shape)
            self._check_memory(X.device, X.shape[0], X.shape[1], resident=True, eigensolver=self.eigensolver)
            return X if X.dtype == torch.float32 else X.float()
        X = host_rows(X)
        N, F = X.shape
        _check_wide_shape(N, F)
        dev = device_of(X, self.device)
        self._check_memory(dev, N, F, resident=False, eigensolver=self.eigensolver)
        with torch.no_grad(), torch.cuda.device(dev):
            x = torch.empty((N, F), dtype=torch.float32, device=dev)
            if X.dtype == torch.float32 and X.is_contiguous() and X.is_pinned():
                x.copy_(X, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                return x
            cr = max(1, min(self.chunk_rows, N, self.STAGE_BYTES // (4 * F)))
            stage = [torch.empty((cr, F), dtype=torch.float32, pin_memory=True) for _ in range(2)]
            ev_in = [torch.cuda.Event() for _ in range(2)]       # chunk has left staging k
            for it, lo in enumerate(range(0, N, cr)):
                k = it & 1
                m = min(cr, N - lo)
                ev_in[k].synchronize()
                stage[k][:m].copy_(X[lo:lo + m])
                x[lo:lo + m].copy_(stage[k][:m], non_blocking=True)
                ev_in[k].record()
            torch.cuda.current_stream().synchronize()
        return x

    @staticmethod
    def _check_memory(dev, N, F, resident, eigensolver="full"):
        """X (unless it is on the device already), K, the row Gram's workspace and eigh's eigenvectors and workspace
        (taken as 3 N^2 float64) against the free memory of the device.  eigensolver="partial": instead of eigh's, the
        solver's blocks (taken as 8 of N x 256 float64: Q, A Q, the Ritz vectors and their images, the QR's copies) and
        dm_eig_apply's workspace; a fit that falls back to the full route allocates eigh's storage unchecked."""
        need_x = 0 if resident else 4 * N * F
        need_k = 8 * N * N
        need_ws = max(int(ops.L.load().dm_pca_rowgram_workspace_bytes(N, F)), 0)
        if eigensolver == "partial":
            need_eigh = 8 * 8 * N * ops.EIG_MAX_BLOCK + max(int(ops.L.load().dm_eig_apply_workspace_bytes(N, ops.EIG_MAX_BLOCK)), 0)
        else:
            need_eigh = 3 * 8 * N * N
        free, _ = torch.cuda.mem_get_info(dev)
        need = need_x + need_k + max(need_ws, need_eigh)
        if need > free:
            raise ValueError(f"PCA of {N} samples of {F} features needs {need / 2**30:.1f} GiB on the device (X "
                             f"{need_x / 2**30:.1f}, K {need_k / 2**30:.1f}, row-Gram workspace {need_ws / 2**30:.1f}, eigh "
                             f"{need_eigh / 2**30:.1f} GiB), {free / 2**30:.1f} GiB are free")

    @staticmethod
    def _blocks(F):
        return [(lo, min(lo + MAX_FEATURES, F)) for lo in range(0, F, MAX_FEATURES)]

    def gram(self, x):
        """(mean (F,) float64, s = fp32(mean), K (N, N) float64 = (x - s)(x - s)^T) of a resident fp32 matrix."""
        mean = column_mean(x)
        s = mean.float()
        return mean, s, ops.pca_rowgram(x, s)

    def _fit_resident(self, x, gram=None, consume_gram=False):
        """Fit from the resident matrix; gram=(mean, s, K) as self.gram(x) returned it is used instead of computing it (the
        k-NN graph of wide latents needs the same matrix: knn.wide_knn_graph).  The finalisation centres K in place: a
        given K is copied first unless consume_gram, one that was computed here is simply used up."""
        N, F = x.shape
        with torch.no_grad(), torch.cuda.device(x.device):
            if gram is None:
                mean, s, K = self.gram(x)
            else:
                mean, s, K = gram
                if tuple(K.shape) != (N, N) or mean.numel() != F or s.numel() != F:
                    raise ValueError(f"gram=(mean, s, K) has shapes {tuple(mean.shape)}, {tuple(s.shape)}, {tuple(K.shape)}; "
                                     f"X is ({N}, {F})")
                if not consume_gram:
                    K = K.clone()
            self._fit_gram(x, mean, s, K)

    def _fit_gram(self, x, mean, s, K):
        """The fit behind the row Gram matrix: K = (x - s)(x - s)^T is centred in place and decomposed (the caller holds the
        device and no_grad)."""
        N, F = x.shape
        attrs = finalize_samples(K.cpu() if self.eigh_device == "cpu" else K, N, F, self.n_components, self.eigensolver)
        W = attrs.pop("W").to(device=x.device, dtype=torch.float32)
        k = W.shape[0]
        V = torch.empty((k, F), dtype=torch.float64, device=x.device)
        for j in range(0, k, MAX_COMPONENTS):
            ops.pca_components(x, W[j:j + MAX_COMPONENTS].contiguous(), s, out=V[j:j + MAX_COMPONENTS])
        attrs["components_"] = orient_components(V).cpu().numpy()
        attrs["mean_"] = mean.cpu().numpy()
        self._set(attrs, x.device)

    def fit(self, X, chunk_rows=None, gram=None, consume_gram=False):
        """gram=(mean, s, K) of self.gram(x) for the resident matrix x = X: the fit equals the plain one bit for bit."""
        if chunk_rows:
            self.chunk_rows = int(chunk_rows)
        self._fit_resident(self._resident(X), gram, consume_gram)
        return self

    def fit_transform(self, X, chunk_rows=None, gram=None, consume_gram=False):
        if chunk_rows:
            self.chunk_rows = int(chunk_rows)
        x = self._resident(X)                       # uploaded once for the fit and the transform
        self._fit_resident(x, gram, consume_gram)
        return self.transform(x)

    def moments(self, X, chunk_rows=None):
        raise ValueError("WidePCA forms the N x N row Gram matrix (gram), not the F x F moments")

    # ---------------------------------------------------------------------------------------------------- applying
    def _operands(self, device):
        """Per column block of at most MAX_FEATURES features: (lo, hi, V block (k, hi - lo) contiguous fp32, shift block);
        and the float64 projection of mean - fp32(mean), removed afterwards."""
        key = str(device)
        if key not in self._dev:
            comps = np.asarray(self.components_)
            mean = np.asarray(self.mean_, dtype=np.float64)
            s = mean.astype(np.float32)
            corr = (mean - s.astype(np.float64)) @ comps.astype(np.float64, copy=False).T
            blocks = [(lo, hi, torch.as_tensor(np.ascontiguousarray(comps[:, lo:hi], dtype=np.float32)).to(device),
                       torch.as_tensor(s[lo:hi]).to(device)) for lo, hi in self._blocks(comps.shape[1])]
            self._dev[key] = (blocks, torch.as_tensor(corr).to(device) if np.any(corr != 0) else None)
        return self._dev[key]

    def transform(self, X):
        """(X - mean_) components_^T as a CUDA fp32 tensor (N, n_components_): dm_pca_transform per column block, the blocks
        added in float64 in order and rounded to fp32 once."""
        x = self._device_rows(X)
        blocks, corr = self._operands(x.device)
        with torch.no_grad(), torch.cuda.device(x.device):
            Y = torch.zeros((x.shape[0], self.n_components_), dtype=torch.float64, device=x.device)
            for lo, hi, V, s in blocks:
                for j in range(0, V.shape[0], MAX_COMPONENTS):
                    Y[:, j:j + MAX_COMPONENTS] += ops.pca_transform(x[:, lo:hi], V[j:j + MAX_COMPONENTS], s)
            if corr is not None:
                Y -= corr
            return Y.float()
