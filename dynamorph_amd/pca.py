"""Latent PCA on the GPU: a drop-in for the sklearn.decomposition.PCA(0.5) of run_dim_reduction.py (fit_PCA, lines 14-50;
process_PCA, lines 52-92).

The fit follows scikit-learn's covariance route (sklearn/decomposition/_pca.py::_fit_full) with the covariance formed on the
device: fp64 column sums (dm_pca_colsum), then the centred Gram matrix (X - s)^T (X - s) for the fp32 shift s = fp32(mean)
(dm_pca_gram), corrected in float64 for the rounding of s.  Host data are streamed in chunks through pinned staging and the
chunks merged with the pairwise (Chan) update, so the data cross PCIe once.  Finalisation -- eigendecomposition, component
count, signs -- is plain float64 torch and runs on a CPU tensor as well.  Every fitted attribute follows scikit-learn's names
and conventions, so PCA(0.5) here chooses the components and signs the reference's call chooses.
"""
import numpy as np
import torch

from . import ops

MAX_FEATURES = 16384           # DM_PCA_MAX_FEATURES
MAX_COMPONENTS = 512           # DM_PCA_MAX_COMPONENTS (one transform launch; more are done in blocks of this many)
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


def select_n_components(n_components, ratio, N, F):
    """_fit_full's rule: a fraction -> searchsorted(cumsum(ratio), frac, side='right') + 1; an int as it is (<= min(N, F));
    None -> min(N, F).  `ratio`: explained_variance_ratio_ of all components, float64 numpy."""
    _check_n_components(n_components)
    m = min(N, F)
    if n_components is None:
        return m
    if isinstance(n_components, (int, np.integer)):
        if n_components > m:
            raise ValueError(f"n_components={n_components} must be between 0 and min(n_samples, n_features)={m}")
        return int(n_components)
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


def finalize(C, mean, N, n_components=0.5):
    """From the float64 scatter matrix C = sum (x - mean)(x - mean)^T (F x F, any device) to scikit-learn's fitted attributes
    (a dict of float64 numpy arrays and ints).  eigh in float64 on C's device; eigenvalues clipped at 0; the top min(N, F)
    eigenpairs are kept (the spectrum of the full SVD _fit_full's 'full' solver computes); signs by
    svd_flip(u_based_decision=False): the entry of largest magnitude of each component is positive."""
    F = C.shape[0]
    _check_shape(N, F)
    _check_n_components(n_components)
    evals, evecs = torch.linalg.eigh(C.to(torch.float64))
    m = min(N, F)
    evals = torch.flip(evals, (0,))[:m].clamp_min(0.0)
    comps = torch.flip(evecs, (1,))[:, :m].T.contiguous()                 # (m, F): rows are components
    idx = comps.abs().argmax(dim=1)
    signs = torch.sign(comps.gather(1, idx[:, None]))
    signs[signs == 0] = 1.0
    comps *= signs
    ev = (evals / (N - 1)).cpu().numpy()
    ratio = ev / ev.sum() if ev.sum() > 0 else np.zeros_like(ev)
    k = select_n_components(n_components, ratio, N, F)
    mean = mean.to(torch.float64).cpu().numpy() if torch.is_tensor(mean) else np.asarray(mean, np.float64)
    return {
        "mean_": mean,
        "components_": comps[:k].cpu().numpy(),
        "explained_variance_": ev[:k].copy(),
        "explained_variance_ratio_": ratio[:k].copy(),
        "singular_values_": np.sqrt(ev[:k] * (N - 1)),
        "noise_variance_": float(ev[k:].mean()) if k < m else 0.0,
        "n_components_": int(k),
        "n_samples_": int(N),
        "n_features_in_": int(F),
    }


def _host_rows(X):
    """Host data as a 2-D torch tensor (a view when it can be)."""
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(X if X.dtype in (np.float32, np.float64) else X.astype(np.float32))
    elif not torch.is_tensor(X):
        X = torch.as_tensor(np.asarray(X, dtype=np.float32))
    if X.dim() != 2:
        raise ValueError(f"PCA expects a 2-D (samples, features) array, got shape {tuple(X.shape)}")
    return X


class PCA:
    """PCA(n_components=0.5, whiten=False): fit / transform / fit_transform on the GPU with scikit-learn's attributes.

    X: a CUDA tensor (used in place: fp32, unit column stride) or host data (numpy array / CPU tensor, streamed in chunks of
    `chunk_rows` rows through pinned staging).  transform returns a CUDA fp32 tensor."""

    def __init__(self, n_components=0.5, whiten=False, chunk_rows=65536, device=None, eigh_device="cuda"):
        if whiten:
            raise ValueError("PCA(whiten=True) is not supported")
        _check_n_components(n_components)
        self.n_components = n_components
        self.whiten = False
        self.chunk_rows = int(chunk_rows)
        self.device = device
        self.eigh_device = eigh_device      # 'cuda' (the fit's device) or 'cpu'
        self._dev = {}

    # ------------------------------------------------------------------------------------------------------ fitting
    def _device_of(self, X):
        if torch.is_tensor(X) and X.is_cuda:
            return X.device
        return torch.device(self.device if self.device is not None else "cuda:%d" % torch.cuda.current_device())

    def moments(self, X, chunk_rows=None):
        """(N, mean (F,) float64, C (F, F) float64 = sum (x - mean)(x - mean)^T) on the device."""
        if torch.is_tensor(X) and X.is_cuda:
            if X.dim() != 2:
                raise ValueError(f"PCA expects a 2-D (samples, features) array, got shape {tuple(X.shape)}")
            N, F = X.shape
            _check_shape(N, F)
            with torch.cuda.device(X.device):
                return (N,) + self._chunk_moments(X)
        X = _host_rows(X)
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
        dev = self._device_of(X)
        cr = max(2, min(chunk_rows, N))
        with torch.no_grad(), torch.cuda.device(dev):
            compute = torch.cuda.current_stream()
            s_in = torch.cuda.Stream()
            direct = X.dtype == torch.float32 and X.is_contiguous() and X.is_pinned()
            stage = None if direct else [torch.empty((cr, F), dtype=torch.float32, pin_memory=True) for _ in range(2)]
            x_dev = [torch.empty((cr, F), dtype=torch.float32, device=dev) for _ in range(2)]
            ev_in = [torch.cuda.Event() for _ in range(2)]       # chunk has reached x_dev[k] (staging k is free again)
            ev_done = [torch.cuda.Event() for _ in range(2)]     # kernels reading x_dev[k] are done
            ws = torch.empty(max(ops.L.load().dm_pca_gram_workspace_bytes(cr, F), 8) // 8, dtype=torch.float64, device=dev)
            C = torch.zeros((F, F), dtype=torch.float64, device=dev)
            n, mean = 0, None
            for it, lo in enumerate(range(0, N, cr)):
                k = it & 1
                m = min(cr, N - lo)
                src = X[lo:lo + m]
                if not direct:
                    ev_in[k].synchronize()
                    stage[k][:m].copy_(src)
                    src = stage[k][:m]
                with torch.cuda.stream(s_in):
                    s_in.wait_event(ev_done[k])
                    x_dev[k][:m].copy_(src, non_blocking=True)
                    ev_in[k].record(s_in)
                compute.wait_event(ev_in[k])
                mean_c, _ = self._chunk_moments(x_dev[k][:m], G=C, accumulate=True, ws=ws)
                n, mean = merge_moments(n, mean, C, m, mean_c) if mean is not None else (m, mean_c)
                ev_done[k].record(compute)
            compute.synchronize()
        return n, mean, C

    def fit(self, X, chunk_rows=None):
        N, mean, C = self.moments(X, chunk_rows)
        if self.eigh_device == "cpu":
            C = C.cpu()
        self._set(finalize(C, mean, N, self.n_components), self._device_of(X))
        return self

    def fit_transform(self, X, chunk_rows=None):
        return self.fit(X, chunk_rows).transform(X)

    # ---------------------------------------------------------------------------------------------------- applying
    def _set(self, attrs, device=None):
        for a in _ATTRS:
            setattr(self, a, attrs[a])
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

    def transform(self, X):
        """(X - mean_) components_^T as a CUDA fp32 tensor (N, n_components_)."""
        if not hasattr(self, "components_"):
            raise ValueError("this PCA instance is not fitted yet")
        if torch.is_tensor(X) and X.is_cuda:
            x = X if X.dtype == torch.float32 else X.float()
        else:
            x = _host_rows(X)
            dev = self._home if getattr(self, "_home", None) is not None else self._device_of(x)
            x = x.to(dev, dtype=torch.float32)
        if x.dim() != 2 or x.shape[1] != self.n_features_in_:
            raise ValueError(f"X has shape {tuple(x.shape)}, expected (n, {self.n_features_in_})")
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
        if attrs["n_features_in_"] > MAX_FEATURES:
            _check_shape(2, attrs["n_features_in_"])
        self._set(attrs)
        return self

    def __getstate__(self):
        st = dict(self.__dict__)
        st["_dev"] = {}
        st["_home"] = None
        return st
