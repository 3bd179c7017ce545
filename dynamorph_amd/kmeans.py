"""Exact Lloyd k-means of the latents on the GPU: what sklearn.cluster.KMeans(n_clusters=n) computes in the reference's
clustering scripts (HiddenStateExtractor/deprecated/morphology_clustering.py:103-141 generate_short_traj_morphorlogy,
Kmean_on_short_trajs, Kmean_on_short_traj_diffs; movement_clustering.py:103) on PCA-ed latent vectors and on short windows of
trajectories built from them.  DESIGN.md section 3.5g.

The kernels (csrc/kmeans.hip) label the rows, add them up by cluster and measure a row against its centre; this module keeps X
resident (knn._resident's rules), runs scikit-learn's loop (_kmeans_single_lloyd: labels, centres, the strict / tolerance /
max_iter stops, the extra labelling pass, the relocation of empty clusters) with one small read-back per iteration, seeds the
runs (a given array, or plain D^2 sampling from the counter-based generator of umap_layout) and keeps the run of lowest
inertia.  The distance is the k-NN graph's exact form, the label the centre of smallest (fp32 distance, index): labels and
centres depend on the inputs only."""
import numpy as np
import torch

from . import knn as _knn
from . import ops
from .rows import chunk_size, device_chunks, device_of, shape_of
from .umap_layout import counter_word

MAX_FEATURES = _knn.MAX_FEATURES
MAX_CLUSTERS = ops.KMEANS_MAX_CLUSTERS
DEFAULT_CHUNK_ROWS = 65536
_VAR_CHUNK_ROWS = 8192


def _check_shape(shape, K=None):
    """The limits, from the shape alone: before anything moves to the device."""
    if len(shape) != 2:
        raise ValueError(f"KMeans expects a 2-D (samples, features) array, got shape {tuple(shape)}")
    N, F = shape
    if F < 1 or F > MAX_FEATURES:
        raise ValueError(f"KMeans on the GPU supports 1 .. {MAX_FEATURES} features, got {F}: reduce wider latents with the PCA "
                         f"first (fit_PCA / process_PCA), which is also what the reference clusters")
    if N < 1:
        raise ValueError("X has no rows")
    if K is not None and K > N:
        raise ValueError(f"n_clusters = {K} exceeds the {N} rows of X")
    return N, F


def seed_uniforms(seed, run, n):
    """u_0 .. u_{n-1} in [0, 1): the top 53 bits of counter_word(seed, run, pick, 0) over 2^53 (float64, exact)."""
    w = counter_word(seed, run, np.arange(n, dtype=np.uint64), 0)
    return (w >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def column_variance_mean(x):
    """mean over the columns of var(X, axis=0), in float64 from fp64 column sums and sums of squares: scikit-learn's scale
    of `tol`.  0-dim float64 on x's device."""
    N = x.shape[0]
    s = ops.pca_colsum(x)
    s2 = torch.zeros_like(s)
    for lo in range(0, N, _VAR_CHUNK_ROWS):
        s2 += x[lo:lo + _VAR_CHUNK_ROWS].double().square_().sum(0)
    mean = s / N
    return (s2 / N - mean * mean).clamp_(min=0).mean()


class KMeans:
    """sklearn.cluster.KMeans(n_clusters, n_init=10, max_iter=300, tol=1e-4, algorithm='lloyd') on the device.

    init: a (K, F) array, used as it is (one run, as scikit-learn does), or 'k-means++' -- plain D^2 sampling, one trial per
    pick (NOT scikit-learn's greedy variant): run r draws u_p from seed_uniforms(seed, r, K); pick 0 is row floor(u_0 N), pick
    p the first row whose float64 prefix sum of the running minimum exact-form d^2 exceeds u_p times the total.  n_init runs;
    the lowest inertia_ wins, ties to the lowest run.  After fit: cluster_centers_ (K, F) float32, labels_ int32, inertia_,
    n_iter_, n_features_in_, rechecked_ (rows the labelling pass redid exactly over the winning run) -- numpy on the host."""

    def __init__(self, n_clusters, init='k-means++', n_init=10, max_iter=300, tol=1e-4, seed=0, device=None):
        K = int(n_clusters)
        if K < 1 or K > MAX_CLUSTERS:
            raise ValueError(f"n_clusters = {n_clusters} is outside 1 .. {MAX_CLUSTERS}")
        if isinstance(init, str):
            if init != 'k-means++':
                raise ValueError(f"init={init!r}: 'k-means++' or a (n_clusters, n_features) array")
        else:
            init = np.array(init.detach().cpu() if torch.is_tensor(init) else init, dtype=np.float32)
            if init.ndim != 2 or init.shape[0] != K:
                raise ValueError(f"init has shape {init.shape}, expected ({K}, n_features)")
        if int(n_init) < 1 or int(max_iter) < 1 or not float(tol) >= 0:
            raise ValueError("n_init and max_iter must be >= 1 and tol >= 0")
        self.n_clusters, self.init, self.n_init, self.max_iter = K, init, int(n_init), int(max_iter)
        self.tol, self.seed, self.device = float(tol), int(seed), device
        self._shift = None

    # ------------------------------------------------------------------------------------------------------- fit
    def _seed_rows(self, x, run):
        """The K rows of run `run` by D^2 sampling, (K,) int64 on the device; no read-back."""
        N, K = x.shape[0], self.n_clusters
        u = seed_uniforms(self.seed, run, K)
        first = min(int(np.floor(u[0] * N)), N - 1)
        picks = [torch.tensor(first, device=x.device, dtype=torch.int64)]
        ud = torch.from_numpy(u).to(x.device)
        mind2 = ops.kmeans_row_d2(x, x[first:first + 1])
        for p in range(1, K):
            cum = torch.cumsum(mind2, 0)
            j = torch.searchsorted(cum, (ud[p] * cum[-1]).reshape(1), right=True).clamp_(max=N - 1)[0]
            picks.append(j)
            if p + 1 < K:
                mind2 = torch.minimum(mind2, ops.kmeans_row_d2(x, x[j].reshape(1, -1)))
        return torch.stack(picks)

    @staticmethod
    def _relocate(x, C_old, labels, sums, counts):
        """sklearn's _relocate_empty_clusters_dense on the kernel's sums and counts: the empty clusters, in ascending id, take
        the rows of largest exact-form distance to their own (old) centre, in descending order, ties to the lowest row; each
        such row leaves its donor's sum and count.  Labels are not touched."""
        empty = torch.nonzero(counts == 0).flatten()
        d2 = ops.kmeans_row_d2(x, C_old, labels)
        far = torch.sort(d2, descending=True, stable=True).indices[:empty.numel()]
        one = torch.ones(1, dtype=counts.dtype, device=counts.device)
        for j in range(empty.numel()):
            r = far[j:j + 1]
            donor = labels[r].long()
            xr = x[r].double()
            sums.index_add_(0, donor, -xr)
            counts.index_add_(0, donor, -one)
            sums[empty[j]] = xr[0]
            counts[empty[j]] = 1

    def _lloyd(self, x, C, shift, ws, tol_abs):
        """One run from the centres C (K, F) fp32: (labels int32, centres fp32, n_iter, rechecked rows) on the device."""
        N, K = x.shape[0], self.n_clusters
        bufs = [torch.full((N,), -1, dtype=torch.int32, device=x.device), torch.empty(N, dtype=torch.int32, device=x.device)]
        sums = counts = None
        rechecked = torch.zeros(1, dtype=torch.int64, device=x.device)
        strict, n_iter = False, 0
        for i in range(self.max_iter):
            old, labels = bufs[i & 1], bufs[(i + 1) & 1]
            _, _, n = ops.kmeans_assign(x, C, shift, labels=labels, want_dist=False, workspace=ws)
            rechecked += n
            sums, counts = ops.kmeans_sums(x, labels, K, sums, counts, workspace=ws)

            def update():
                Cn = (sums / counts.double()[:, None]).float()
                return Cn, (Cn.double() - C.double()).square_().sum()
            Cn, sh2 = update()
            flags = torch.stack([(labels != old).any().double(), (counts == 0).any().double(), sh2]).cpu()
            if flags[1]:
                self._relocate(x, C, labels, sums, counts)
                Cn, sh2 = update()
                flags[2] = sh2.cpu()
            C, n_iter = Cn, i + 1
            if not flags[0]:
                strict = True
                break
            if float(flags[2]) <= tol_abs:
                break
        labels = bufs[n_iter & 1]
        if not strict:
            _, _, n = ops.kmeans_assign(x, C, shift, labels=labels, want_dist=False, workspace=ws)
            rechecked += n
        return labels, C, n_iter, rechecked

    def fit(self, X):
        K = self.n_clusters
        N, F = _check_shape(shape_of(X), K)
        given = not isinstance(self.init, str)
        if given and self.init.shape[1] != F:
            raise ValueError(f"init has shape {self.init.shape}, expected ({K}, {F})")
        x = _knn._resident(X, self.device)
        with torch.no_grad(), torch.cuda.device(x.device):
            shift = _knn.column_shift(x)
            ws = ops.kmeans_workspace(N, F, K, x)
            tol_abs = float(self.tol * column_variance_mean(x).item())
            best = None
            for run in range(1 if given else self.n_init):
                if given:
                    C0 = torch.from_numpy(np.ascontiguousarray(self.init)).to(x.device)
                else:
                    C0 = x[self._seed_rows(x, run)].contiguous()
                labels, C, n_iter, rechecked = self._lloyd(x, C0, shift, ws, tol_abs)
                d2 = ops.kmeans_row_d2(x, C, labels).cpu().numpy()
                inertia = float(np.cumsum(d2)[-1])              # float64, in row order
                if best is None or inertia < best[0]:
                    best = (inertia, labels.clone(), C, n_iter, int(rechecked.item()))
            self.inertia_, labels, C, self.n_iter_, self.rechecked_ = best
            self.labels_ = labels.cpu().numpy()
            self.cluster_centers_ = C.cpu().numpy()
            self.n_features_in_ = F
            self._shift = shift.cpu().numpy()
        return self

    def fit_predict(self, X):
        return self.fit(X).labels_

    # --------------------------------------------------------------------------------------------------- predict
    def _fitted(self):
        if not hasattr(self, "cluster_centers_"):
            raise ValueError("this KMeans is not fitted")

    def predict(self, X, chunk_rows=DEFAULT_CHUNK_ROWS, shift="fit", return_rechecked=False):
        """labels int32 (numpy) of the rows of X against cluster_centers_.  X on the device is used in place; host X is
        streamed in chunks of chunk_rows rows through pinned staging, the next chunk's copy overlapping the current chunk's
        kernels, like knn_query.  shift: "fit" (the training column mean), None or an (F,) fp32 device tensor -- the labels do
        not depend on it."""
        self._fitted()
        F, K = self.n_features_in_, self.n_clusters
        N, Fx = _check_shape(shape_of(X))
        if Fx != F:
            raise ValueError(f"X has shape {(N, Fx)}, expected (n, {F})")
        dev = device_of(X, self.device)
        cr = chunk_size(chunk_rows, N)
        with torch.no_grad(), torch.cuda.device(dev):
            C = torch.from_numpy(np.ascontiguousarray(self.cluster_centers_, dtype=np.float32)).to(dev)
            if isinstance(shift, str):
                s = None if self._shift is None else torch.from_numpy(self._shift).to(dev)
            else:
                s = shift
            ws = ops.kmeans_workspace(cr, F, K, C)
            labels = torch.empty(N, dtype=torch.int32, device=dev)
            counts = []
            for lo, x in device_chunks(X, cr, dev):
                counts.append(ops.kmeans_assign(x, C, s, labels=labels[lo:lo + x.shape[0]], want_dist=False, workspace=ws)[2])
            out = labels.cpu().numpy()
            return (out, int(torch.cat(counts).sum().item())) if return_rechecked else out

    # ------------------------------------------------------------------------------------------- scikit-learn interchange
    def to_sklearn(self):
        """A fitted sklearn.cluster.KMeans(n_clusters, n_init, max_iter, tol, algorithm='lloyd') with cluster_centers_,
        labels_, inertia_, n_iter_, n_features_in_ and the two private attributes its predict needs."""
        self._fitted()
        try:
            from sklearn.cluster import KMeans as SkKMeans
        except ImportError as e:
            raise ImportError("to_sklearn needs scikit-learn, which is not importable here") from e
        sk = SkKMeans(n_clusters=self.n_clusters, n_init=self.n_init, max_iter=self.max_iter, tol=self.tol, algorithm='lloyd')
        sk.cluster_centers_ = np.array(self.cluster_centers_, dtype=np.float32)
        sk.labels_ = np.array(self.labels_, dtype=np.int32)
        sk.inertia_ = float(self.inertia_)
        sk.n_iter_ = int(self.n_iter_)
        sk.n_features_in_ = int(self.n_features_in_)
        sk._n_features_out = int(self.n_clusters)
        sk._n_threads = 1
        return sk

    @classmethod
    def from_sklearn(cls, obj, device=None):
        """Apply a fitted sklearn KMeans (e.g. a clustering the reference pickled) on the GPU."""
        C = np.ascontiguousarray(obj.cluster_centers_, dtype=np.float32)
        _check_shape((max(C.shape[0], 1), C.shape[1]) if C.ndim == 2 else C.shape)
        n_init = obj.n_init if isinstance(obj.n_init, int) else 1
        self = cls(C.shape[0], init='k-means++', n_init=n_init, max_iter=obj.max_iter, tol=obj.tol, device=device)
        self.cluster_centers_ = C
        self.labels_ = np.asarray(getattr(obj, "labels_", np.zeros(0)), dtype=np.int32)
        self.inertia_ = float(getattr(obj, "inertia_", np.nan))
        self.n_iter_ = int(getattr(obj, "n_iter_", 0))
        self.n_features_in_ = int(C.shape[1])
        self.rechecked_ = 0
        self._shift = C.mean(0, dtype=np.float64).astype(np.float32)
        return self
