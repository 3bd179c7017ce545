"""Float64 truth for the k-means of the latents (dynamorph_amd/kmeans.py): fixture generators, a
reference Lloyd loop, the restatement of the seeding rule and the acceptance criterion of one labelling pass.

The reference loop is scikit-learn's _kmeans_single_lloyd on float64 differences of the fp32 inputs: labels = argmin of d^2
(lowest index), new centres = sum / count (rounded to fp32 every iteration unless float64 centres are asked for), empty
clusters relocated as _relocate_empty_clusters_dense does (ascending id; the rows of largest d^2 to their own old centre,
descending, ties to the lowest row; the row leaves its donor's sum and count; labels untouched), stop when the labels
repeat (strict), else when sum |c_new - c_old|^2 <= tol mean(var(X, axis=0)), else at max_iter; labels once more from the
final centres unless the stop was strict.

The criterion of a labelling pass is complete (no row exempt), in knn_reference's style, tau = 1e-6 on d^2 (the exact form's
own error is about 5 u = 3e-7):
  1. every label's float64 d^2 is <= the row minimum (1 + tau);
  2. the reported distance is within tau / 2 relative plus one fp32 ulp of the float64 one (exactly 0 where that is 0);
  3. labels equal the float64 argmin wherever the row's relative top-2 gap (d2_2 - d2_1) / d2_2 exceeds 1e-5;
  4. the rows NOT bound by 3 are at most 1 % of the case."""
import functools

import numpy as np

from dynamorph_amd.umap_layout import counter_word

TAU = 1e-6
GAP = 1e-5
MAX_UNBOUND_SHARE = 0.01


# --------------------------------------------------------------------------------------------------------- fixtures
def randn(seed, shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def blobs(seed, N, F, K, off=0., scale=1., sep=3.):
    r = np.random.default_rng(seed)
    cen = r.standard_normal((K, F)) * sep
    lab = r.integers(0, K, N)
    return (off + scale * (cen[lab] + r.standard_normal((N, F)))).astype(np.float32)


def init_rows(seed, X, K):
    return X[np.sort(np.random.default_rng(seed).choice(X.shape[0], K, replace=False))].copy()


def empty_cluster_fixture():
    """A fit whose first iteration leaves cluster 2 empty (one relocation)."""
    X = blobs(206, 400, 16, 3)
    C0 = init_rows(301, X, 4)
    C0[2] = 1000
    return X, C0


# whole-fit fixtures: name -> (X, C0)
@functools.lru_cache(maxsize=None)
def fit_fixture(name):
    if name == "blobs_1000x37":
        X = blobs(410, 1000, 37, 5, sep=.6)
        C0 = init_rows(1410, X, 5)
    elif name == "offset_600x64":
        X = blobs(433, 600, 64, 4, off=10., scale=1e-2, sep=.6)
        C0 = init_rows(1433, X, 4)
    elif name == "wide_300x4096":
        X = blobs(423, 300, 4096, 3, sep=.05)
        C0 = init_rows(1423, X, 3)
    elif name == "empty_cluster":
        X, C0 = empty_cluster_fixture()
    else:
        raise KeyError(name)
    X.setflags(write=False)
    C0.setflags(write=False)
    return X, C0


FIT_FIXTURES = ("blobs_1000x37", "offset_600x64", "wide_300x4096", "empty_cluster")


# ------------------------------------------------------------------------------------------------------------ truth
def d2_float64(X, C):
    """(N, K) float64 squared distances from float64 differences."""
    X64, C64 = np.asarray(X, np.float64), np.asarray(C, np.float64)
    N, K, F = X64.shape[0], C64.shape[0], X64.shape[1]
    out = np.empty((N, K), np.float64)
    step = max(1, (1 << 24) // max(1, K * F))
    for lo in range(0, N, step):
        diff = X64[lo:lo + step, None, :] - C64[None, :, :]
        out[lo:lo + step] = np.einsum("nkf,nkf->nk", diff, diff)
    return out


def top2_gap(d2):
    """Per row (d2_2 - d2_1) / d2_2 of the two smallest squared distances (+inf with one centre; 0 for 0 / 0)."""
    if d2.shape[1] < 2:
        return np.full(d2.shape[0], np.inf)
    s = np.partition(d2, 1, axis=1)[:, :2]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (s[:, 1] - s[:, 0]) / s[:, 1]
    return np.where(s[:, 1] == 0, 0.0, g)


def tolerance(X, tol):
    return float(tol * np.mean(np.var(np.asarray(X, np.float64), axis=0)))


def cluster_sums(X, labels, K):
    X64 = np.asarray(X, np.float64)
    sums = np.zeros((K, X64.shape[1]), np.float64)
    np.add.at(sums, labels, X64)
    return sums, np.bincount(labels, minlength=K).astype(np.int64)


def relocate(X, C_old, labels, sums, counts):
    """_relocate_empty_clusters_dense with its order fixed: ascending empty id, descending distance, ties to the lowest row."""
    empty = np.flatnonzero(counts == 0)
    if empty.size == 0:
        return 0
    X64 = np.asarray(X, np.float64)
    diff = X64 - np.asarray(C_old, np.float64)[labels]
    far = np.argsort(-np.einsum("nf,nf->n", diff, diff), kind="stable")[:empty.size]
    for k, r in zip(empty, far):
        sums[labels[r]] -= X64[r]
        counts[labels[r]] -= 1
        sums[k] = X64[r]
        counts[k] = 1
    return int(empty.size)


def lloyd(X, C0, max_iter=300, tol=1e-4, centre_dtype=np.float32):
    """The reference loop: dict(labels int32, centres, inertia, n_iter, min_gap, relocations, strict)."""
    X = np.asarray(X, np.float32)
    K = C0.shape[0]
    C = np.asarray(C0, centre_dtype).copy()
    tol_abs = tolerance(X, tol)
    old = np.full(X.shape[0], -1, np.int64)
    min_gap, relocations, strict, n_iter = np.inf, 0, False, 0
    for i in range(max_iter):
        d2 = d2_float64(X, C)
        min_gap = min(min_gap, float(top2_gap(d2).min()))
        labels = np.argmin(d2, axis=1)
        sums, counts = cluster_sums(X, labels, K)
        relocations += relocate(X, C, labels, sums, counts)
        Cn = (sums / counts[:, None]).astype(centre_dtype)
        shift2 = float(((Cn.astype(np.float64) - C.astype(np.float64)) ** 2).sum())
        C, n_iter = Cn, i + 1
        if np.array_equal(labels, old):
            strict = True
            break
        if shift2 <= tol_abs:
            break
        old = labels
    if not strict:
        d2 = d2_float64(X, C)
        min_gap = min(min_gap, float(top2_gap(d2).min()))
        labels = np.argmin(d2, axis=1)
    d2 = d2_float64(X, C)
    inertia = float(np.cumsum(d2[np.arange(X.shape[0]), labels])[-1])
    return dict(labels=labels.astype(np.int32), centres=C, inertia=inertia, n_iter=n_iter, min_gap=min_gap,
                relocations=relocations, strict=strict)


@functools.lru_cache(maxsize=None)
def fit_reference(name, max_iter=300, tol=1e-4):
    X, C0 = fit_fixture(name)
    return lloyd(X, C0, max_iter=max_iter, tol=tol)


# ---------------------------------------------------------------------------------------------------------- seeding
def exact_form_d2(X, c):
    """The exact form of every row against one centre on the CPU: differences and squares in fp32, the four squares of a
    16-byte step added in fp32 as (x^2 + y^2) + (z^2 + w^2), the steps in float64 (the device adds them in another order:
    below 1e-15 relative)."""
    X, c = np.asarray(X, np.float32), np.asarray(c, np.float32)
    F = X.shape[1]
    sq = np.zeros((X.shape[0], (F + 3) // 4 * 4), np.float32)
    diff = X - c[None, :]
    sq[:, :F] = diff * diff
    q = sq.reshape(X.shape[0], -1, 4)
    return ((q[:, :, 0] + q[:, :, 1]) + (q[:, :, 2] + q[:, :, 3])).astype(np.float64).sum(axis=1)


def seed_rows(X, K, seed, run, margin=1e-9):
    """Plain D^2 sampling, one trial per pick: u_p = (counter_word(seed, run, p, 0) >> 11) / 2^53; pick 0 is row floor(u_0 N);
    pick p is the first row whose float64 prefix sum of the running minimum exact-form d^2 exceeds u_p times the total.
    Asserts that no pick lies within margin * total of a prefix boundary (so that the order of the device's prefix sum
    cannot change it)."""
    N = X.shape[0]
    w = counter_word(seed, run, np.arange(K, dtype=np.uint64), 0)
    u = (w >> np.uint64(11)).astype(np.float64) / float(1 << 53)
    picks = [min(int(np.floor(u[0] * N)), N - 1)]
    mind2 = exact_form_d2(X, X[picks[0]])
    for p in range(1, K):
        cum = np.cumsum(mind2)
        t = u[p] * cum[-1]
        j = int(np.searchsorted(cum, t, side="right"))
        assert j < N, (p, t, cum[-1])
        near = np.abs(cum[max(j - 1, 0):j + 1] - t).min()
        assert near > margin * cum[-1], f"pick {p} of run {run}: {near} from a prefix boundary (total {cum[-1]})"
        picks.append(j)
        mind2 = np.minimum(mind2, exact_form_d2(X, X[j]))
    return np.asarray(picks, np.int64)


# -------------------------------------------------------------------------------------------------------- criterion
def failing_rows(labels, dist, X, C):
    """Rows of one labelling pass that miss the criterion: ({row: reason}, share of rows the index equality does not bind)."""
    labels, d2 = np.asarray(labels).astype(np.int64), d2_float64(X, C)
    N, K = d2.shape
    bad = {}

    def fail(rows, why):
        for r in np.flatnonzero(rows):
            bad.setdefault(int(r), why)

    assert labels.shape == (N,), labels.shape
    fail((labels < 0) | (labels >= K), "label out of range")
    lc = np.clip(labels, 0, K - 1)
    got = d2[np.arange(N), lc]
    dmin = d2.min(axis=1)
    fail(got > dmin * (1 + TAU), "1: the labelled centre is not a nearest one")
    if dist is not None:
        dist = np.asarray(dist)
        assert dist.shape == (N,) and dist.dtype == np.float32, (dist.shape, dist.dtype)
        d64 = np.sqrt(got)
        tol = TAU / 2 * d64 + np.spacing(d64.astype(np.float32)).astype(np.float64)
        fail(np.abs(dist.astype(np.float64) - d64) > tol, "2: the reported distance is off")
        fail((got == 0) & (dist != 0), "2: a zero distance is not reported as 0")
    clear = top2_gap(d2) > GAP
    fail(clear & (labels != np.argmin(d2, axis=1)), "3: the label differs from the argmin although the gap exceeds 1e-5")
    return bad, float(1.0 - clear.mean())


def assert_assign(labels, dist, X, C, what):
    bad, unbound = failing_rows(labels, dist, X, C)
    print(f"{what}: {unbound:.4%} of the rows are not bound by label equality")
    assert unbound <= MAX_UNBOUND_SHARE, f"{what}: {unbound:.3%} of the rows have a top-2 gap below 1e-5"
    assert not bad, f"{what}: {len(bad)} of {len(labels)} rows fail, e.g. {sorted(bad.items())[:5]}"
