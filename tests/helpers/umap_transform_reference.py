"""numpy restatement of DESIGN.md section 3.5d (UMAPEmbedding.transform and the transform kernels of csrc/umap.hip): the query
graph, sigma at rho = 0 with the row's own floor, memberships, the per-row schedule, the weighted-mean initialisation and one
layout epoch in which only the queries move -- in float64, and for the schedule and the epoch in float32 as well, which gives
the schedule bits and the yardstick of the position tolerance.  The generator and S are umap_reference's."""
import numpy as np

import umap_reference as UR

N_EPOCHS_T = 66
KS = (2, 15, 200, 256)


# ------------------------------------------------------------------------------------------------------------ fixture
def fixture(seed=77, M=300, R=70, F=32):
    """(X (M, F), Q (R, F), y_train (M, 2)) float32: three blobs (centres 6 randn, unit noise, label i % 3); rows 1-4 of X are
    copies of row 0; Q[0] = X[0], Q[1] = X[7], Q[3] = Q[2]; y_train uniform in [0, 10]."""
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.standard_normal((3, F))
    X = (centres[np.arange(M) % 3] + rng.standard_normal((M, F))).astype(np.float32)
    X[1:5] = X[0]
    Q = (centres[np.arange(R) % 3] + rng.standard_normal((R, F))).astype(np.float32)
    Q[0], Q[1], Q[3] = X[0], X[7], Q[2]
    y_train = (10.0 * rng.random((M, 2))).astype(np.float32)
    return X, Q, y_train


def query_knn_float64(X, Q, k):
    """(indices (R, k) int64, distances (R, k) float32) of the rows of Q against the rows of X, sorted by (distance, index):
    float64 differences of the float32 rows, rounded once.  No column is excluded."""
    X, Q = np.asarray(X, np.float64), np.asarray(Q, np.float64)
    d2 = np.zeros((Q.shape[0], X.shape[0]))
    for lo in range(0, X.shape[1], 16):
        d2 += ((Q[:, None, lo:lo + 16] - X[None, :, lo:lo + 16]) ** 2).sum(-1)
    d = np.sqrt(d2).astype(np.float32)
    order = np.lexsort((np.broadcast_to(np.arange(X.shape[0]), d.shape), d), axis=1)[:, :k]
    return order.astype(np.int64), np.take_along_axis(d, order, 1)


# ------------------------------------------------------------------------------------------------------------ T-B sigma
def S(dists, sigma):
    """S_i(sigma_i) in float64 over all k columns with rho = 0 (umap_reference.S skips a column 0, which is added here)."""
    d = np.asarray(dists, np.float64)
    return UR.S(np.concatenate([np.zeros((d.shape[0], 1)), d], 1), np.zeros(d.shape[0]), sigma)


def floors(dists):
    d = np.asarray(dists, np.float64)
    return 1e-3 * (d.sum(1) / d.shape[1])


def smooth(dists, full=False):
    """sigma float32 and per row: floored, out_of_steps; full=True: also sigma before its rounding to float32."""
    d = np.asarray(dists, np.float32)
    R, k = d.shape
    target = np.log2(float(k))
    lo, hi, mid = np.zeros(R), np.full(R, np.inf), np.ones(R)
    done = np.zeros(R, bool)
    for _ in range(64):
        s = S(d, mid)
        done |= np.abs(s - target) < 1e-5
        up = ~done & (s > target)
        dn = ~done & ~(s > target)
        hi[up] = mid[up]
        mid[up] = (lo[up] + hi[up]) * 0.5
        lo[dn] = mid[dn]
        dbl = dn & np.isinf(hi)
        mid[dbl] = mid[dbl] * 2.0
        avg = dn & ~np.isinf(hi)
        mid[avg] = (lo[avg] + hi[avg]) * 0.5
    fl = floors(d)
    floored = mid < fl
    sigma = np.where(floored, fl, mid)
    res = sigma.astype(np.float32), floored, ~done
    return res + (sigma,) if full else res


# ---------------------------------------------------------------------------------------- T-C memberships and schedule
def membership(dists, sigma):
    """The closed form in float64 from the given sigma: 1 where d <= 0 or sigma = 0, else exp(-(d / sigma))."""
    d = np.asarray(dists, np.float64)
    sg = np.asarray(sigma, np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where((d <= 0) | (sg == 0), 1.0, np.exp(-(d / np.where(sg == 0, 1.0, sg))))


def schedule(a, n_epochs, negative_sample_rate=5):
    """(pruned mask, eps, eps_neg) in float32 numpy from float32 memberships (R, k); +inf at the pruned entries."""
    a = np.asarray(a, np.float32)
    m = a.max(1, keepdims=True)
    pruned = (a == 0) | (a < m / np.float32(n_epochs))
    with np.errstate(divide="ignore"):
        eps = np.where(pruned, np.float32(np.inf), m / a).astype(np.float32)
        eps_neg = np.where(pruned, np.float32(np.inf), eps / np.float32(negative_sample_rate)).astype(np.float32)
    return pruned, eps, eps_neg


# ---------------------------------------------------------------------------------------------------- T-D initialisation
def init(indices, a, y_train):
    """y0 (R, 2) float64: the membership-weighted mean of the neighbours' training positions over all k entries (the nearest
    neighbour's position where every membership is 0)."""
    a = np.asarray(a, np.float64)
    Y = np.asarray(y_train, np.float64)[np.asarray(indices)]
    sa = a.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        y0 = (a[:, :, None] * Y).sum(1) / sa[:, None]
    return np.where(sa[:, None] > 0, y0, Y[:, 0])


def prepare(indices, dists, y_train, n_epochs=N_EPOCHS_T, negative_sample_rate=5):
    """Everything before the layout from a query graph: dict of sigma (float32), floored, out_of_steps, a (float32 rounding of
    the float64 closed form), pruned, eps, eps_neg, y0 (float64)."""
    sigma, floored, out_of_steps = smooth(dists)
    a = membership(dists, sigma).astype(np.float32)
    pruned, eps, eps_neg = schedule(a, n_epochs, negative_sample_rate)
    return dict(sigma=sigma, floored=floored, out_of_steps=out_of_steps, a=a, pruned=pruned, eps=eps, eps_neg=eps_neg,
                y0=init(indices, a, y_train))


# ------------------------------------------------------------------------------------------------------------ T-E layout
def advance(eps, eps_neg, nxt, nxt_neg, n):
    """The float32 schedule state after epoch n from the state before it (it does not depend on positions)."""
    nf = np.float32(n)
    nxt, nxt_neg = np.array(nxt, np.float32), np.array(nxt_neg, np.float32)
    f = nxt <= nf
    nxt[f] = nxt[f] + eps[f]
    n_neg = np.trunc((nf - nxt_neg[f]) / eps_neg[f]).astype(np.float32)
    nxt_neg[f] = nxt_neg[f] + n_neg * eps_neg[f]
    return nxt, nxt_neg


def state_at(eps, eps_neg, n):
    """The float32 schedule state before epoch n, from next = eps, next_neg = eps_neg."""
    nxt, nxt_neg = eps.copy(), eps_neg.copy()
    for e in range(n):
        nxt, nxt_neg = advance(eps, eps_neg, nxt, nxt_neg, e)
    return nxt, nxt_neg


def epoch(indices, eps, eps_neg, nxt, nxt_neg, y_train, y, n, n_epochs, a, b, gamma, seed, row_offset=0, dtype=np.float64):
    """One epoch of the transform from query positions y (float32) and the float32 schedule state: (y_next in dtype, next,
    next_neg, counts).  Only the queries move; the schedule arithmetic is float32 whatever dtype is.  counts: fired entries,
    pairs at distance 0, clipped components, negatives drawn."""
    T = dtype
    R, k = eps.shape
    M = len(y_train)
    Yt = np.asarray(y_train, np.float32).astype(T)
    out = np.asarray(y, np.float32).astype(T).copy()
    nxt, nxt_neg = np.array(nxt, np.float32), np.array(nxt_neg, np.float32)
    nf = np.float32(n)
    alpha = T(0.25) * (T(1) - T(n) / T(n_epochs))
    a_, b_, four = T(a), T(b), T(4)
    m2ab, g2b = T(-2) * a_ * b_, T(2) * T(gamma) * b_
    counts = {"fired": 0, "coincident": 0, "clipped": 0, "negatives": 0}

    def move(c, g, other):
        for d in range(2):
            raw = g * (c[d] - other[d])
            cl = min(max(raw, -four), four)
            counts["clipped"] += int(cl != raw)
            c[d] = c[d] + alpha * cl

    for i in range(R):
        c = [out[i, 0], out[i, 1]]
        for j in np.nonzero(nxt[i] <= nf)[0]:
            counts["fired"] += 1
            yj = Yt[indices[i, j]]
            dx, dy = c[0] - yj[0], c[1] - yj[1]
            d2 = dx * dx + dy * dy
            g = T(0)
            if d2 > 0:
                pb = d2 ** b_
                g = (m2ab * (pb / d2)) / (a_ * pb + T(1))
            else:
                counts["coincident"] += 1
            move(c, g, yj)
            nxt[i, j] = nxt[i, j] + eps[i, j]
            n_neg = int((nf - nxt_neg[i, j]) / eps_neg[i, j])
            entry = (int(row_offset) + i) * k + int(j)
            for p in range(n_neg):
                counts["negatives"] += 1
                yv = Yt[UR.R(seed, n, entry, p) % M]
                dx, dy = c[0] - yv[0], c[1] - yv[1]
                d2 = dx * dx + dy * dy
                if d2 > 0:
                    pb = d2 ** b_
                    move(c, g2b / ((T(0.001) + d2) * (a_ * pb + T(1))), yv)
                else:
                    counts["coincident"] += 1
            nxt_neg[i, j] = nxt_neg[i, j] + np.float32(n_neg) * eps_neg[i, j]
        out[i] = c
    return out, nxt, nxt_neg, counts


# ------------------------------------------------------------------------------------------------------------- quality
def label_share_against_training(Y_new, labels_new, Y_train, labels_train, n_neighbors=10):
    """The share of each new point's n_neighbors nearest TRAINING points in 2-D that carry its label."""
    Yn, Yt = np.asarray(Y_new, np.float64), np.asarray(Y_train, np.float64)
    d = ((Yn[:, None, :] - Yt[None, :, :]) ** 2).sum(-1)
    nb = np.argsort(d, axis=1, kind="stable")[:, :n_neighbors]
    return float((np.asarray(labels_train)[nb] == np.asarray(labels_new)[:, None]).mean())
