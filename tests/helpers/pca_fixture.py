"""Planted-spectrum latents of tests/golden/g13_pca.npz, rebuilt exactly from the stored recipe.

X[n][f] = offset + sum_j u[n][j] * s[j] * r[j][f] * 2^-10 + e[n][f] * 2^-10 with small integers u, s, r (+-1), e: every entry
is a multiple of 2^-10 below 2^14, so the float64 matrix is exact and its float32 cast is the same numbers."""
import hashlib

import numpy as np


def recipe(N, F, seed, n_planted=40):
    s = np.array([96 - 2 * j for j in range(n_planted)], np.int64)       # 96 .. 18: eigenvalues ~ s^2, adjacent ratios >= 1.2
    u_var = (33 ** 2 - 1) / 12.0                                       # u uniform on -16 .. 16
    e_var = (65 ** 2 - 1) / 12.0                                       # e uniform on -32 .. 32
    sigma = np.sqrt((u_var * float((s ** 2).sum()) + e_var) * 2.0 ** -20)
    offset = np.round(30.0 * sigma * 1024.0) / 1024.0                  # the common offset: 30 sigma, a multiple of 2^-10
    return {"N": N, "F": F, "seed": seed, "s": s, "offset": offset}


def make_x(rec):
    N, F = int(rec["N"]), int(rec["F"])
    rng = np.random.default_rng(int(rec["seed"]))
    s = np.asarray(rec["s"], np.int64)
    u = rng.integers(-16, 17, size=(N, len(s)))
    r = rng.integers(0, 2, size=(len(s), F)) * 2 - 1
    e = rng.integers(-32, 33, size=(N, F))
    X = ((u * s) @ r + e).astype(np.float64) * 2.0 ** -10 + float(rec["offset"])
    assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
    return X


def checksum(X):
    return hashlib.sha256(np.ascontiguousarray(X, np.float64).tobytes()).hexdigest()
