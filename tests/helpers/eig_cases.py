"""Shared by tests/test_eig_host.py and tests/test_gpu_eig.py: the shapes of dm_eig_apply, the planted spectra of the
partial eigensolver and the gates its results are held to.

The gates are derived, not measured (n the order, lambda / u the pairs of numpy.linalg.eigh of the same matrix):
    |theta_j - lambda_j| <= residual_j + 4 n 2^-53 lambda_1     the residual bound of a symmetric matrix + eigh's own error
    sin angle(v_j, u_j)  <= 2 residual_j / gap_j + n 2^-50      Davis-Kahan for a pair separated by gap_j from the others
    ||V^T V - I||_max    <= n 2^-50
    residual_j           <= tol theta_1
"""
import numpy as np

# n: one below / at / above the row tile (64), the two stage lengths (16 for b > 64, 32 below), the shortest split range (256)
# and a whole number of ranges (512); 1030 = 5 ranges of 224 with a ragged tail; b: one, three and sixteen column tiles.
APPLY_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 512, 1030)
APPLY_B = (16, 48, 256)
TOL = 1e-10


def planted(lam, seed=1):
    """A = U diag(lam) U^T, symmetrised, with U the Q factor of a seeded normal matrix."""
    n = len(lam)
    U = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))[0]
    A = (U * np.asarray(lam, np.float64)) @ U.T
    return (A + A.T) * 0.5


def spectrum(name, n=600):
    """(lam, arguments of top_eigenpairs, expected k or None)."""
    j = np.arange(1, n + 1, dtype=np.float64)
    if name == "a":
        return 0.9 ** j, {"k": 20}, 20
    if name == "b":
        return 1.0 / j, {"fraction": 0.5}, 18
    if name == "c":
        lam = 0.9 ** j
        lam[9] = lam[8] * (1.0 - 1e-9)
        return lam, {"k": 12}, 12
    if name == "d":
        return j ** -0.5, {"fraction": 0.5}, 159
    if name == "e":
        return 1.0 + 1e-3 * j / n, {"fraction": 0.5}, None
    raise KeyError(name)


def _sin(V, U):
    """The sine of the largest principal angle between span(V) and span(U) (orthonormal columns), as a norm -- not from
    the cosine, which cannot resolve small angles."""
    R = V - U @ (U.T @ V)
    return float(np.linalg.norm(R, 2))


def check_pairs(A, theta, V, info, groups=(), tol=TOL, angles=True):
    """The gates above for the result of top_eigenpairs on the numpy matrix A.  groups: tuples of 0-based indices whose
    eigenvalues are too close to tell apart: their subspace is compared as one, against the gap of the whole group.
    angles=False: without the angle gate -- for a block of n columns, where the residuals are a few units of rounding and what
    the gate would measure is the error of the two eigh's themselves."""
    n = A.shape[0]
    w, U = np.linalg.eigh(A)
    w, U = w[::-1], U[:, ::-1]
    theta, V, res = np.asarray(theta), np.asarray(V), np.asarray(info["residual"])
    k = theta.shape[0]
    assert V.shape == (n, k) and res.shape == (k,)
    assert np.all(np.diff(theta) <= 0)
    assert np.abs(V.T @ V - np.eye(k)).max() <= n * 2.0 ** -50
    assert np.all(res <= tol * theta[0]), (res.max(), tol * theta[0])
    assert np.all(np.abs(theta - w[:k]) <= res + 4 * n * 2.0 ** -53 * w[0]), np.abs(theta - w[:k]).max()
    true_res = np.linalg.norm(A @ V - V * theta, axis=0)
    assert np.all(np.abs(true_res - res) <= 8 * n * 2.0 ** -53 * w[0]), np.abs(true_res - res).max()
    if not angles:
        return
    grouped = {i for g in groups for i in g}
    sets = [tuple(g) for g in groups] + [(i,) for i in range(k) if i not in grouped]
    for g in sets:
        others = np.delete(w, list(g))
        gap = min(np.abs(others - w[i]).min() for i in g)
        bound = 2 * res[list(g)].max() / gap + n * 2.0 ** -50
        s = _sin(V[:, list(g)], U[:, list(g)])
        assert s <= bound, (g, s, bound)
