"""The leading eigenpairs of a symmetric float64 matrix by block subspace iteration with a Rayleigh-Ritz step: the partial
eigensolver behind pca.finalize / pca.finalize_samples (eigensolver="partial").

The heavy step, Y = A Q (O(n^2 b)), is dm_eig_apply on the device (ops.eig_apply); the block products (O(n b^2)), the
Householder QR of the block and the b x b eigh of the Rayleigh-Ritz step are float64 torch operations on A's device.  A CPU
tensor takes A @ Q, so the whole driver runs without a GPU.  One small read-back per step: the Ritz values and residuals.

What the result certifies: every returned pair has |theta - lambda| <= residual for SOME eigenvalue lambda of A (the residual
bound of a symmetric matrix).  It does not certify that no larger eigenvalue was missed -- no iterative solver proves that; a
start block orthogonal to an eigenvector would never find it.  The start block is a fixed pseudo-random one, `guard` extra
columns converge ahead of the wanted ones, and the callers compare against the full decomposition in the tests.
"""
import numpy as np
import torch

from . import ops
from .umap_layout import counter_word

APPLIES_PER_STEP = 2            # applications of A between two Rayleigh-Ritz steps (the last one feeds the step)


class NotApplicable(ValueError):
    """The wanted pairs and the guard do not fit a block of max_block columns."""


class NotConverged(RuntimeError):
    """max_applies applications did not bring the wanted pairs under the tolerance."""


def start_block(n, cols, seed=0, first=0):
    """Columns first .. first + cols - 1 of the start block, (n, cols) float64 numpy: entry (row i, column j) is
    (counter_word(seed, j, i, 0) >> 11) / 2^52 - 1, in [-1, 1).  Not orthonormalised."""
    i = np.arange(n, dtype=np.uint64)[:, None]
    out = np.empty((n, cols), dtype=np.float64)
    for c in range(cols):
        w = counter_word(seed, first + c, i, 0)
        out[:, c:c + 1] = (w >> np.uint64(11)).astype(np.float64) / float(2 ** 52) - 1.0
    return out


def _orth(Y):
    """An orthonormal basis of the columns of Y (Householder QR: rank-deficient blocks are completed, not refused)."""
    return torch.linalg.qr(Y, mode="reduced")[0]


def _round_block(b, n, max_block):
    """The block the kernel takes: a multiple of 16, at most max_block; n itself when the matrix is not larger."""
    b = min(int(b), int(max_block))
    if b >= n:
        return n
    return min((b + 15) // 16 * 16, int(max_block))


def _default_apply(A, ws):
    if not A.is_cuda:
        return lambda Q: A @ Q

    def apply(Q):
        b = Q.shape[1]
        if b % 16 or b > ops.EIG_MAX_BLOCK:       # b == n of a small matrix: columns of zeros up to the next multiple
            bp = (b + 15) // 16 * 16
            if bp > ops.EIG_MAX_BLOCK:
                raise NotApplicable(f"a block of {b} columns exceeds the kernel's {ops.EIG_MAX_BLOCK}")
            Qp = torch.zeros((Q.shape[0], bp), dtype=torch.float64, device=Q.device)
            Qp[:, :b] = Q
            return ops.eig_apply(A, Qp, workspace=ws.get(A.shape[0], bp, A))[:, :b]
        return ops.eig_apply(A, Q if Q.stride(1) == 1 else Q.contiguous(), workspace=ws.get(A.shape[0], b, A))
    return apply


class _Workspaces:
    def __init__(self):
        self._ws = {}

    def get(self, n, b, like):
        if b not in self._ws:
            self._ws[b] = ops.eig_workspace(n, b, like)
        return self._ws[b]


def top_eigenpairs(A, k=None, fraction=None, trace=None, block=32, guard=16, max_block=256, tol=1e-10, max_applies=400, seed=0,
                   apply=None):
    """(theta (k,) float64 descending, V (n, k) float64 with orthonormal columns, info) of the symmetric float64 matrix A
    (n x n, any device).  Exactly one of k (int) and fraction (in (0, 1)) is given; a fraction asks for
    searchsorted(cumsum(theta) / trace, fraction, side="right") + 1 pairs -- pca.select_n_components' rule; trace defaults
    to the float64 sum of A's diagonal.  Ritz values never exceed the eigenvalues they approximate, so the count taken
    from unconverged values is never too small.

    The block starts at `block` columns and doubles (to at most min(max_block, n)) while the wanted count + guard exceeds
    it; NotApplicable when they exceed max_block < n.  A block of n columns makes the Rayleigh-Ritz step the exact
    decomposition.  Returns when every wanted pair has ||A v - theta v||_2 <= tol theta_1; NotConverged after max_applies
    applications.  apply(Q) -> A Q defaults to ops.eig_apply (A @ Q for a CPU tensor).
    info: block, applies, steps, residual (numpy, one per returned pair)."""
    if not torch.is_tensor(A) or A.dim() != 2 or A.shape[0] != A.shape[1] or A.dtype != torch.float64:
        raise ValueError("top_eigenpairs: A must be a square float64 tensor")
    if (k is None) == (fraction is None):
        raise ValueError("top_eigenpairs: give exactly one of k and fraction")
    n = A.shape[0]
    if k is not None:
        k = int(k)
        if k < 1 or k > n:
            raise ValueError(f"top_eigenpairs: k = {k} is outside 1 .. {n}")
    elif not 0.0 < float(fraction) < 1.0:
        raise ValueError(f"top_eigenpairs: fraction = {fraction} must lie in (0, 1)")
    guard, max_block = int(guard), int(max_block)
    if block < 1 or guard < 0 or max_block < block:
        raise ValueError(f"top_eigenpairs: block = {block}, guard = {guard}, max_block = {max_block}")
    dev = A.device
    if apply is None:
        apply = _default_apply(A, _Workspaces())
    if trace is None:
        trace = float(torch.diagonal(A).sum(dtype=torch.float64))
    trace = float(trace)
    if not np.isfinite(trace):
        raise ValueError("top_eigenpairs: the trace of A is not finite")
    if k is not None and k + guard > max_block and max_block < n:
        raise NotApplicable(f"k + guard = {k + guard} exceeds max_block = {max_block}")

    b = _round_block(block, n, max_block)
    Q = _orth(torch.from_numpy(start_block(n, b, seed)).to(dev))
    applies = steps = 0
    while True:
        if applies + APPLIES_PER_STEP > max_applies:
            raise NotConverged(f"top_eigenpairs: {applies} applications of the {n} x {n} matrix at block {b} left residuals "
                               f"above {tol:g} theta_1")
        for _ in range(APPLIES_PER_STEP - 1):
            Q = _orth(apply(Q))
        Y = apply(Q)
        applies += APPLIES_PER_STEP
        steps += 1
        H = Q.T @ Y
        H = (H + H.T) * 0.5
        evals, S = torch.linalg.eigh(H)
        evals, S = torch.flip(evals, (0,)), torch.flip(S, (1,))
        X, AX = Q @ S, Y @ S
        res = torch.linalg.vector_norm(AX - X * evals, dim=0)
        back = torch.stack((evals, res)).cpu().numpy()          # the step's one read-back
        theta, resid = back[0], back[1]
        if not np.all(np.isfinite(theta)) or not np.all(np.isfinite(resid)):
            raise ValueError("top_eigenpairs: the Ritz values are not finite")
        if k is not None:
            need = k
        else:
            need = int(np.searchsorted(np.cumsum(theta) / trace, float(fraction), side="right") + 1)
        if b == n:
            need = min(need, n)
        if need + guard > b and b < n:
            if b >= max_block:
                raise NotApplicable(f"{need} pairs + guard {guard} exceed max_block = {max_block}")
            nb = _round_block(2 * b, n, max_block)
            new = torch.from_numpy(start_block(n, nb - b, seed, first=b)).to(dev)
            Q = _orth(torch.cat((AX, new), dim=1))
            b = nb
            continue
        if np.all(resid[:need] <= tol * theta[0]):
            info = {"block": int(b), "applies": int(applies), "steps": int(steps), "residual": resid[:need].copy()}
            return torch.from_numpy(theta[:need].copy()).to(dev), X[:, :need].contiguous(), info
        Q = _orth(AX)
