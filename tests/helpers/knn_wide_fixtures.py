"""Fixtures for the k-nearest-neighbour graph of wide latents (more than 16384 features; knn.wide_knn_graph).

Plain randn is useless at this width: distances concentrate, and the float64 reference's own gaps fall under the 1e-5 that
index equality needs (clear_share of randn(130, 65536) is 0.53 at k = 15 and 0.0 at k = 100).  The fixtures are planted rows:
a rank-r signal plus a little noise, so that neighbours are separated by the signal."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_reference as KR  # noqa: E402

# name -> (seed, N, F, offset)
WIDE = {
    "201_130x16385": (201, 130, 16385, 0),
    "202_130x65536": (202, 130, 65536, 0),
    "203_130x65536_offset30": (203, 130, 65536, 30),
}


def planted(seed, N, F, r=8, noise=0.05, offset=0):
    """offset + a b + noise e: a (N, r), b (r, F), e (N, F) standard normal, drawn in that order; every array fp32."""
    g = np.random.default_rng(seed)
    a = g.standard_normal((N, r)).astype(np.float32)
    b = g.standard_normal((r, F)).astype(np.float32)
    e = g.standard_normal((N, F)).astype(np.float32)
    X = (np.float32(offset) + a @ b + np.float32(noise) * e).astype(np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """(X, float64 d^2 with the self pairs at +inf): the truth takes seconds at this width and is computed once."""
    seed, N, F, offset = WIDE[name]
    X = planted(seed, N, F, offset=offset)
    d2 = KR.d2_float64(X, X, self_r0=0)
    d2.setflags(write=False)
    return X, d2
