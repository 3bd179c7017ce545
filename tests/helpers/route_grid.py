"""The host-side route queries of dm_conv4x4s2, dm_conv3x3 and dm_wgrad over one fixed grid of shapes.

These six functions tell a caller how many slabs to allocate, how much scratch to attach and whether T may be AFFINE2; the
launch of the same entry point picks its kernel and grid from the same decision, so a value that moves means a shape changed
kernels or slab counts.  tables(lib) evaluates all of them; tests/golden/make_golden_routes.py recorded the result once
(tests/golden/g14_routes.npz) and tests/test_routes_host.py compares the built library against it.

The streaming / one-pass switches (DM_WIDE_STREAM, DM_WIDE_WGRAD1) are read once per process, so the grid with them off is
evaluated in a child:   python3 tests/helpers/route_grid.py LIBRARY OUT.npz
"""
import ctypes as C
import itertools
import sys

import numpy as np

BATCHES = (1, 3, 2048)
# every channel count of a row of the register-resident kernel tables (conv_mfma.hip, wgrad_mfma.hip), then counts without
# one: 6, 7, 12, 64, 128
CHANNELS = (1, 2, 3, 4, 5, 8, 16, 32, 6, 7, 12, 64, 128)
_EDGES = (8, 16, 32, 64, 128, 256)
SIZES = tuple(itertools.product(_EDGES, _EDGES)) + ((8, 48), (16, 24))
TAPS = (1, 9)
KS = (1, 3, 4)
SWITCHES_OFF = {"DM_WIDE_STREAM": "0", "DM_WIDE_WGRAD1": "0"}

_SIGNATURES = {
    "dm_conv4x4s2_num_blocks": (C.c_int, 6),
    "dm_conv4x4s2_scratch_floats": (C.c_int64, 5),
    "dm_conv3x3_num_blocks": (C.c_int, 8),
    "dm_conv3x3_scratch_floats": (C.c_int64, 7),
    "dm_wgrad_num_blocks": (C.c_int, 6),
    "dm_wgrad_t_affine2_supported": (C.c_int, 5),
}


def bind(path):
    """The six queries of the library at `path`, with their signatures (host-only calls: no device is touched)."""
    lib = C.CDLL(path)
    for name, (res, nargs) in _SIGNATURES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, [C.c_int] * nargs
    return lib


def _table(f, dtype, *axes):
    """f over the product of the axes (a (H, W) pair counts as one axis and is passed as two arguments), C order."""
    out = np.empty([len(a) for a in axes], dtype)
    flat = out.reshape(-1)
    for i, combo in enumerate(itertools.product(*axes)):
        args = []
        for v in combo:
            args += v if isinstance(v, tuple) else (v,)
        flat[i] = f(*args)
    return out


def tables(lib):
    ch, sz, two = CHANNELS, SIZES, (0, 1)
    return {
        # (B, CIN, NOUT, (H, W), per_tile)
        "conv4_num_blocks": _table(lib.dm_conv4x4s2_num_blocks, np.int32, BATCHES, ch, ch, sz, two),
        # (CIN, NOUT, (H, W), fallback)
        "conv4_scratch_floats": _table(lib.dm_conv4x4s2_scratch_floats, np.int64, ch, ch, sz, two),
        # (B, CIN, NOUT, (H, W), taps, pixel_shuffle, per_tile)
        "conv3_num_blocks": _table(lib.dm_conv3x3_num_blocks, np.int32, BATCHES, ch, ch, sz, TAPS, two, two),
        # (CIN, NOUT, (H, W), taps, pixel_shuffle, per_tile)
        "conv3_scratch_floats": _table(lib.dm_conv3x3_scratch_floats, np.int64, ch, ch, sz, TAPS, two, two),
        # (B, CS, CT, (Hs, Ws), k)
        "wgrad_num_blocks": _table(lib.dm_wgrad_num_blocks, np.int32, BATCHES, ch, ch, sz, KS),
        # (CS, CT, (Hs, Ws), k)
        "wgrad_t_affine2": _table(lib.dm_wgrad_t_affine2_supported, np.int8, ch, ch, sz, KS),
    }


if __name__ == "__main__":
    np.savez_compressed(sys.argv[2], **tables(bind(sys.argv[1])))
