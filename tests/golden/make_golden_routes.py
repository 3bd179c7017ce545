#!/usr/bin/env python3
"""Golden fixture for the host-side route queries: tests/golden/g14_routes.npz.

What dm_conv4x4s2 / dm_conv3x3 / dm_wgrad answer about slab counts, scratch and AFFINE2 support over the grid of
tests/helpers/route_grid.py, as the library of the commit BEFORE the kernel tables and routes were each declared once
answered it: once as shipped ("on_*") and once with the streaming and one-pass kernels switched off ("off_*").  Each table is
evaluated in a child process, because the library reads the switches once per process.  Only the values are stored.

    python3 tests/golden/make_golden_routes.py path/to/that/commit/dynamorph_amd/libdynamorph_hip.so
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HELPERS = os.path.join(os.path.dirname(HERE), "helpers")
sys.path.insert(0, HELPERS)
from route_grid import SWITCHES_OFF  # noqa: E402


def main(library):
    out = {}
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES_OFF}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, env in (("on", base), ("off", dict(base, **SWITCHES_OFF))):
            path = os.path.join(tmp, tag + ".npz")
            subprocess.check_call([sys.executable, os.path.join(HELPERS, "route_grid.py"), library, path], env=env)
            with np.load(path) as f:
                for k in f.files:
                    out[f"{tag}_{k}"] = f[k]
                    print(tag, k, f[k].shape, "distinct values:", len(np.unique(f[k])), flush=True)
    np.savez_compressed(os.path.join(HERE, "g14_routes.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
