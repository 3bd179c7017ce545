"""`not gpu`: the route queries of dm_conv4x4s2, dm_conv3x3 and dm_wgrad answer what they answered before each kernel table
and each route was declared once (tests/golden/g14_routes.npz, recorded from that earlier library by
tests/golden/make_golden_routes.py over the grid of tests/helpers/route_grid.py).  The launches read the same route, so a
dropped or mistyped table row shows here as scratch floats going from 0 to a positive value or as another slab count."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

HELPERS = os.path.join(ROOT, "tests", "helpers")
sys.path.insert(0, HELPERS)
import route_grid as RG  # noqa: E402


@pytest.fixture(scope="module")
def library():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    return _lib.LIB_PATH


@pytest.fixture(scope="module")
def recorded():
    return load_golden("g14_routes.npz")


def _same(got, recorded, tag):
    assert sorted(got) == sorted(k[len(tag) + 1:] for k in recorded if k.startswith(tag + "_"))
    for name, table in got.items():
        want = recorded[f"{tag}_{name}"]
        assert table.shape == want.shape and table.dtype == want.dtype, name
        bad = np.argwhere(table != want)
        assert len(bad) == 0, f"{name} ({tag}): {len(bad)} grid points moved, first at index {bad[0].tolist()}: " \
                              f"{table[tuple(bad[0])]} (recorded {want[tuple(bad[0])]})"


def test_routes_as_shipped(library, recorded):
    assert not any(k in os.environ for k in RG.SWITCHES_OFF), "this test needs the library's default switches"
    _same(RG.tables(RG.bind(library)), recorded, "on")


def test_routes_with_streaming_and_one_pass_kernels_off(library, recorded, tmp_path):
    out = str(tmp_path / "off.npz")
    subprocess.check_call([sys.executable, os.path.join(HELPERS, "route_grid.py"), library, out],
                          env=dict(os.environ, **RG.SWITCHES_OFF))
    with np.load(out) as f:
        _same({k: f[k] for k in f.files}, recorded, "off")


def test_the_two_recorded_tables_differ(recorded):
    """The switches do move slab counts (the streaming weight gradients size their grids differently) and AFFINE2 support, so
    the second table is not a copy of the first."""
    assert (recorded["on_wgrad_num_blocks"] != recorded["off_wgrad_num_blocks"]).any()
    assert recorded["on_wgrad_t_affine2"].any() and not recorded["off_wgrad_t_affine2"].any()
