"""The shifted-product forward of the decoder's transposed convolutions (conv_mfma.hip, kernel E): dec.2 (8 -> 4 channels on a
32 x 32 grid) and dec.0 (16 -> 8 on 16 x 16), and the same layers on the 256-pixel workload's grids (64 x 64 with four M tiles
per row, 32 x 32 in bands of 8 rows), through the call the engine makes.

Every product of the kernel carries a real weight; the side products reach their output one column (and, for dec.2, through the
skewed accumulator rows, one row) away.  So the tests look at the places where a shift can go wrong: the image's border
(padding instead of a neighbour), the seam between the two M tiles of a row, the seam between row bands / waves, and a
workgroup's tile walk (first tile, a middle one, a ragged last round)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (CIN, COUT, H, W, persistent grid of the layer's kernel: 256 CUs x workgroups per CU)
LAYERS = {"dec2": (8, 4, 32, 32, 768), "dec0": (16, 8, 16, 16, 512), "dec2_64": (8, 4, 64, 64, 768), "dec0_32": (16, 8, 32, 32, 512)}
ALL = sorted(LAYERS)
CASES = [(l, b) for l in ALL for b in (1, 3)] + [("dec2", "walk"), ("dec0", "walk")]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def tiles_per_sample(layer):
    ci, co, h, w, grid = LAYERS[layer]
    return h // (16 if w == 16 else 8)         # 16-wide tiles take 16 rows, the others 8


def big_batch(layer):
    """Smallest batch with at least 2 x grid + 1 tiles: every workgroup walks two tiles, the first ones a third."""
    grid = LAYERS[layer][4]
    return -(-(2 * grid + 1) // tiles_per_sample(layer))


def run(ops, layer, x, wt, bias):
    ci, co, h, w, _ = LAYERS[layer]
    out, _ = ops.conv3x3(ops.Op(x.to(DEV)), ops.weight_view(wt.to(DEV), 16, co * 16, 4, 1), x.shape[0], ci, 4 * co, h, w, taps=9,
                         pixel_shuffle=True, bias=bias.to(DEV), relu=True)
    torch.cuda.synchronize()
    return out.cpu()


@functools.lru_cache(maxsize=None)
def case(layer, B):
    """Inputs, the float64 reference and the elementwise bound, computed once per (layer, batch)."""
    ci, co, h, w, _ = LAYERS[layer]
    x = rnd(B, ci, h, w, seed=11 + B)
    wt = rnd(ci, co, 4, 4, seed=5, scale=0.3)
    bias = rnd(co, seed=6)
    ref = F.relu(F.conv_transpose2d(x.double(), wt.double(), bias.double(), stride=2, padding=1))
    # sum |w| |x| over the output's own 2 x 2 x CIN window, + |bias|
    mag = F.conv_transpose2d(x.double().abs(), wt.double().abs(), bias.double().abs(), stride=2, padding=1)
    bound = (4 * ci + 4) * 2.0 ** -24 * mag
    return x, wt, bias, ref, bound


@pytest.fixture(scope="module")
def ops():
    from dynamorph_amd import ops as o
    return o


@pytest.mark.parametrize("layer,batch", CASES)
def test_float64_bound(ops, layer, batch):
    """|out - ref| <= (4 CIN + 4) 2^-24 (sum |w| |x| + |bias|): the standard bound for the at most 4 CIN + 4 fp32 operations of
    an output, whatever their order; ReLU does not enlarge it."""
    B = big_batch(layer) if batch == "walk" else batch
    x, wt, bias, ref, bound = case(layer, B)
    out = run(ops, layer, x, wt, bias)
    assert out.shape == ref.shape
    err = (out.double() - ref).abs()
    worst = float((err / bound).max())
    print(f"{layer} B={B}: max |out - ref| = {float(err.max()):.3e}, max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst


@pytest.mark.parametrize("layer", ALL)
def test_placed_values(ops, layer):
    """One non-zero input per sample -- the corners, the edge midpoints, one interior position -- and a different weight for every
    (ci, co, ky, kx): every output is bias, or the ONE product that reaches it plus bias, exactly.  A shift taken the wrong way
    or a missing padding column / row puts a product somewhere else."""
    ci, co, h, w, _ = LAYERS[layer]
    places = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 2 - 1), (h // 2, 0), (h // 2 - 1, w - 1),
              (h // 2 - 1, w // 2 - 1), (h // 4 - 1, w // 2 - 1), (h // 4, w // 2)]      # (the last two: a row-band seam)
    B = len(places)
    x = torch.zeros(B, ci, h, w)
    wt = ((torch.arange(ci * co * 16, dtype=torch.float32) + 1.0) / 4096.0).reshape(ci, co, 4, 4)      # exact, all different
    bias = (torch.arange(co, dtype=torch.float32) + 1.0) / 64.0
    exp = np.broadcast_to(bias.numpy()[None, :, None, None], (B, co, 2 * h, 2 * w)).copy()
    for s, (y, xx) in enumerate(places):
        c, val = s % ci, np.float32(1.5 + s)
        x[s, c, y, xx] = float(val)
        for ky in range(4):
            for kx in range(4):
                oy, ox = 2 * y - 1 + ky, 2 * xx - 1 + kx
                if 0 <= oy < 2 * h and 0 <= ox < 2 * w:
                    exp[s, :, oy, ox] = (val * wt[c, :, ky, kx].numpy()).astype(np.float32) + bias.numpy()
    out = run(ops, layer, x, wt, bias).numpy()
    bad = np.argwhere(out != exp)
    assert bad.size == 0, (len(bad), bad[:8].tolist())


@pytest.mark.parametrize("layer", ALL)
def test_non_finite_inputs_reach_only_what_they_feed(ops, layer):
    """A NaN and an Inf input: the outputs are non-finite exactly where the float64 reference's are (no 0 x NaN from a weight
    that is zero by construction), and the rest stays within the bound."""
    ci, co, h, w, _ = LAYERS[layer]
    x, wt, bias, _, _ = case(layer, 3)
    x = x.clone()
    x[0, 1, 0, 0] = float("nan")                 # a corner: its products also point into the padding
    x[1, ci - 1, h // 2, w // 2 - 1] = float("inf")       # beside the seam of the row's two M tiles (dec.2), on a wave's band edge
    x[2, 2, h - 1, w - 1] = float("-inf")
    ref = F.relu(F.conv_transpose2d(x.double(), wt.double(), bias.double(), stride=2, padding=1))
    out = run(ops, layer, x, wt, bias).double()
    fin_ref, fin_out = torch.isfinite(ref), torch.isfinite(out)
    assert int((~fin_ref).sum()) > 0
    assert torch.equal(fin_out, fin_ref), int((fin_out != fin_ref).sum())
    assert torch.equal(torch.isnan(out), torch.isnan(ref))
    xf = torch.where(torch.isfinite(x), x, torch.zeros(()))
    mag = F.conv_transpose2d(xf.double().abs(), wt.double().abs(), bias.double().abs(), stride=2, padding=1)
    err = torch.where(fin_ref, (out - ref).abs(), torch.zeros((), dtype=torch.float64))
    assert bool((err <= (4 * ci + 4) * 2.0 ** -24 * mag).all())
