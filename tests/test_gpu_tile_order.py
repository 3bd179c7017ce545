"""The order in which a persistent workgroup walks its tiles (csrc/tile.h, tile_id) must not show in the results.

enc.4's forward (dm_conv4x4s2, 8 -> 16 channels) and kernel D (dm_conv_bwd_s2_fused, 16 -> 8) walk their tiles from the END of
the tensors; the training decoder tail (dm_dec_tail_train) was measured both ways and walks up -- the test holds
whichever way a kernel walks.  Each is run on a batch with more than two tiles per
workgroup and a ragged last round (ntiles > 2 * grid, ntiles % grid != 0; the grid taken from the entry point's *_num_blocks),
on one sample, and on a batch with fewer tiles than workgroups, and held to the SAME entry point run on consecutive chunks of
the batch of at most 256 tiles each: every variant launches at least one workgroup per compute unit (256), so a chunk is one
tile per workgroup and no traversal order exists.

  data tensors (a2, dx, g2, per-tile statistics slabs)   bit-equal to the chunks': a wrong decode, a misplaced store, a stale
                                                          next-tile coefficient or a slab under the wrong tile id shows
  per-workgroup slabs, summed on the host in float64     against the float64 sums of the chunks' slabs, within the bounds of
                                                          tests/helpers/glue_reference.py:
      double slabs (statistics, loss): the terms are fp32 values added in double, only the order differs: F64_SLOP times the
          sum of the terms' magnitudes (sum_slabs_ref);
      float slabs (weight gradients) and the tail's per-lane fp32 partials: a workgroup adds its tiles in fp32, the chunks add
          them in float64: n U sum |x| over the chunks' slabs x with n the slab count of the whole run (reduce_slabs_ref).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import glue_reference as G  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ONE_PER_WG = 256          # tiles of a chunk: no variant launches fewer workgroups than compute units


@pytest.fixture(scope="module")
def ops():
    from dynamorph_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from dynamorph_amd import _lib
    return _lib.load()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def ragged_batch(grid, per_sample, pow2_chunks=False):
    """Smallest B with ntiles > 2 * grid and a ragged last round for every grid a variant may take (a multiple of 256 up to
    `grid`: ntiles % 256 != 0 covers them all).  pow2_chunks: B is also 2**k chunks of at most ONE_PER_WG tiles."""
    B = 2 * grid // per_sample + 1
    while True:
        nt = B * per_sample
        c = B
        while pow2_chunks and c % 2 == 0 and c * per_sample > ONE_PER_WG:
            c //= 2
        if nt > 2 * grid and nt % 256 != 0 and nt % grid != 0 and (not pow2_chunks or c * per_sample <= ONE_PER_WG):
            return B, (c if pow2_chunks else ONE_PER_WG // per_sample)
        B += 1


def chunks_of(B, step):
    return [slice(s, min(s + step, B)) for s in range(0, B, step)]


def d64(t):
    return t.detach().cpu().double()


def within(got, want, bound, what):
    err = (d64(got) - want).abs()
    worst = float(torch.nan_to_num(err / bound, nan=0.0).max())
    print(f"[tile order] {what}: worst error / bound {worst:.3g}")
    assert not (err > bound).any(), f"{what}: {worst:.2f} bounds (max err {float(err.max()):.3e})"


def double_slabs(got, ref_slabs, what):
    """Double slabs (nslabs, n, 2) of the whole run against the chunks' slabs: float64 sums, order only."""
    ref = torch.cat([d64(s) for s in ref_slabs], 0)
    within(d64(got).sum(0), ref.sum(0), G.F64_SLOP * ref.abs().sum(0) + G.DENORM, what)


def float_slabs(got, ref_slabs, what):
    """Slabs a workgroup filled by adding its tiles in fp32 (weight gradients; the tail's partials, stored as doubles)."""
    ref = torch.cat([d64(s) for s in ref_slabs], 0)
    within(d64(got).sum(0), ref.sum(0), got.shape[0] * G.U * ref.abs().sum(0) + G.DENORM, what)


# ====================================================================================== enc.4 forward: dm_conv4x4s2, 8 -> 16
C4_CIN, C4_NOUT, C4_HW = 8, 16, 64


def conv4_inputs(B, per_sample):
    x = rnd(B, C4_CIN, C4_HW, C4_HW, seed=11)
    shape = (B, C4_CIN) if per_sample else (C4_CIN,)
    coef = torch.stack([rnd(*shape, seed=12).abs() + 0.5, torch.zeros(shape), rnd(*shape, seed=13) * 0.3, torch.zeros(shape)], -1)
    return x.to(DEV), coef.to(DEV), rnd(C4_NOUT, C4_CIN, 4, 4, seed=14, scale=0.2).to(DEV), rnd(C4_NOUT, seed=15).to(DEV)


def conv4_run(ops, x, coef, w, bias, sl, per_sample):
    n = sl.stop - sl.start
    c = coef[sl].contiguous() if per_sample else coef
    return ops.conv4x4s2(ops.Op(x[sl].contiguous(), 3, c, per_sample=per_sample), ops.weight_view(w, C4_CIN * 16, 16, 4, 1), n,
                         C4_CIN, C4_NOUT, C4_HW, C4_HW, want_stats=True, bias=bias, per_tile=per_sample)


@pytest.mark.parametrize("per_sample", [False, True], ids=["batch_stats", "per_sample_coef"])
def test_conv4x4s2_whole_batch_equals_one_tile_per_workgroup(ops, lib, per_sample):
    per = (C4_HW // 2 // 8) * (C4_HW // 2 // 32)                         # 8 x 32 output tiles
    grid = lib.dm_conv4x4s2_num_blocks(1 << 20, C4_CIN, C4_NOUT, C4_HW, C4_HW, 0)
    B, step = ragged_batch(grid, per)
    assert lib.dm_conv4x4s2_num_blocks(B, C4_CIN, C4_NOUT, C4_HW, C4_HW, 0) == grid and B * per > 2 * grid and (B * per) % grid
    x, coef, w, bias = conv4_inputs(B, per_sample)
    parts = [conv4_run(ops, x, coef, w, bias, sl, per_sample) for sl in chunks_of(B, step)]
    ref_out = torch.cat([p[0] for p in parts], 0)
    for Bs in (B, 1, step // 2 + 1):                                     # ragged rounds; one sample; fewer tiles than workgroups
        out, st = conv4_run(ops, x, coef, w, bias, slice(0, Bs), per_sample)
        assert torch.equal(out, ref_out[:Bs]), f"B = {Bs}: output differs from the one-tile-per-workgroup runs"
        if per_sample:          # one slab per TILE, under the tile's id, through the sample's own coefficients: bit for bit
            ref_st = torch.cat([p[1] for p in parts], 0)[:Bs * per]
            assert st.shape[0] == Bs * per and torch.equal(st, ref_st), f"B = {Bs}: per-tile statistics slabs"
        else:
            o = d64(ref_out[:Bs])
            want = torch.stack([o.sum((0, 2, 3)), (o * o).sum((0, 2, 3))], 1)
            mag = torch.stack([o.abs().sum((0, 2, 3)), (o * o).sum((0, 2, 3))], 1)
            # four elements in fp32, then double: C_STATS U against the exact sums; the ORDER of the doubles against the chunks
            within(d64(st).sum(0), want, G.C_STATS * G.U * mag, f"conv4x4s2 B = {Bs} statistics vs float64")
            if Bs == B:
                double_slabs(st, [p[1] for p in parts], f"conv4x4s2 B = {Bs} statistics vs chunks")


# ====================================================================================== kernel D: dm_conv_bwd_s2_fused, 16 -> 8
def test_conv_bwd_s2_fused_whole_batch_equals_one_tile_per_workgroup(ops, lib):
    CD, CX, H = 16, 8, 32
    per = (H // 8) * (H // 32)
    grid = lib.dm_conv_bwd_s2_fused_num_blocks(1 << 16, CD, CX, H, H)
    B, step = ragged_batch(grid, per)
    assert lib.dm_conv_bwd_s2_fused_num_blocks(B, CD, CX, H, H) == grid and B * per > 2 * grid and (B * per) % grid
    dy, a_out, a_in = rnd(B, CD, H, H, seed=1).to(DEV), rnd(B, CD, H, H, seed=2).to(DEV), rnd(B, CX, 2 * H, 2 * H, seed=6).to(DEV)
    cD = torch.stack([rnd(CD, seed=3), rnd(CD, seed=4) * 0.1, rnd(CD, seed=5) * 0.1, torch.zeros(CD)], 1).to(DEV)
    cT = torch.stack([rnd(CX, seed=7).abs() + 0.5, torch.zeros(CX), rnd(CX, seed=8) * 0.3, torch.zeros(CX)], 1).to(DEV)
    w = rnd(CD, CX, 4, 4, seed=9, scale=0.2).to(DEV)

    def run(sl):
        n = sl.stop - sl.start
        ai = a_in[sl].contiguous()                                      # (one tensor: the kernel checks that the mask IS the input)
        pending = []
        dx, st = ops.conv_bwd_s2_fused(ops.Op(dy[sl].contiguous(), 4, cD, p1=a_out[sl].contiguous()), ops.Op(ai, 3, cT),
                                       ops.weight_view(w, 16, CX * 16, 4, 1), None, n, CD, CX, H, H, mask=ops.Op(ai, 2, cT),
                                       stat_q=ai, pending=pending)
        return dx, st, pending[0][0]

    parts = [run(sl) for sl in chunks_of(B, step)]
    ref_dx = torch.cat([p[0] for p in parts], 0)
    for Bs in (B, 1, step // 2 + 1):                                     # ragged rounds; one sample; fewer tiles than workgroups
        dx, st, ws = run(slice(0, Bs))
        assert torch.equal(dx, ref_dx[:Bs]), f"B = {Bs}: data gradient differs from the one-tile-per-workgroup runs"
        if Bs == B:
            double_slabs(st, [p[1] for p in parts], "kernel D statistics vs chunks")
            float_slabs(ws, [p[2] for p in parts], "kernel D weight-gradient slabs vs chunks")


# ====================================================================================== decoder tail: dm_dec_tail_train
@pytest.mark.parametrize("NIN", [2, 4])
def test_dec_tail_train_whole_batch_equals_one_tile_per_workgroup(ops, lib, NIN):
    H2 = 64
    per = H2 // 8
    grid = lib.dm_dec_tail_num_blocks(1 << 16, H2, H2)
    # the kernel scales the gradient by 2 gscale / (B NIN OH OW), rounded to fp32: a chunk reproduces the whole batch's factor
    # bit for bit where B / chunk is a power of two (gscale of the chunk = gscale * chunk / B)
    B, step = ragged_batch(grid, per, pow2_chunks=True)
    assert lib.dm_dec_tail_num_blocks(B, H2, H2) == grid and B * per > 2 * grid and (B * per) % grid and (B // step) * step == B
    g = torch.Generator().manual_seed(40 + NIN)
    d2 = torch.randn(B, 4, H2, H2, generator=g).clamp(min=0).to(DEV)
    w4, b4 = (torch.randn(4, 4, 4, 4, generator=g) * 0.3).to(DEV), torch.randn(4, generator=g).to(DEV)
    w6, b6 = torch.randn(NIN, 4, generator=g).to(DEV), torch.randn(NIN, generator=g).to(DEV)
    x = torch.randn(B, NIN, 2 * H2, 2 * H2, generator=g).to(DEV)
    var = torch.logspace(-1.0, 0.5, NIN).to(DEV)
    gscale = 0.75

    def run(sl, of):
        n = sl.stop - sl.start
        assert (of // n) * n == of and ((of // n) & (of // n - 1)) == 0
        gs = torch.tensor([gscale * n / of], device=DEV)
        return ops.dec_tail_train(d2[sl].contiguous(), w4, b4, w6, b6, x[sl].contiguous(), None, var, gs)

    parts = [run(sl, B) for sl in chunks_of(B, step)]
    ref_g2 = torch.cat([p[0] for p in parts], 0)
    g2, part, wsl, loss = run(slice(0, B), B)
    assert torch.equal(g2, ref_g2), "g2 differs from the one-tile-per-workgroup runs"
    assert float(part[:, :, 1].abs().max()) == 0.0
    float_slabs(part[:, :, 0], [p[1][:, :, 0] for p in parts], f"tail NIN = {NIN} dW6 | db6 | db4 | db2 vs chunks")
    float_slabs(wsl, [p[2] for p in parts], f"tail NIN = {NIN} dW4 slabs vs chunks")
    double_slabs(loss.reshape(-1, 1, 1), [p[3].reshape(-1, 1, 1) for p in parts], f"tail NIN = {NIN} loss vs chunks")
    if NIN == 2:
        # fewer tiles than workgroups (16 samples against chunks of one), and one sample against sample 0 of a pair
        few = run(slice(0, 16), 16)
        ones = [run(slice(i, i + 1), 16) for i in range(16)]
        assert torch.equal(few[0], torch.cat([p[0] for p in ones], 0)), "16 samples: g2 differs from single-sample runs"
        double_slabs(few[3].reshape(-1, 1, 1), [p[3].reshape(-1, 1, 1) for p in ones], "tail 16 samples loss")
        float_slabs(few[2], [p[2] for p in ones], "tail 16 samples dW4 slabs")
        assert torch.equal(run(slice(0, 1), 2)[0], run(slice(0, 2), 2)[0][:1]), "one sample: g2 differs from sample 0 of a pair"
