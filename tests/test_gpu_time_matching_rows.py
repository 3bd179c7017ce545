"""GPU: the row-range time-matching pair (dm_time_matching_forward_rows / _backward_rows) against the square pair on the same
latents and relation block.  A partition of the batch's rows into ranges -- ragged ones and an empty one included -- must
give S and dz rows bit-equal to the square call's, and row shares of the loss that add up to its loss; the global value is
also held against float64 torch from the reference's formula (vq_vae.py:324-332, vae.py:327-336)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
W_A, W_T, W_N, MARGIN = 1.5, 0.5, -0.25, 0.1       # mode 1 weights: a live and a dead part of the hinge


def _latents(Bg, n, seed):
    """Random latents with near pairs: every fourth sample is a small perturbation of its predecessor (the pairs the term
    exists for, re-evaluated from differences), and one exact duplicate."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(Bg, n, generator=g) * 0.5
    for i in range(1, Bg, 4):
        z[i] = z[i - 1] + 1e-3 * torch.randn(n, generator=g)
    if Bg > 5:
        z[5] = z[2]
    return z.to(DEV).contiguous()


def _relations(Bg, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "dense_sym":
        t = torch.randint(0, 3, (Bg, Bg), generator=g).float()
        t = torch.triu(t) + torch.triu(t, 1).T
    elif kind == "dense_asym":
        t = torch.randint(0, 3, (Bg, Bg), generator=g).float()
    else:                                           # a few related frames per row (mode 0's sparse form), not symmetric
        t = torch.zeros(Bg, Bg)
        for i in range(Bg):
            for d in (1, 2, 5):
                if i + d < Bg:
                    t[i, i + d] = float(1 + (i + d) % 2)
            if i >= 3:
                t[i, i - 3] = 1.0
    return t.to(DEV).contiguous()


def _splits(Bg, parts):
    """Contiguous row ranges: the data-parallel shards (sizes differing by one), and one partition with an empty range."""
    from dynamorph_amd import dist as D
    even = [D.shard_range(Bg, r, parts) for r in range(parts)]
    cuts = sorted({0, Bg} | {min(Bg, (Bg * k * k) // (parts * parts)) for k in range(1, parts)} | {Bg // 3})
    skew = [(0, 0)] + [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    return [even, skew]


def _reference_loss(z, tm, mode):
    z = z.double()
    gram = z @ z.T
    d = torch.diagonal(gram)
    sim = (d[:, None] + d[None, :] - 2 * gram) / z.shape[1]
    sim.fill_diagonal_(0.0)
    # (near pairs from differences, as the reference forms every pair)
    t = tm.double()
    if mode == 0:
        return float((sim * t).sum())
    w = torch.where(t == 2, torch.full_like(t, W_A), torch.where(t == 1, torch.full_like(t, W_T),
                                                                  torch.where(t == 0, torch.full_like(t, W_N), t)))
    v = sim * w
    v = torch.where(t == 0, torch.clamp(v + MARGIN, min=0), v)
    return float(v.mean())


@pytest.mark.parametrize("n", [4096, 65536])
@pytest.mark.parametrize("Bg", [6, 64, 200, 768])
@pytest.mark.parametrize("mode", [0, 1])
def test_row_ranges_equal_square_rows(mode, Bg, n):
    from dynamorph_amd import ops
    z = _latents(Bg, n, seed=Bg + n + mode)
    add = torch.randn(Bg, n, generator=torch.Generator().manual_seed(3)).to(DEV)
    args = (mode, W_A, W_T, W_N, MARGIN)
    for kind in ("dense_sym", "dense_asym", "sparse"):
        tm = _relations(Bg, kind, seed=Bg + 7)
        loss_sq, S_sq = ops.time_matching_forward(z, tm, *args)
        dz_sq = ops.time_matching_backward(z, S_sq, None, 3.0, add=add)
        ref = _reference_loss(z, tm, mode)
        assert abs(float(loss_sq) - ref) <= 1e-5 * max(abs(ref), 1e-6 * Bg * Bg), (kind, float(loss_sq), ref)
        for parts in (1, 2, 3, 8):                  # 1: the single range (0, Bg), the row-range pair as the square one
            for ranges in ([[(0, Bg)]] if parts == 1 else _splits(Bg, parts)):
                total = 0.0
                covered = 0
                for r0, r1 in ranges:
                    R = r1 - r0
                    part, S = ops.time_matching_forward_rows(z, tm, r0, R, *args)
                    dz = ops.time_matching_backward_rows(z, S, None, 3.0, add=add[r0:r1].contiguous())
                    assert S.shape == (2, R, Bg) and dz.shape == (R, n)
                    what = (kind, parts, r0, r1)
                    assert torch.equal(S, S_sq[:, r0:r1]), what
                    assert torch.equal(dz, dz_sq[r0:r1]), what
                    total += float(part)
                    covered += R
                assert covered == Bg
                assert abs(total - float(loss_sq)) <= 1e-6 * max(abs(float(loss_sq)), 1e-30), (kind, parts, total, float(loss_sq))


def _relations_filled(Bg, per_row, seed):
    """An asymmetric relation block with `per_row` nonzero entries (1 or 2) in every row, the diagonal included or not as the
    draw has it: above 32 per row mode 0 takes the Gram path, at or below it the sparse one."""
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(Bg, Bg)
    for i in range(Bg):
        cols = torch.randperm(Bg, generator=g)[:per_row]
        t[i, cols] = torch.randint(1, 3, (len(cols),), generator=g).float()
    return t.to(DEV).contiguous()


@pytest.mark.parametrize("Bg", [6, 70, 130])
@pytest.mark.parametrize("mode", [0, 1])
def test_whole_range_equals_square_at_small_batches(mode, Bg):
    """The row-range pair with r0 = 0, R = B against the square pair -- the identity the shared backward launch rests on --
    and a ragged two-way cut, on one, two and three tiles of 64 with a ragged last tile; 6, 70 and 130 are no multiples of
    four (the scalar S loads) and keep 4 rows per epilogue workgroup.  Two asymmetric relation blocks: 40 entries per row
    (6 at Bg = 6: every entry) where a row can hold them -- above the sparse form's 32 per row --, and 3 per row, sparse."""
    from dynamorph_amd import ops
    n = 256
    z = _latents(Bg, n, seed=Bg + mode)
    add = torch.randn(Bg, n, generator=torch.Generator().manual_seed(5)).to(DEV)
    args = (mode, W_A, W_T, W_N, MARGIN)
    for per_row in (min(40, Bg), 3):
        tm = _relations_filled(Bg, per_row, seed=Bg + per_row)
        dense = int((tm != 0).sum()) > 32 * Bg
        assert dense == (per_row > 32)
        slabs_sq, S_sq = ops.time_matching_forward(z, tm, *args, want_slabs=True)
        loss_sq = float(slabs_sq[:, 0, 0].sum())
        dz_sq = ops.time_matching_backward(z, S_sq, None, 3.0, add=add)
        dz_sq_plain = ops.time_matching_backward(z, S_sq, None, 3.0)
        ref = _reference_loss(z, tm, mode)
        assert abs(loss_sq - ref) <= 1e-5 * max(abs(ref), 1e-6 * Bg * Bg), (per_row, loss_sq, ref)
        for ranges in ([(0, Bg)], [(0, Bg // 3), (Bg // 3, Bg)]):
            total = 0.0
            for r0, r1 in ranges:
                slabs, S = ops.time_matching_forward_rows(z, tm, r0, r1 - r0, *args, want_slabs=True)
                dz = ops.time_matching_backward_rows(z, S, None, 3.0, add=add[r0:r1].contiguous())
                dz_plain = ops.time_matching_backward_rows(z, S, None, 3.0)
                what = (per_row, r0, r1)
                assert torch.equal(S, S_sq[:, r0:r1]), what
                assert torch.equal(dz, dz_sq[r0:r1]), what
                assert torch.equal(dz_plain, dz_sq_plain[r0:r1]), what
                total += float(slabs[:, 0, 0].sum())
            assert abs(total - loss_sq) <= 1e-6 * max(abs(loss_sq), 1e-30), (per_row, ranges, total, loss_sq)


def test_row_ranges_on_a_side_stream():
    """The pair enqueued on a stream other than the default one (a captured training step records on a side stream)."""
    from dynamorph_amd import ops
    Bg, n = 64, 4096
    z = _latents(Bg, n, seed=4)
    tm = _relations(Bg, "dense_asym", seed=5)
    _, S_sq = ops.time_matching_forward(z, tm, 1, W_A, W_T, W_N, MARGIN)
    dz_sq = ops.time_matching_backward(z, S_sq, None, 1.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _, S = ops.time_matching_forward_rows(z, tm, 20, 30, 1, W_A, W_T, W_N, MARGIN)
        dz = ops.time_matching_backward_rows(z, S, None, 1.0)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(dz, dz_sq[20:50])


def test_row_ranges_reject_ranges_outside_the_batch():
    from dynamorph_amd import ops
    z = _latents(8, 4096, seed=1)
    tm = _relations(8, "dense_sym", seed=2)
    with pytest.raises(ValueError):
        ops.time_matching_forward_rows(z, tm, 5, 4, 0)
    with pytest.raises(ValueError):
        ops.time_matching_forward_rows(z, tm[:4, :4].contiguous(), 0, 4, 0)
