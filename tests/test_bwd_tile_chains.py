"""The persistent fused backward kernels on batches where a workgroup runs a first, a middle and a last tile.

Their tile loops keep the next tile's loads and the finished tile's stores in flight across the commit.  What a wrong wait
corrupts there is a tile that FOLLOWS another tile, and the other kernel tests stop at two tiles per workgroup.  Here every
entry point runs B = 2 x grid + 1 distinct samples (grid: what *_num_blocks answers for B = 2048), so some workgroups run
three tiles, the others two, and the last position has no successor.  For the samples 0, grid - 1, grid, 2 grid (= B - 1):
the data gradient is bit-equal to the same sample run alone and within 3e-6 x scale of float64 autograd; weight gradient and
statistics are checked against float64 on the whole batch with the bounds of test_gpu_kernels.py; two calls are bit-equal.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from dynamorph_amd import ops as o
    return o


def close(a, b, rtol, atol, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max():.3e} (ref max {b.abs().max():.3e})"


def picks(grid, B):
    assert B == 2 * grid + 1
    return sorted({0, grid - 1, grid, 2 * grid, B - 1})


def d(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("CI,CO,H,W,mask", [(16, 8, 16, 16, False), (8, 4, 32, 32, True)])
def test_conv_transpose_backward_fused_three_tiles_per_workgroup(ops, CI, CO, H, W, mask):
    from dynamorph_amd import _lib as L
    grid = L.load().dm_convt_bwd_fused_num_blocks(2048, CI, CO, H, W)
    assert grid == (768 if CI == 8 else 512)                     # (a sample is 4 / 2 tiles here: every workgroup runs a chain of them)
    B = 2 * grid + 1
    g = torch.Generator().manual_seed(CI + H)
    S = torch.randn(B, CI, H, W, generator=g)
    if mask:
        S = S.clamp(min=0)
    G = torch.randn(B, CO, 2 * H, 2 * W, generator=g)
    w = torch.randn(CI, CO, 4, 4, generator=g) * 0.2
    dS, dG, dw = d(S), d(G), d(w)
    dst = torch.zeros(CI, CO, 4, 4, device=DEV)
    gin, st = ops.convT_bwd_fused(dS, dG, dw, dst, mask_relu=mask, want_stats=True)
    assert st.shape[0] == grid
    S64, w64 = S.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv_transpose2d(S64, w64, stride=2, padding=1).backward(G.double())
    gin_ref = S64.grad * (S.double() > 0) if mask else S64.grad
    scale = float(gin_ref.abs().max())
    for i in picks(grid, B):
        one, _ = ops.convT_bwd_fused(dS[i:i + 1].contiguous(), dG[i:i + 1].contiguous(), dw, torch.zeros_like(dst), mask_relu=mask)
        assert torch.equal(one[0], gin[i]), f"sample {i}: differs from the sample run alone"
        assert float((gin[i].cpu().double() - gin_ref[i]).abs().max()) <= 3e-6 * scale, f"sample {i}"
    close(dst, w64.grad.float(), 1e-5, 3e-5 * float(w64.grad.abs().max()), "weight gradient vs float64")
    close(st.sum(0)[:, 0].cpu(), gin.cpu().double().sum((0, 2, 3)), 1e-6, 1e-6 * float(gin_ref.abs().sum((0, 2, 3)).max()), "channel sums")
    dst3 = torch.zeros_like(dst)
    gin3, st3 = ops.convT_bwd_fused(dS, dG, dw, dst3, mask_relu=mask, want_stats=True)
    assert torch.equal(gin3, gin) and torch.equal(dst3, dst) and torch.equal(st3, st)


@pytest.mark.parametrize("CD,form,hw", [(32, "res", (16, 16)), (16, "enc10", (16, 16)), (32, "res", (32, 32))])
def test_conv3x3_backward_fused_three_tiles_per_workgroup(ops, CD, form, hw):
    from dynamorph_amd import _lib as L
    CX, (H, W) = 16, hw
    grid = L.load().dm_conv3x3_bwd_fused_num_blocks(2048, CD, CX, H, W)
    assert grid == (256 if CD == 32 else 512)
    B = 2 * grid + 1
    g = torch.Generator().manual_seed(CD + H)
    gy, y = torch.randn(B, CD, H, W, generator=g), torch.randn(B, CD, H, W, generator=g)
    x = torch.randn(B, CX, H, W, generator=g)
    w = torch.randn(CD, CX, 3, 3, generator=g) * 0.2
    cd = torch.randn(CD, 4, generator=g) * 0.5
    dgy, dyy, dx_in, dw, dcd = d(gy), d(y), d(x), d(w), d(cd)
    da = (cd[:, 0].view(1, CD, 1, 1).double() * gy.double() + cd[:, 1].view(1, CD, 1, 1).double() * y.double()
          + cd[:, 2].view(1, CD, 1, 1).double())
    if form == "enc10":
        cx = torch.zeros(CX, 4)
        cx[:, 0] = torch.rand(CX, generator=g) + 0.5
        cx[:, 2] = torch.randn(CX, generator=g) * 0.3
        xcoef, resid, q = d(cx), None, dx_in
        t = cx[:, 0].view(1, CX, 1, 1).double() * x.double() + cx[:, 2].view(1, CX, 1, 1).double()
    else:
        xcoef, t = None, x.double()
        resid, q = d(torch.randn(B, CX, H, W, generator=g)), d(torch.randn(B, CX, H, W, generator=g))
    run = lambda sl, dst, n: ops.conv3x3_bwd_fused(ops.Op(dgy[sl].contiguous(), 4, dcd, p1=dyy[sl].contiguous()), dx_in[sl].contiguous(),
                                                   xcoef, dw, dst, n, CD, resid=None if resid is None else resid[sl].contiguous(),
                                                   q=q[sl].contiguous())
    dst = torch.zeros(CD, CX, 3, 3, device=DEV)
    dx, st = run(slice(0, B), dst, B)
    assert st.shape[0] == grid
    t_in, w64 = t.clamp(min=0).requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(t_in, w64, padding=1).backward(da)
    dx_ref = t_in.grad * (t > 0) + (resid.cpu().double() if resid is not None else 0.0)
    near = t.abs() < 1e-5
    scale = float(dx_ref.abs().max())
    for i in picks(grid, B):
        one, _ = run(slice(i, i + 1), torch.zeros_like(dst), 1)
        assert torch.equal(one[0], dx[i]), f"sample {i}: differs from the sample run alone"
        assert float(((dx[i].cpu().double() - dx_ref[i]).abs() * ~near[i]).max()) <= 3e-6 * scale, f"sample {i}"
    close(dst, w64.grad.float(), 1e-5, 3e-5 * float(w64.grad.abs().max()), "weight gradient vs float64")
    qq = q.cpu().double()
    want1, want2 = dx.cpu().double().sum((0, 2, 3)), (dx.cpu().double() * qq).sum((0, 2, 3))
    close(st.sum(0)[:, 0].cpu(), want1, 1e-6, 1e-6 * float(dx_ref.abs().sum((0, 2, 3)).max()), "sum dx")
    close(st.sum(0)[:, 1].cpu(), want2, 1e-6, 1e-6 * float((dx_ref.abs() * qq.abs()).sum((0, 2, 3)).max()), "sum dx * q")
    dst3 = torch.zeros_like(dst)
    dx3, st3 = run(slice(0, B), dst3, B)
    assert torch.equal(dx3, dx) and torch.equal(dst3, dst) and torch.equal(st3, st)


def test_conv4x4s2_backward_fused_three_tiles_per_workgroup(ops):
    from dynamorph_amd import _lib as L
    C, H = 16, 16
    grid = L.load().dm_conv4x4s2_bwd_fused_num_blocks(2048, C, C, H, H)
    assert grid == 256
    B = 2 * grid + 1
    g = torch.Generator().manual_seed(7)
    gy, y = torch.randn(B, C, H, H, generator=g), torch.randn(B, C, H, H, generator=g)
    x = torch.randn(B, C, 2 * H, 2 * H, generator=g)
    w = torch.randn(C, C, 4, 4, generator=g) * 0.2
    cd = torch.randn(C, 4, generator=g) * 0.5
    cx = torch.zeros(C, 4)
    cx[:, 0] = torch.rand(C, generator=g) + 0.5
    cx[:, 2] = torch.randn(C, generator=g) * 0.3
    dgy, dyy, dxi, dw, dcd, dcx = d(gy), d(y), d(x), d(w), d(cd), d(cx)
    run = lambda sl, dst, n: ops.conv4x4s2_bwd_fused(ops.Op(dgy[sl].contiguous(), 4, dcd, p1=dyy[sl].contiguous()),
                                                     dxi[sl].contiguous(), dcx, dw, dst, n)
    dst = torch.zeros(C, C, 4, 4, device=DEV)
    dx, st = run(slice(0, B), dst, B)
    assert st.shape[0] == grid
    da = (cd[:, 0].view(1, C, 1, 1).double() * gy.double() + cd[:, 1].view(1, C, 1, 1).double() * y.double()
          + cd[:, 2].view(1, C, 1, 1).double())
    t = cx[:, 0].view(1, C, 1, 1).double() * x.double() + cx[:, 2].view(1, C, 1, 1).double()
    t_in, w64 = t.clamp(min=0).requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(t_in, w64, stride=2, padding=1).backward(da)
    dx_ref = t_in.grad * (t > 0)
    near = t.abs() < 1e-5
    scale = float(dx_ref.abs().max())
    for i in picks(grid, B):
        one, _ = run(slice(i, i + 1), torch.zeros_like(dst), 1)
        assert torch.equal(one[0], dx[i]), f"sample {i}: differs from the sample run alone"
        assert float(((dx[i].cpu().double() - dx_ref[i]).abs() * ~near[i]).max()) <= 3e-6 * scale, f"sample {i}"
    close(dst, w64.grad.float(), 1e-5, 3e-5 * float(w64.grad.abs().max()), "weight gradient vs float64")
    want1, want2 = dx.cpu().double().sum((0, 2, 3)), (dx.cpu().double() * x.double()).sum((0, 2, 3))
    close(st.sum(0)[:, 0].cpu(), want1, 1e-6, 1e-6 * float(dx_ref.abs().sum((0, 2, 3)).max()), "sum dx")
    close(st.sum(0)[:, 1].cpu(), want2, 1e-6, 1e-6 * float((dx_ref.abs() * x.double().abs()).sum((0, 2, 3)).max()), "sum dx * x")
    dst3 = torch.zeros_like(dst)
    dx3, st3 = run(slice(0, B), dst3, B)
    assert torch.equal(dx3, dx) and torch.equal(dst3, dst) and torch.equal(st3, st)


def test_conv4x4s2_whole_patch_forward_three_tiles_per_workgroup(ops):
    """The forward kernel of the same file walks patches the same way (256 workgroups)."""
    C, grid = 16, 256
    B = 2 * grid + 1
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, C, 32, 32, generator=g)
    w = torch.randn(C, C, 4, 4, generator=g) * 0.2
    bias = torch.randn(C, generator=g)
    coef = torch.stack([torch.rand(C, generator=g) + 0.5, torch.zeros(C), torch.randn(C, generator=g) * 0.3, torch.zeros(C)], 1)
    dxi, dw, db, dc = d(x), d(w), d(bias), d(coef)
    run = lambda sl, n: ops.conv4x4s2(ops.Op(dxi[sl].contiguous(), 3, dc), ops.weight_view(dw, C * 16, 16, 4, 1), n, C, C, 32, 32,
                                      want_stats=True, bias=db)
    out, st = run(slice(0, B), B)
    t = (coef[:, 0].view(1, C, 1, 1).double() * x.double() + coef[:, 2].view(1, C, 1, 1).double()).clamp(min=0)
    ref = F.conv2d(t, w.double(), bias.double(), stride=2, padding=1)
    for i in picks(grid, B):
        one, _ = run(slice(i, i + 1), 1)
        assert torch.equal(one[0], out[i]), f"sample {i}: differs from the sample run alone"
        close(out[i], ref[i], 2e-5, 2e-5, f"sample {i} vs float64")
    # sums of B * 256 = 131 k values per channel: 1e-6 of the sum of magnitudes (double accumulation of fp32 row sums)
    got = st.sum(0).cpu()
    o64 = out.cpu().double()
    close(got[:, 0], o64.sum((0, 2, 3)), 0, 1e-6 * float(o64.abs().sum((0, 2, 3)).max()), "sum out")
    close(got[:, 1], (o64 * o64).sum((0, 2, 3)), 0, 1e-6 * float((o64 * o64).sum((0, 2, 3)).max()), "sum out^2")
    out2, st2 = run(slice(0, B), B)
    assert torch.equal(out2, out) and torch.equal(st2, st)
