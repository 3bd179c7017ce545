"""GPU: the per-sample forms of BatchNorm's backward finaliser and of the channel statistics (csrc/bn.hip) against float64,
and the per-patch backward of the 16 x 16 latent stage (engine.latent_stage_backward: ops.latent_tail_backward and the chain) against
a float64 torch restatement of that stage (tests/helpers/patch_grad_reference.latent_stage_reference).

Bounds.  The finaliser's coefficients are float64 expressions of the given double sums stored once (scale: two roundings):
tests/helpers/glue_reference.bn_backward_ref's bounds for the batch form hold per patch as they stand.  dgamma / dbeta are
sums of B such float64 terms stored once: C_FIN U |sum| plus the float64 slop of the terms.  channel_stats: C_STATS, as for
the batch form (the same groups of four in fp32, added in double).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import glue_reference as R  # noqa: E402
import patch_grad_reference as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case(B, Cn, spg, seed):
    g = torch.Generator().manual_seed(seed)
    # slabs whose entries are fp32 values: any order of adding eight of them in double is exact, so the comparison with the
    # batch form at B = 1 (another order of the same additions) is a comparison of the arithmetic after the sums
    stats = torch.randn(B * spg, Cn, 2, generator=g).double() * 3.0
    saved = torch.stack([torch.randn(B, Cn, generator=g), torch.rand(B, Cn, generator=g) + 0.2], 2).float()
    gamma = (torch.randn(Cn, generator=g) * 0.5 + 1.0).float()
    return stats, saved, gamma


@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("Cn", [8, 16, 32])
@pytest.mark.parametrize("spg", [1, 8])
def test_bn_backward_finalize_per_sample_against_float64(B, Cn, spg):
    from dynamorph_amd import ops
    stats, saved, gamma = _case(B, Cn, spg, 100 * B + Cn + spg)
    count = 64 * spg
    sd, svd, gd = stats.to(DEV), saved.to(DEV), gamma.to(DEV)
    dgamma, dbeta = torch.full((Cn,), 7.0, device=DEV), torch.full((Cn,), 7.0, device=DEV)
    coef = ops.bn_backward_finalize_per_sample(sd, spg, count, gd, svd, dgamma, dbeta)
    assert tuple(coef.shape) == (B, Cn, 4)
    sums = stats.reshape(B, spg, Cn, 2).sum(1)
    tot_g, tot_b = torch.zeros(Cn, dtype=torch.float64), torch.zeros(Cn, dtype=torch.float64)
    slop_g, worst = torch.zeros(Cn, dtype=torch.float64), 0.0
    got = coef.cpu().double()
    for b in range(B):
        ref = R.bn_backward_ref(sums[b], count, gamma, saved[b])
        for j, k in ((0, "A"), (1, "Bc"), (2, "Cc")):
            err = (got[b, :, j] - ref[k]).abs()
            worst = max(worst, float((err / ref["b_" + k].clamp(min=1e-300)).max()))
            assert bool((err <= ref["b_" + k]).all()), (b, k, float(err.max()))
        assert float(got[b, :, 3].abs().max()) == 0.0
        tot_g, tot_b = tot_g + ref["dgamma"], tot_b + ref["dbeta"]
        slop_g = slop_g + ref["b_dgamma"] - R.C_FIN * R.U * ref["dgamma"].abs()
    print(f"B {B} C {Cn} slabs/patch {spg}: worst coefficient error / bound {worst:.2f}")
    assert bool(((dgamma.cpu().double() - tot_g).abs() <= R.C_FIN * R.U * tot_g.abs() + slop_g).all())
    assert bool(((dbeta.cpu().double() - tot_b).abs() <= R.C_FIN * R.U * tot_b.abs()).all())
    # the same bits at every launch, with and without the parameter sums
    dg2, db2 = torch.empty_like(dgamma), torch.empty_like(dbeta)
    coef2 = ops.bn_backward_finalize_per_sample(sd, spg, count, gd, svd, dg2, db2)
    coef3 = ops.bn_backward_finalize_per_sample(sd, spg, count, gd, svd)
    assert torch.equal(coef, coef2) and torch.equal(coef, coef3) and torch.equal(dgamma, dg2) and torch.equal(dbeta, db2)
    if B == 1:                               # one patch is a batch: the batch form with count = H * W, to the bit
        dg1, db1 = torch.empty_like(dgamma), torch.empty_like(dbeta)
        coef1 = ops.bn_backward_finalize(sd, count, gd, svd[0].contiguous(), dg1, db1)
        assert torch.equal(coef1, coef[0]) and torch.equal(dg1, dgamma) and torch.equal(db1, dbeta)


@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("Cn,hw", [(8, 32), (16, 16), (32, 8), (16, 6)])
@pytest.mark.parametrize("with_q", [True, False])
def test_channel_stats_per_sample_against_float64(B, Cn, hw, with_q):
    from dynamorph_amd import ops
    g = torch.Generator().manual_seed(7 * B + Cn + hw)
    p = torch.randn(B, Cn, hw, hw, generator=g)
    q = torch.randn(B, Cn, hw, hw, generator=g) + 0.5 if with_q else None
    st = ops.channel_stats_per_sample(p.to(DEV), None if q is None else q.to(DEV))
    assert tuple(st.shape) == (B, Cn, 2) and st.dtype == torch.float64
    st2 = ops.channel_stats_per_sample(p.to(DEV), None if q is None else q.to(DEV))
    assert torch.equal(st, st2)
    for b in range(B):
        s1, s2, b1, b2 = R.channel_stats_ref(p[b:b + 1], None if q is None else q[b:b + 1])
        assert bool(((st[b, :, 0].cpu() - s1).abs() <= b1).all()) and bool(((st[b, :, 1].cpu() - s2).abs() <= b2).all()), b
    # a patch's slab does not depend on its position or its neighbours
    if B > 1:
        one = ops.channel_stats_per_sample(p[B - 1:].to(DEV), None if q is None else q[B - 1:].to(DEV))
        assert torch.equal(one[0], st[B - 1])


def _encoder_context(B, nres, seed, hw=128):
    import dynamorph_amd
    from dynamorph_amd import engine as E
    torch.manual_seed(seed)
    m = dynamorph_amd.VQ_VAE(num_residual_layers=nres).to(DEV)
    with torch.no_grad():                                   # BatchNorm weights and biases away from 1 and 0
        for mod in m.enc.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
    L = E.Layers(m)
    x = torch.randn(B, 2, hw, hw, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    with torch.no_grad():
        z, cx = E.encoder_forward(L, x, per_sample=True)
    return m, L, cx, z


def _latent_stage(L, cx, g_z, fused):
    """engine.latent_stage_backward (encoder_backward's own first step) on a per_sample context, data only, by the one-launch
    kernel (ops.latent_tail_backward) or by the layer-by-layer chain: (dy3, per-patch slab (B, C, 2))."""
    from dynamorph_amd import engine as E
    dy3, st = E.latent_stage_backward(L, cx, g_z, None, want_param_grads=False, fused=fused)
    return dy3, st.reshape(cx.B, -1, L.nh, 2).sum(1)


@pytest.mark.parametrize("B,nres,zero_patch", [(1, 2, None), (2, 1, None), (5, 2, 3), (2, 2, 0)])
def test_latent_stage_backward_per_patch_against_float64(B, nres, zero_patch, monkeypatch):
    """enc.12 .. enc.10 backward with every patch's own statistics, fused and chain on the same saved context, both against
    autograd through functional batch_norm per patch in float64, on the yardstick of patch_gradients (e_ref: the same
    restatement in fp32).  A patch whose g_z is zero gets an exactly zero dy3 and slab: nothing of a neighbour leaked."""
    from dynamorph_amd import ops
    m, L, cx, _ = _encoder_context(B, nres, 300 + 10 * B + nres)
    g_z = torch.randn(B, 16, 16, 16, generator=torch.Generator().manual_seed(5))
    if zero_patch is not None:
        g_z[zero_patch] = 0.0
    calls = []
    real = ops.latent_tail_backward
    monkeypatch.setattr(ops, "latent_tail_backward", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        routes = {"chain": _latent_stage(L, cx, g_z.to(DEV), False), "fused": _latent_stage(L, cx, g_z.to(DEV), True)}
    assert len(calls) == 1                                 # the fused route ran the one-launch kernel, the chain did not
    w = lambda t: t.detach().cpu()        # noqa: E731
    res = [(w(ca.weight), w(ca.bias), w(bna.weight), w(bna.bias), bna.eps, w(cb.weight), w(cb.bias), w(bnb.weight), w(bnb.bias),
            bnb.eps) for ca, bna, cb, bnb in L.res]
    args = (w(cx.a3), w(L.bn3.weight), w(L.bn3.bias), L.bn3.eps, w(L.enc10.weight), w(L.enc10.bias), w(L.bn4.weight),
            w(L.bn4.bias), L.bn4.eps, res, g_z)
    _, dy64, slab64, frag = P.latent_stage_reference(*args, dtype=torch.float64)
    _, dy32, slab32, _ = P.latent_stage_reference(*args, dtype=torch.float32)
    for route, (dy3, slab) in routes.items():
        assert tuple(dy3.shape) == (B, 16, 16, 16) and tuple(slab.shape) == (B, 16, 2) and slab.dtype == torch.float64
        for b in range(B):
            if b == zero_patch:
                assert float(dy3[b].abs().max()) == 0.0 and float(slab[b].abs().max()) == 0.0, route
                continue
            fragile = int(frag[b])
            P.yardstick(dy3[b].cpu(), dy32[b], dy64[b], fragile, f"{route} dy3 B {B} nres {nres} patch {b}")
            P.yardstick(slab[b].cpu(), slab32[b], slab64[b], fragile, f"{route} slab B {B} nres {nres} patch {b}")


@pytest.mark.parametrize("fused", [True, False])
def test_a_patch_does_not_see_its_batch(fused):
    """The patch at positions 0 and B - 1 of a batch, and alone: bit-equal dy3 and slab; two launches give the same bits."""
    from dynamorph_amd import engine as E
    m, L, cx, _ = _encoder_context(4, 2, 77)
    x = cx.x
    g = torch.randn(4, 16, 16, 16, generator=torch.Generator().manual_seed(6)).to(DEV)
    perm = [3, 1, 2, 0]
    with torch.no_grad():
        dy_a, sl_a = _latent_stage(L, cx, g, fused)
        dy_r, sl_r = _latent_stage(L, cx, g, fused)
        _, cx2 = E.encoder_forward(L, x[perm].contiguous(), per_sample=True)
        dy_b, sl_b = _latent_stage(L, cx2, g[perm].contiguous(), fused)
        _, cx1 = E.encoder_forward(L, x[:1].contiguous(), per_sample=True)
        dy_c, sl_c = _latent_stage(L, cx1, g[:1].contiguous(), fused)
    assert torch.equal(dy_a, dy_r) and torch.equal(sl_a, sl_r)
    assert torch.equal(dy_a[0], dy_b[3]) and torch.equal(sl_a[0], sl_b[3])
    assert torch.equal(dy_a[3], dy_b[0]) and torch.equal(sl_a[3], sl_b[0])
    assert torch.equal(dy_a[0], dy_c[0]) and torch.equal(sl_a[0], sl_c[0])


def test_many_patches_per_workgroup():
    """More patches than workgroups (the kernel's grid stops at 256): patch b and patch b + 256 share a workgroup's LDS one
    after the other; every patch still equals its own single-patch launch."""
    from dynamorph_amd import engine as E
    m, L, cx, _ = _encoder_context(259, 2, 99)
    g = torch.randn(259, 16, 16, 16, generator=torch.Generator().manual_seed(8)).to(DEV)
    with torch.no_grad():
        dy, sl = _latent_stage(L, cx, g, True)
        for b in (0, 2, 256, 258):
            _, cx1 = E.encoder_forward(L, cx.x[b:b + 1].contiguous(), per_sample=True)
            dy1, sl1 = _latent_stage(L, cx1, g[b:b + 1].contiguous(), True)
            assert torch.equal(dy[b], dy1[0]) and torch.equal(sl[b], sl1[0]), b


@pytest.mark.parametrize("hw,routed", [(128, True), (64, False), (256, False)])
def test_the_gate_and_the_route_the_driver_takes(hw, routed, monkeypatch):
    """dm_latent_tail_supported is the gate: 16 x 16 latents take the one-launch kernel, 8 x 8 and 32 x 32 the chain."""
    import dynamorph_amd
    from dynamorph_amd import ops
    from dynamorph_amd.patch_vae import patch_gradients
    assert ops.latent_tail_supported(16, 32, hw // 8, hw // 8, 2) == routed
    calls = []
    real = ops.latent_tail_backward
    monkeypatch.setattr(ops, "latent_tail_backward", lambda *a, **k: calls.append(1) or real(*a, **k))
    torch.manual_seed(3)
    m = dynamorph_amd.VQ_VAE().to(DEV)
    x = torch.randn(2, 2, hw, hw, generator=torch.Generator().manual_seed(4))
    g = patch_gradients(m, x, device=DEV, batch_size=2)
    assert g.shape == (2, 2, hw, hw) and np.isfinite(g).all() and np.abs(g).max() > 0
    assert len(calls) == (1 if routed else 0)
    m.eval()                                                  # shared statistics: the chain, whatever the shape
    patch_gradients(m, x, device=DEV, batch_size=2)
    assert len(calls) == (1 if routed else 0)


def test_fused_backward_kernels_are_not_reached_per_sample(monkeypatch):
    """The four fused backward kernels keep one coefficient set per workgroup: a per_sample context never launches them."""
    from dynamorph_amd import engine as E, ops
    from dynamorph_amd.vq_vae import _GradBag
    m, L, cx, z = _encoder_context(3, 2, 88)

    def refuse(*a, **k):
        raise AssertionError("a fused backward kernel was launched with per-sample coefficients")
    for name in ("conv3x3_bwd_fused", "conv4x4s2_bwd_fused", "conv1x1_bwd_fused", "conv_bwd_s2_fused"):
        monkeypatch.setattr(ops, name, refuse)
    with torch.no_grad():
        dx = E.encoder_backward(L, cx, torch.randn_like(z), _GradBag(), want_dx=True)
    assert tuple(dx.shape) == tuple(cx.x.shape) and bool(torch.isfinite(dx).all())


class _Refuse:
    """A gradient bag a data-only pass must never ask."""

    def __call__(self, p):
        raise AssertionError("a data-only backward pass asked for a parameter's gradient buffer")


@pytest.mark.parametrize("synced", [False, True])
def test_data_only_mode_with_batch_statistics(synced, monkeypatch):
    """want_param_grads=False on a batch-statistics context, plain and under the synchronized-BatchNorm glue (one rank: the
    exchange is the identity): the gradient bag is never called, no weight-gradient, e1_chain or slab-reduction launch runs,
    and dx is the full pass's dx (two-launch pairs on both sides) to the bit."""
    import contextlib
    import dynamorph_amd
    from dynamorph_amd import engine as E, ops
    from dynamorph_amd.vq_vae import _GradBag
    torch.manual_seed(120)
    m = dynamorph_amd.VQ_VAE().to(DEV)
    L = E.Layers(m)
    x = torch.randn(3, 2, 128, 128, generator=torch.Generator().manual_seed(121)).to(DEV)
    g = torch.randn(3, 16, 16, 16, generator=torch.Generator().manual_seed(122)).to(DEV)
    monkeypatch.setattr(E, "FUSED_BACKWARD", False)      # the same data-gradient kernels on both sides
    sync = E.BnSync(torch.ones(2, dtype=torch.float64, device=DEV), lambda payload: None) if synced else None
    with torch.no_grad(), (E.bn_sync(sync) if synced else contextlib.nullcontext()):
        _, cx = E.encoder_forward(L, x)
        want = E.encoder_backward(L, cx, g, _GradBag(), want_dx=True)
        for name in ("wgrad", "e1_chain", "reduce_slabs_multi", "reduce_slabs"):
            monkeypatch.setattr(ops, name, _Refuse())
        got = E.encoder_backward(L, cx, g, _Refuse(), want_dx=True, want_param_grads=False)
    assert torch.equal(got, want) and float(got.abs().max()) > 0
