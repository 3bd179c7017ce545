"""GPU: the kernels of the EMA codebook mode on their own, against the float64 restatement of
tests/helpers/ema_reference.py: the quantiser's backward with the update's statistics as its slab payload
(dm_vq_backward_stats) on each of its three routes, the one-launch update (dm_vq_ema_apply) and the mode's scalar launches."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ema_reference as R  # noqa: E402
import hparams as HP  # noqa: E402
from conftest import loss_gate  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, K, D, H, W): the route each shape reaches (csrc/vq.hip, vq_backward_launch)
ROUTES = [
    pytest.param(2, 64, 16, 16, 16, id="mfma-8chunks"),          # fewer chunks than one workgroup has waves
    pytest.param(3, 64, 16, 8, 8, id="mfma-1chunk-per-sample"),
    pytest.param(2, 40, 32, 16, 16, id="mfma-K40-D32"),          # K below 64: code tiles past K
    pytest.param(2, 1000, 16, 16, 16, id="lds-K1000"),           # K no multiple of 16
    pytest.param(2, 512, 64, 16, 16, id="lds-K512-D64"),         # 512 x 65 floats = 130 KB: the largest single window
    pytest.param(2, 1100, 64, 16, 16, id="lds-three-windows"),   # 1100 x 65 floats: windows of 535 codes over grid.y
    pytest.param(2, 40, 24, 6, 6, id="anywidth-D24-6x6"),        # run-time width; H W no multiple of 64
    # the remaining instantiations: the MFMA kernel without its prefetch (D = 64), the window kernel at 8 / 32 / 128
    pytest.param(2, 64, 64, 16, 16, id="mfma-D64"),
    pytest.param(3, 100, 8, 8, 8, id="lds-D8"),
    pytest.param(3, 100, 32, 8, 8, id="lds-D32"),
    pytest.param(3, 100, 128, 8, 8, id="lds-D128"),
    pytest.param(2, 64, 16, 6, 6, id="lds-K64-6x6"),             # K <= 64 but H W % 64 != 0: the window kernel
]


def _inputs(B, K, D, H, W, seed, idx=None, floor=0.0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, D, H, W, generator=g)
    if floor:
        z = torch.where(z >= 0, z + floor, z - floor)           # |z| >= floor: one missed position cannot hide in the bound
    e = torch.randn(K, D, generator=g)
    if idx is None:
        idx = torch.randint(0, K, (B, H, W), generator=g)
    g_out = torch.randn(B, D, H, W, generator=g)
    return z, e, idx, g_out


def _check(B, K, D, H, W, z, e, idx, g_out, cc=0.25):
    from dynamorph_amd import ops
    zd, ed, id_, gd = z.to(DEV), e.to(DEV), idx.to(DEV), g_out.to(DEV)
    g_loss = torch.full((1,), 0.7, device=DEV)
    dz_ref, _ = ops.vq_backward_slabs(zd, ed, id_, gd, g_loss, cc)
    dz, slabs = ops.vq_backward_stats(zd, ed, id_, gd, g_loss, cc)
    dz2, slabs2 = ops.vq_backward_stats(zd, ed, id_, gd, g_loss, cc)
    assert slabs.shape[1] == K * (D + 1)
    stats = ops.reduce_slabs(slabs, torch.empty(K * (D + 1), device=DEV))
    torch.cuda.synchronize()
    # dz: the bits of the gradient form; a second launch: equal bits everywhere
    assert torch.equal(dz, dz_ref)
    assert torch.equal(dz, dz2) and torch.equal(slabs, slabs2)
    n64, s64 = R.ema_statistics_f64(z.numpy(), idx.numpy(), K)
    got = stats.cpu().double().numpy()
    s, n = got[:K * D].reshape(K, D), got[K * D:]
    assert np.array_equal(n, np.bincount(idx.numpy().reshape(-1), minlength=K).astype(np.float64))
    assert np.array_equal(n, n64)
    # |s - s64| <= n_k 2^-24 sum |z|: the first-order bound of ANY fp32 summation order (nothing measured)
    zf = np.abs(z.double().numpy()).transpose(0, 2, 3, 1).reshape(-1, D)
    onehot = np.zeros((idx.numel(), K))
    onehot[np.arange(idx.numel()), idx.numpy().reshape(-1)] = 1.0
    bound = n64[:, None] * 2.0 ** -24 * (onehot.T @ zf)
    err = np.abs(s - s64)
    print(f"stats {B}x{K}x{D}x{H}x{W}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, "
          f"codes used {int((n64 > 0).sum())} of {K}")
    assert np.all(err <= bound), float(np.max(err - bound))
    # statistics alone (no dz, no upstream gradient): the same slabs
    none, slabs3 = ops.vq_backward_stats(zd, ed, id_, None, None, cc, want_dz=False)
    assert none is None and torch.equal(slabs3, slabs)


@pytest.mark.parametrize("B,K,D,H,W", ROUTES)
def test_backward_stats_on_every_route(B, K, D, H, W):
    z, e, idx, g_out = _inputs(B, K, D, H, W, seed=100 + K + D)
    _check(B, K, D, H, W, z, e, idx, g_out)


@pytest.mark.parametrize("kind", ["one-code", "half-unused"])
def test_backward_stats_constructed_index_maps(kind):
    B, K, D, H, W = 2, 64, 16, 16, 16
    if kind == "one-code":
        idx = torch.full((B, H, W), 37, dtype=torch.int64)
    else:
        idx = 2 * torch.randint(0, K // 2, (B, H, W), generator=torch.Generator().manual_seed(5))      # odd codes never used
    z, e, idx, g_out = _inputs(B, K, D, H, W, seed=7, idx=idx, floor=0.25)
    assert float(z.abs().min()) >= 0.25
    _check(B, K, D, H, W, z, e, idx, g_out)


def _ulp_distance(a, b):
    """Distance in units of the last place between two float32 arrays (same-sign or zero values)."""
    ia = a.view(np.int32).astype(np.int64)
    ib = b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 31) - ib, ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("K,D", [(64, 16), (1000, 16), (40, 24)])
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.99])
@pytest.mark.parametrize("eps", [0.0, 1e-5])
@pytest.mark.parametrize("case", ["random", "zero-counts", "one-code"])
def test_ema_apply_within_one_ulp_of_float64(K, D, decay, eps, case):
    from dynamorph_amd import ops
    g = torch.Generator().manual_seed(K + D)
    P = 4096
    if case == "random":
        n = torch.bincount(torch.randint(0, K, (P,), generator=g), minlength=K).float()
    elif case == "zero-counts":
        n = torch.bincount(2 * torch.randint(0, K // 2, (P,), generator=g), minlength=K).float()      # odd codes: zero
    else:
        n = torch.zeros(K)
        n[K // 3] = P
    s = torch.randn(K, D, generator=g) * n[:, None]
    N = torch.rand(K, generator=g) * 20.0 + 0.5
    m = torch.randn(K, D, generator=g) * N[:, None]
    e = torch.randn(K, D, generator=g)
    stats = torch.cat([s.reshape(-1), n]).to(DEV)
    Nd, md, ed = N.to(DEV), m.to(DEV), e.to(DEV)
    ops.vq_ema_apply(stats, Nd, md, ed, decay, eps)
    torch.cuda.synchronize()
    N2, m2, e2 = R.ema_apply_f64(n.numpy(), s.numpy(), N.numpy(), m.numpy(), decay, eps)
    for name, got, want in (("N", Nd, N2), ("m", md, m2), ("e", ed, e2)):
        got = got.cpu().numpy()
        want32 = want.astype(np.float32)
        nan = np.isnan(want32)
        # 0 / 0 by the definition, and only there: decay = 0 and epsilon = 0 leave a code without positions N = m = 0
        empty = (n.numpy() == 0) if (decay == 0.0 and eps == 0.0 and name == "e") else np.zeros(K, bool)
        assert np.array_equal(nan, np.broadcast_to(empty[:, None] if want32.ndim == 2 else empty, want32.shape)), name
        assert np.array_equal(np.isnan(got), nan), name
        assert np.array_equal(np.isinf(got), np.isinf(want32)), name
        ok = ~nan & ~np.isinf(want32)
        d = _ulp_distance(got[ok], want32[ok])
        assert d.max() <= 1, (name, int(d.max()))


@pytest.mark.parametrize("cc", HP.C_CCS + (0.25, 0.4))
def test_scalars_in_ema_mode(cc):
    """commitment = cc * mse from both scalar launches (the module's dm_vq_finalize_ema and the step's
    dm_vq_loss_finalize_ema, without and with the pairwise term), against float64; perplexity and mse are the other mode's."""
    from dynamorph_amd import ops
    B, K, D, H, W = 4, 64, 16, 16, 16
    g = torch.Generator().manual_seed(11)
    z = torch.randn(B, D, H, W, generator=g).to(DEV)
    e = torch.randn(K, D, generator=g).to(DEV)
    idx, out, slabs, hist = ops.vq_forward(z, e)
    ref = ops.vq_finalize(slabs, hist, B * H * W, D, cc)
    got = ops.vq_finalize(slabs, hist, B * H * W, D, cc, ema=True)
    q = e.double()[idx].permute(0, 3, 1, 2)
    mse = float(((q - z.double()) ** 2).mean())
    loss_gate(got[0], cc * mse, f"ema vq_finalize cc={cc}")
    assert torch.equal(got[1:], ref[1:])
    loss_gate(ref[0], mse + cc * mse, f"vq_finalize cc={cc}")
    # the step's launch: the counters stay in the workspace
    idx2, _, slabs2, ws = ops.vq_forward(z, e, want_hist=False)
    loss_slabs = torch.tensor([3.0, 5.0], dtype=torch.float64, device=DEV)
    count, wr, wc = 16, 0.7, 1.3
    fin = (slabs2, ws, K, D, B * H * W, cc, loss_slabs, count, wr, wc)
    a, b = ops.vq_loss_finalize(*fin), ops.vq_loss_finalize(*fin, ema=True)
    recon = 8.0 / count
    loss_gate(b[0], recon, "ema recon")
    loss_gate(b[1], cc * mse, f"ema vq_loss_finalize cc={cc}")
    loss_gate(b[2], wr * recon + wc * cc * mse, f"ema total cc={cc}")
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
    loss_gate(a[1], mse + cc * mse, f"vq_loss_finalize cc={cc}")
    tm_slabs = torch.tensor([[0.25, 0.0], [0.5, 0.0]], dtype=torch.float64, device=DEV)
    c = ops.vq_loss_finalize_tm(*fin, tm_slabs, 3.0, ema=True)
    assert c.numel() == 5 and torch.equal(c[1], b[1])
    loss_gate(c[4], 0.75, "ema tm")
    loss_gate(c[2], wr * recon + wc * cc * mse + 3.0 * 0.75, f"ema total with tm cc={cc}")
    # per patch (score_patches)
    sc, _ = ops.vq_patch_scalars(z, idx, e, cc, ema=True)
    sc0, _ = ops.vq_patch_scalars(z, idx, e, cc)
    mse_b = ((q - z.double()) ** 2).mean(dim=(1, 2, 3)).cpu().numpy()
    for i in range(B):
        loss_gate(sc[i, 0], cc * mse_b[i], f"ema patch scalars cc={cc}")
    assert torch.equal(sc[:, 1:], sc0[:, 1:])
