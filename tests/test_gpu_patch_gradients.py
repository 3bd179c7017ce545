"""GPU: patch_gradients (per-patch input gradients in batched passes) and the module path with enc.per_sample_stats, against
the oracle's batch-of-one loop -- x = patches[i:i+1].requires_grad_(); model(x, batch_mask=m[i:i+1])[1][of].backward() -- on
the CPU in fp32 and float64 (tests/helpers/patch_grad_reference.py, held to plain autograd by
tests/test_patch_gradients_host.py).

The yardstick is test_gpu_model.py::test_gradient_with_respect_to_the_input_patches', per patch: with e_ref the fp32 oracle's
error against float64 and scale the float64 gradient's largest magnitude, every element within max(1.5 e_ref, 2e-4 scale),
except around ReLU inputs the float64 run decides by less than 4e-7 of the tensor's largest value (at most 8192 elements per
such input beyond it, none beyond 5e-2 scale).  Codes first: conftest.codes_gate must accept every difference between the
device's codes and the oracle's; a patch that holds one is evaluated with the device's codes (OracleVQ.force_idx).  Over a
test's patches at most one patch may need that, and a patch may have at most one fragile ReLU input.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from conftest import codes_gate, grad_gate

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import patch_grad_reference as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HPARAMS = dict(commitment_cost=0.4, weight_recon=0.7, weight_commitment=1.3)       # tests/helpers/hparams.py, part B


def rand_mask(N, mc, hw, seed):
    return (torch.rand(N, mc, hw, hw, generator=torch.Generator().manual_seed(seed)) > 0.3).float()


def golden_case(golden, kw=None):
    from oracle import vqvae_oracle as O
    kw = kw or {}
    ref = O.OracleVQVAE(**kw)
    O.load_numpy_state(ref, golden("g1_state_dict.npz"))
    return ref, kw, torch.from_numpy(golden("g2_input.npz")["x"]), torch.from_numpy(golden("g5_forward_masked.npz")["mask"])


def seeded_case(seed, N, kw, hw=128, mask_channels=None, z32=False):
    """tests/test_gpu_score.py's cases."""
    from oracle import vqvae_oracle as O
    torch.manual_seed(seed)
    ref = (O.OracleVQVAEz32 if z32 else O.OracleVQVAE)(**kw)
    x = torch.randn(N, kw.get("num_inputs", 2), hw, hw, generator=torch.Generator().manual_seed(seed + 1000))
    mask = None if mask_channels is None else rand_mask(N, mask_channels, hw, seed + 2000)
    return ref, kw, x, mask


CASES = {
    "golden-masked": (lambda g: golden_case(g), 2),
    "seed11-n6-2ch-var-masks": (lambda g: seeded_case(11, 6, dict(channel_var=np.array([0.5, 1.5])), mask_channels=2), 4),
    "64px-chain": (lambda g: seeded_case(15, 3, dict(), hw=64), 2),
    "z32-default-64px": (lambda g: seeded_case(17, 4, dict(), hw=64, z32=True), 2),
}


def hip_model(ref, kw):
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    m = (dynamorph_amd.VQ_VAE_z32 if isinstance(ref, O.OracleVQVAEz32) else dynamorph_amd.VQ_VAE)(**kw).to(DEV)
    m.load_state_dict(ref.state_dict())
    m.train(ref.training)
    return m


def device_codes(m, x):
    """The codes of the per-patch forward patch_gradients runs (the layer-by-layer encoder with per-sample statistics)."""
    from dynamorph_amd import VQ_VAE_z32
    from dynamorph_amd.patch_vae import encode_patches
    mp = copy.deepcopy(m)
    with torch.no_grad():
        if isinstance(mp, VQ_VAE_z32):
            zb, _ = encode_patches(mp, x, device=DEV, batch_size=4)
            D = mp.num_hiddens
            z = torch.from_numpy(zb).reshape(x.shape[0], D, x.shape[2] // 4, x.shape[3] // 4).to(DEV)
        else:
            mp.enc.per_sample_stats = True
            z = mp.enc(x.to(DEV))
        return mp.vq.encode_inputs(z).cpu()


def forced_codes(ref, m, x, what):
    """{patch: the device's codes} for the patches whose codes differ from the oracle's (after codes_gate admitted them)."""
    with torch.no_grad():
        z_r = torch.cat([copy.deepcopy(ref).enc(x[i:i + 1]) for i in range(x.shape[0])], 0)
        idx_r = ref.vq.encode_inputs(z_r)
    idx_d = device_codes(m, x)
    flips = idx_d != idx_r
    codes_gate(flips, z_r, ref.vq.w.weight.detach(), what)
    flipped = np.nonzero(flips.reshape(x.shape[0], -1).any(1).numpy())[0]
    assert len(flipped) <= 1, f"{what}: {len(flipped)} patches hold a flipped code"
    return {int(i): idx_d[i:i + 1].clone() for i in flipped}


def check_against_oracle(ref, got, x, mask, of, force, what):
    g32, _ = P.oracle_patch_gradients(ref, x, mask, of, torch.float32, force)
    g64, fragile = P.oracle_patch_gradients(ref, x, mask, of, torch.float64, force, count_fragile=True)
    assert got.shape == tuple(x.shape) and got.dtype == np.float32
    for i in range(x.shape[0]):
        assert fragile[i] <= 1, (what, i, int(fragile[i]))
        P.yardstick(got[i], g32[i], g64[i], fragile[i], f"{what} patch {i}")
    return g32, g64


@pytest.mark.parametrize("name", list(CASES))
def test_total_loss_gradients_against_the_oracle_loop(name, golden):
    from dynamorph_amd.patch_vae import patch_gradients
    make, bs = CASES[name]
    ref, kw, x, mask = make(golden)
    m = hip_model(ref, kw)
    force = forced_codes(ref, m, x, name)
    got = patch_gradients(m, x, masks=mask, of="total_loss", device=DEV, batch_size=bs)
    check_against_oracle(ref, got, x, mask, "total_loss", force, name)


def test_loss_terms_at_other_scalars_and_their_weighted_sum(golden):
    """recon_loss and commitment_loss are the dict's unweighted entries; weight_recon * d recon + weight_commitment * d commitment
    is the total_loss result.  The three are separate fp32 evaluations of the same linear backward chain, and in exact arithmetic
    the identity is exact, so what it may miss by is the fp32 rounding of the three evaluations.  The yardstick for that rounding
    is the reference's own: e_ref, the fp32 oracle's error against float64, per patch and term -- the figure is
    weight_recon e_ref(recon) + weight_commitment e_ref(commitment) + e_ref(total), about 2e-6 of the gradient's scale here."""
    from dynamorph_amd.patch_vae import patch_gradients
    ref, kw, x, mask = golden_case(golden, HPARAMS)
    m = hip_model(ref, kw)
    force = forced_codes(ref, m, x, "hparams")
    got = {of: patch_gradients(copy.deepcopy(m), x, masks=mask, of=of, device=DEV, batch_size=2)
           for of in ("total_loss", "recon_loss", "commitment_loss")}
    e_ref = {}
    for of, g in got.items():
        g32, g64 = check_against_oracle(ref, g, x, mask, of, force, f"hparams {of}")
        e_ref[of] = (g32.double() - g64).abs().amax((1, 2, 3)).numpy()
    comb = HPARAMS["weight_recon"] * got["recon_loss"].astype(np.float64) + HPARAMS["weight_commitment"] * got["commitment_loss"].astype(np.float64)
    for i in range(x.shape[0]):
        scale = np.abs(got["total_loss"][i]).max()
        err = np.abs(comb[i] - got["total_loss"][i]).max()
        tol = HPARAMS["weight_recon"] * e_ref["recon_loss"][i] + HPARAMS["weight_commitment"] * e_ref["commitment_loss"][i] + e_ref["total_loss"][i]
        print(f"patch {i}: weighted sum of the terms against total_loss {err:.2e}, scale {scale:.2e}; the reference's own rounding "
              f"{tol:.2e} ({tol / scale:.1e} of scale): {err / tol:.2f} of it")
        assert err <= tol, (i, err, tol, scale)


@pytest.mark.parametrize("name", ["golden-masked", "64px-chain"])
@pytest.mark.parametrize("per_patch", [False, True])
def test_latent_cotangents(name, per_patch, golden):
    """of = an array on z_before: the encoder alone, no codes involved, so every patch is held."""
    from dynamorph_amd.patch_vae import patch_gradients
    ref, kw, x, _ = CASES[name][0](golden)
    N = x.shape[0]
    n = 16 * (x.shape[2] // 8) * (x.shape[3] // 8)
    w = torch.randn((N, n) if per_patch else (n,), generator=torch.Generator().manual_seed(70))
    w = w / w.norm(dim=-1, keepdim=True)
    m = hip_model(ref, kw)
    before = copy.deepcopy(m.state_dict())
    got = patch_gradients(m, x, of=w.numpy(), device=DEV, batch_size=2)
    check_against_oracle(ref, got, x, None, w, None, f"{name} cotangent {'per patch' if per_patch else 'shared'}")
    assert int(m.state_dict()["enc.2.num_batches_tracked"]) == int(before["enc.2.num_batches_tracked"]) + N


def _bit_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("hw", [128, 64])
def test_batch_size_and_position_do_not_change_a_bit(hw):
    import dynamorph_amd
    from dynamorph_amd.patch_vae import patch_gradients
    torch.manual_seed(40)
    m = dynamorph_amd.VQ_VAE(weight_recon=0.7, weight_commitment=1.3).to(DEV)
    x = torch.randn(11, 2, hw, hw, generator=torch.Generator().manual_seed(41))
    mask = rand_mask(11, 1, hw, 42)
    outs = [patch_gradients(copy.deepcopy(m), x, masks=mask, device=DEV, batch_size=bs) for bs in (1, 3, 4, 11)]
    for o in outs[1:]:
        assert _bit_equal(o, outs[0])
    perm = torch.randperm(11, generator=torch.Generator().manual_seed(43))
    o = patch_gradients(copy.deepcopy(m), x[perm], masks=mask[perm], device=DEV, batch_size=4)
    assert _bit_equal(o, outs[0][perm.numpy()])
    assert float(np.abs(outs[0]).max()) > 0


def test_eval_mode_against_the_oracle_loop(golden):
    from dynamorph_amd.patch_vae import patch_gradients
    ref, kw, x, mask = seeded_case(19, 3, dict())
    with torch.no_grad():
        ref(x)                              # running statistics away from their initial values
    ref.eval()
    m = hip_model(ref, kw)
    before = copy.deepcopy(m.state_dict())
    force = forced_codes(ref, m, x, "eval mode")
    got = patch_gradients(m, x, device=DEV, batch_size=2)
    check_against_oracle(ref, got, x, None, "total_loss", force, "eval mode")
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("name", ["golden-masked", "64px-chain", "z32-default-64px"])
def test_parameters_stay_and_running_statistics_advance_as_under_score_patches(name, golden):
    from dynamorph_amd.patch_vae import patch_gradients, score_patches
    ref, kw, x, mask = CASES[name][0](golden)
    m = hip_model(ref, kw)
    for i, p in enumerate(m.parameters()):
        if p.requires_grad:
            p.grad = torch.randn(p.shape, generator=torch.Generator().manual_seed(i)).to(DEV)
    m_score = copy.deepcopy(m)
    params = {k: (p.detach().clone(), None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}
    patch_gradients(m, x, masks=mask, device=DEV, batch_size=2)
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), params[k][0]), k
        assert (p.grad is None) == (params[k][1] is None) and (p.grad is None or torch.equal(p.grad, params[k][1])), k
    score_patches(m_score, x, masks=mask, device=DEV, batch_size=2)
    nbn = 0
    for (k, a), (_, b) in zip(m.named_buffers(), m_score.named_buffers()):
        assert torch.equal(a, b), k
        if "tracked" in k:
            nbn += 1
            assert int(a) == x.shape[0], k
    assert nbn in (8, 11)


def test_sharded_in_one_process_equals_patch_gradients():
    import dynamorph_amd
    from dynamorph_amd.patch_vae import patch_gradients, patch_gradients_sharded
    torch.manual_seed(50)
    m = dynamorph_amd.VQ_VAE().to(DEV)
    x = torch.randn(5, 2, 128, 128, generator=torch.Generator().manual_seed(51))
    w = torch.randn(5, 4096, generator=torch.Generator().manual_seed(52))
    for of in ("total_loss", w.numpy()):
        a = patch_gradients(copy.deepcopy(m), x, of=of, device=DEV, batch_size=2)
        b = patch_gradients_sharded(copy.deepcopy(m), x, of=of, device=DEV, batch_size=2)
        assert _bit_equal(a, b)


def test_module_path_with_per_sample_statistics(golden):
    """model.enc.per_sample_stats = True; (4 * total_loss).backward() at B = 4: the parameter gradients are the sums over the
    oracle's four batch-of-one backward passes (conftest.grad_gate, default factor and floor), and x.grad meets the yardstick
    as patch_gradients' result does; where both take the layer-by-layer kernels (64 px: 8 x 8 latents) the two are equal to the
    bit (same operands, and 2 is a power of two)."""
    from dynamorph_amd.patch_vae import patch_gradients
    ref, kw, x, mask = golden_case(golden)
    m = hip_model(ref, kw)
    force = forced_codes(ref, m, x, "module path")
    want = patch_gradients(copy.deepcopy(m), x, masks=mask, device=DEV, batch_size=4)
    m.enc.per_sample_stats = True
    xd = x.to(DEV).requires_grad_(True)
    _, ld = m(xd, batch_mask=mask.to(DEV))
    (4 * ld["total_loss"]).backward()
    sums = {}
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        model = copy.deepcopy(ref).to(dtype)
        for i in range(x.shape[0]):
            model.vq.force_idx = force.get(i)
            model(x[i:i + 1].to(dtype), batch_mask=mask[i:i + 1].to(dtype))[1]["total_loss"].backward()     # .grad accumulates
        sums[tag] = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert grad_gate(m, sums["f32"], sums["f64"], what="per-sample statistics, B = 4") >= 30
    # (the driver's data-only pass takes the one-launch latent-stage kernel here, the module's full pass the chain: the two
    # agree within the yardstick, not to the bit)
    P.yardstick(want, xd.grad.cpu(), P.oracle_patch_gradients(ref, x, mask, "total_loss", torch.float64, force)[0], 1, "driver against module")
    check_against_oracle(ref, xd.grad.cpu().numpy(), x, mask, "total_loss", force, "module path x.grad")


def test_module_path_equals_the_driver_to_the_bit_on_the_chain_route():
    import dynamorph_amd
    from dynamorph_amd.patch_vae import patch_gradients
    torch.manual_seed(60)
    m = dynamorph_amd.VQ_VAE(weight_recon=0.7, weight_commitment=1.3).to(DEV)
    x = torch.randn(2, 2, 64, 64, generator=torch.Generator().manual_seed(61))
    mask = rand_mask(2, 1, 64, 62)
    want = patch_gradients(copy.deepcopy(m), x, masks=mask, device=DEV, batch_size=2)
    m.enc.per_sample_stats = True
    xd = x.to(DEV).requires_grad_(True)
    (2 * m(xd, batch_mask=mask.to(DEV))[1]["total_loss"]).backward()
    assert _bit_equal(xd.grad.cpu().numpy(), want)
