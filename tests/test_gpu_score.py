"""GPU: score_patches (per-patch losses and code usage in batched passes) against the oracle's batch-of-one loop -- the
reference's `model(x[i:i+1], batch_mask=m[i:i+1])` -- through the float64 helper tests/helpers/score_reference.py (held to
that loop on the host by tests/test_score_host.py).

Code flips.  The HIP encoder accumulates in another order than oneDNN, so a code may differ from the reference's where the
reference's own two best distances are within 1e-4 of each other (conftest.codes_gate admits nothing else).  A patch that
holds such a code is left out of the commitment / total / perplexity / counts comparison ONLY; its reconstruction loss is
still held, against the oracle evaluated with the device's own codes (OracleVQ.force_idx).  At most one patch per case may
be left out: on these inputs the reference has 0 or 1 near-ties per case."""
import copy
import os
import pickle
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import codes_gate, loss_gate

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import score_reference as S  # noqa: E402
from hparams import B_KW  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rand_mask(N, mc, hw, seed):
    return (torch.rand(N, mc, hw, hw, generator=torch.Generator().manual_seed(seed)) > 0.3).float()


def golden_case(golden):
    from oracle import vqvae_oracle as O
    ref = O.OracleVQVAE()
    O.load_numpy_state(ref, golden("g1_state_dict.npz"))
    return ref, {}, torch.from_numpy(golden("g2_input.npz")["x"]), torch.from_numpy(golden("g5_forward_masked.npz")["mask"])


def seeded_case(seed, N, kw, hw=128, mask_channels=None, z32=False):
    from oracle import vqvae_oracle as O
    torch.manual_seed(seed)
    ref = (O.OracleVQVAEz32 if z32 else O.OracleVQVAE)(**kw)
    nin = kw.get("num_inputs", 2)
    x = torch.randn(N, nin, hw, hw, generator=torch.Generator().manual_seed(seed + 1000))
    mask = None if mask_channels is None else rand_mask(N, mask_channels, hw, seed + 2000)
    return ref, kw, x, mask


CASES = {
    "golden-masked": lambda g: golden_case(g),
    "seed11-n6-2ch-var-masks": lambda g: seeded_case(11, 6, dict(channel_var=np.array([0.5, 1.5])), mask_channels=2),
    "seed12-n5-1ch": lambda g: seeded_case(12, 5, dict(num_inputs=1, channel_var=np.ones(1))),
    "seed13-n3-4ch": lambda g: seeded_case(13, 3, dict(num_inputs=4, channel_var=np.ones(4)), mask_channels=1),
    "nh32-unfused-tail": lambda g: seeded_case(14, 3, dict(num_hiddens=32)),
    "64px-wide-tiling": lambda g: seeded_case(15, 3, dict(), hw=64),
    "hparams": lambda g: seeded_case(16, 3, dict(B_KW)),
    "z32-default-64px": lambda g: seeded_case(17, 4, dict(), hw=64, z32=True),
    "z32-64-64-512-64px": lambda g: seeded_case(18, 2, dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512), hw=64,
                                                z32=True, mask_channels=1),
    "eval-mode": lambda g: seeded_case(19, 3, dict()),
}


def hip_model(ref, kw, z32):
    import dynamorph_amd
    m = (dynamorph_amd.VQ_VAE_z32 if z32 else dynamorph_amd.VQ_VAE)(**kw).to(DEV)
    m.load_state_dict(ref.state_dict())
    return m


@pytest.mark.parametrize("name", list(CASES))
def test_score_patches_against_the_oracle_loop(name, golden, golden_threads):
    from dynamorph_amd.patch_vae import encode_patches, score_patches
    from oracle import vqvae_oracle as O
    ref, kw, x, mask = CASES[name](golden)
    z32 = isinstance(ref, O.OracleVQVAEz32)
    N, C = x.shape[:2]
    if name == "eval-mode":
        with torch.no_grad():
            ref(x)                          # running statistics away from their initial values
        ref.eval()
    m = hip_model(ref, kw, z32)
    m.train(ref.training)
    m_enc = copy.deepcopy(m)
    ref0 = copy.deepcopy(ref)
    cc = float(ref.vq.commitment_cost)
    w_r, w_c = (1.0, 1.0) if z32 else (float(ref.weight_recon), float(ref.weight_commitment))
    var = ref.channel_var.detach().reshape(-1)
    cb = ref.vq.w.weight.detach()

    out = score_patches(m, x, masks=mask, device=DEV, batch_size=4, return_decoded=True, return_code_counts=True)
    zb, za = encode_patches(m_enc, x, device=DEV, batch_size=4)
    assert np.array_equal(out["z_before"], zb) and np.array_equal(out["z_after"], za)
    assert out["recon_loss"].shape == (N,) and out["recon_loss_per_channel"].shape == (N, C)
    assert out["code_counts"].shape == (N, cb.shape[0]) and out["code_counts"].dtype == np.int32
    assert out["decoded"].shape == tuple(x.shape)

    ld, dec_r, z_r, idx_r = S.oracle_loop(ref, x, mask)
    zshape = tuple(z_r.shape)
    idx_d = m.vq.encode_inputs(torch.from_numpy(zb).reshape(zshape).to(DEV)).cpu()
    flips = idx_d != idx_r
    codes_gate(flips, z_r, cb, name)
    flipped = flips.reshape(N, -1).any(1).numpy()
    assert flipped.sum() <= 1, f"{int(flipped.sum())} patches hold a flipped code"
    for i in np.nonzero(flipped)[0]:        # the oracle on the device's own codes, for this patch's reconstruction loss
        twin = copy.deepcopy(ref0)
        twin.vq.force_idx = idx_d[i:i + 1]
        with torch.no_grad():
            dec_r[i:i + 1] = twin(x[i:i + 1], batch_mask=None if mask is None else mask[i:i + 1])[0]
    want = S.score_ref(dec_r, x, mask, var, z_r, idx_r, cb, cc, w_r, w_c)
    for i in range(N):
        loss_gate(out["recon_loss"][i], want["recon_loss"][i], f"{name} recon[{i}]")
        for c in range(C):
            loss_gate(out["recon_loss_per_channel"][i, c], want["recon_loss_per_channel"][i, c], f"{name} recon[{i}, ch {c}]")
        if flipped[i]:
            continue
        loss_gate(out["commitment_loss"][i], want["commitment_loss"][i], f"{name} commitment[{i}]")
        loss_gate(out["total_loss"][i], want["total_loss"][i], f"{name} total[{i}]")
        assert abs(out["perplexity"][i] - want["perplexity"][i]) <= 1e-4 * want["perplexity"][i], (i, out["perplexity"][i])
        assert np.array_equal(out["code_counts"][i], want["code_counts"][i]), i
    # the device's counts are its own codes' histogram on every patch, flipped or not
    assert np.array_equal(out["code_counts"], np.stack([np.bincount(idx_d[i].reshape(-1).numpy(), minlength=cb.shape[0]) for i in range(N)]))
    # running statistics: N batch-of-one calls in train mode, untouched in eval mode
    sd, sd_r = m.state_dict(), ref.state_dict()
    nbn = 0
    for k in sd:
        if "running" in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), sd_r[k].numpy(), rtol=1e-4, atol=1e-6, err_msg=k)
        if "tracked" in k:
            nbn += 1
            assert int(sd[k]) == int(sd_r[k]) == (N if ref.training else 1), k
    assert nbn == (11 if z32 else 8)


def test_batch_size_does_not_change_a_bit():
    from dynamorph_amd.patch_vae import score_patches
    import dynamorph_amd
    torch.manual_seed(40)
    m = dynamorph_amd.VQ_VAE().to(DEV)
    x = torch.randn(23, 2, 128, 128, generator=torch.Generator().manual_seed(41))
    mask = rand_mask(23, 1, 128, 42)
    outs = [score_patches(copy.deepcopy(m), x, masks=mask, device=DEV, batch_size=bs, return_decoded=True, return_code_counts=True)
            for bs in (1, 8, 23)]
    for o in outs[1:]:
        assert sorted(o) == sorted(outs[0])
        for k in o:
            assert o[k].dtype == outs[0][k].dtype and np.array_equal(o[k].view(np.int32), outs[0][k].view(np.int32)), k
    # ... nor does a patch's position or its neighbours
    perm = torch.randperm(23, generator=torch.Generator().manual_seed(43))
    o = score_patches(copy.deepcopy(m), x[perm], masks=mask[perm], device=DEV, batch_size=8, return_code_counts=True)
    for k in o:
        assert np.array_equal(o[k].view(np.int32), outs[0][k][perm.numpy()].view(np.int32)), k


def test_return_decoded_agrees_with_the_batch_of_one_model_call(golden):
    """save_recon_samples' route: model(sample)[0] on one patch at a time (batch statistics of a batch of one).  Another
    kernel route through the encoder (layer by layer instead of the fused latent tail): 5e-4, the gate
    test_process_vae_pickle_contract holds that route's output to."""
    from dynamorph_amd.patch_vae import score_patches
    ref, kw, x, mask = golden_case(golden)
    m = hip_model(ref, kw, False)
    out = score_patches(copy.deepcopy(m), x, masks=mask, device=DEV, return_decoded=True)
    for i in range(x.shape[0]):
        with torch.no_grad():
            dec, ld = copy.deepcopy(m)(x[i:i + 1].to(DEV), batch_mask=mask[i:i + 1].to(DEV))
        assert np.abs(out["decoded"][i] - dec[0].cpu().numpy()).max() < 5e-4
        loss_gate(out["recon_loss"][i], float(ld["recon_loss"]), f"model(sample) recon[{i}]")
        loss_gate(out["commitment_loss"][i], float(ld["commitment_loss"]), f"model(sample) commitment[{i}]")


def test_sharded_in_one_process_equals_score_patches():
    from dynamorph_amd.patch_vae import score_patches, score_patches_sharded
    import dynamorph_amd
    torch.manual_seed(50)
    m = dynamorph_amd.VQ_VAE().to(DEV)
    x = torch.randn(5, 2, 128, 128, generator=torch.Generator().manual_seed(51))
    a = score_patches(copy.deepcopy(m), x, device=DEV, batch_size=2, return_code_counts=True)
    b = score_patches_sharded(copy.deepcopy(m), x, device=DEV, batch_size=2, return_code_counts=True)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_score_vae_round_trips_its_pickle(tmp_path, golden):
    from dynamorph_amd.patch_vae import score_VAE, score_patches
    from dynamorph_amd.train_utils import zscore_patch
    import dynamorph_amd
    raw, wdir = tmp_path / "raw", tmp_path / "weights" / "vqvae_test"
    raw.mkdir(), wdir.mkdir(parents=True)
    rng = np.random.RandomState(0)
    patches = rng.rand(5, 2, 1, 128, 128) * 1000 + 200        # (N,C,1,H,W) float64 as extract_patches writes them
    masks = (rng.rand(5, 1, 1, 128, 128) > 0.2).astype(np.float64)
    with open(raw / "C5_file_paths.pkl", "wb") as f:
        pickle.dump([f"/data/C5-Site_0/{i}_0.h5" for i in range(5)], f)
    with open(raw / "C5_static_patches.pkl", "wb") as f:
        pickle.dump(patches, f)
    with open(raw / "C5_static_patches_mask.pkl", "wb") as f:
        pickle.dump(masks, f)
    sd = {k: torch.from_numpy(v) for k, v in golden("g1_state_dict.npz").items()}
    torch.save(sd, wdir / "model.pt")
    cfg = SimpleNamespace(latent_encoding=SimpleNamespace(
        weights=str(wdir), channels=[0, 1], num_hiddens=16, num_residual_hiddens=32, num_embeddings=64,
        commitment_cost=0.25, network="VQ_VAE_z16", save_output=False, channel_mean=None, channel_std=None))
    got = score_VAE(str(raw), None, ["C5-Site_0"], cfg, gpu=0, batch_size=2, use_mask=True, return_code_counts=True)
    with open(raw / "vqvae_test" / "C5_patch_scores.pkl", "rb") as f:
        disk = pickle.load(f)
    assert sorted(disk) == sorted(got) == sorted(["recon_loss", "recon_loss_per_channel", "commitment_loss", "perplexity",
                                                   "total_loss", "z_before", "z_after", "code_counts"])
    m = dynamorph_amd.VQ_VAE_z16().to(DEV)
    m.load_state_dict(sd)
    want = score_patches(m, torch.from_numpy(zscore_patch(np.squeeze(patches))).float(), device=DEV,
                         masks=torch.from_numpy(masks.reshape(5, 1, 128, 128)).float(), return_code_counts=True)
    for k in want:
        assert isinstance(disk[k], np.ndarray) and np.array_equal(disk[k], want[k]) and np.array_equal(got[k], want[k]), k
    assert disk["recon_loss"].shape == (5,) and disk["z_before"].shape == (5, 4096)
