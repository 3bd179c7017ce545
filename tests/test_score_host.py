"""`not gpu`: the float64 yardstick of the per-patch scores (tests/helpers/score_reference.py) against the oracle's own
batch-of-one loop, and the host-side argument handling of score_patches / score_VAE.  With this the reference the GPU tests
(tests/test_gpu_score.py, tests/test_gpu_score_kernels.py) hold the kernels to is verified without a GPU.

Gate: 1e-6 of max(1, |value|).  The fp32 oracle sits within 1.1e-7 of its own float64 copy on these inputs, and the helper
evaluates the loss expressions in float64 on the oracle's fp32 tensors: what separates the two is the fp32 rounding of the
oracle's reductions (means over 16 384 ... 32 768 terms, relative error well below 1e-6)."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import score_reference as S  # noqa: E402

GATE = 1e-6


def hold(ref, x, mask, cc, w_recon=1.0, w_commit=1.0):
    ld, dec, z, idx = S.oracle_loop(ref, x, mask)
    got = S.score_ref(dec, x, mask, ref.channel_var.detach().reshape(-1), z, idx, ref.vq.w.weight, cc, w_recon, w_commit)
    for k in ("recon_loss", "commitment_loss", "total_loss", "perplexity"):
        err = np.abs(got[k] - ld[k]) / np.maximum(1.0, np.abs(ld[k]))
        print(f"{k}: worst error {err.max():.2e} of max(1, |value|)")
        assert err.max() <= GATE, (k, got[k], ld[k])
    # the pieces agree with each other: recon is the mean of its channels, the counts are the patch's own h * w codes
    np.testing.assert_allclose(got["recon_loss_per_channel"].mean(1), got["recon_loss"], rtol=1e-14)
    assert (got["code_counts"].sum(1) == idx[0].numel()).all()
    np.testing.assert_allclose(got["commitment_loss"], (1 + cc) * got["mse"], rtol=1e-14)
    return got


def test_helper_equals_the_oracle_loop_vqvae_golden_masked(golden, golden_threads):
    from oracle import vqvae_oracle as O
    ref = O.OracleVQVAE()
    O.load_numpy_state(ref, golden("g1_state_dict.npz"))
    x = torch.from_numpy(golden("g2_input.npz")["x"])
    mask = torch.from_numpy(golden("g5_forward_masked.npz")["mask"])
    got = hold(ref, x, mask, 0.25)
    assert got["recon_loss"].shape == (4,) and got["recon_loss_per_channel"].shape == (4, 2) and got["code_counts"].shape == (4, 64)


def test_helper_equals_the_oracle_loop_vqvae_weights_and_eval_mode(golden_threads):
    from oracle import vqvae_oracle as O
    torch.manual_seed(21)
    ref = O.OracleVQVAE(commitment_cost=0.4, weight_recon=0.7, weight_commitment=1.3, channel_var=np.array([0.5, 1.5]))
    x = torch.randn(3, 2, 64, 64, generator=torch.Generator().manual_seed(22))
    hold(ref, x, None, 0.4, 0.7, 1.3)
    ref.eval()
    hold(ref, x, (torch.rand(3, 2, 64, 64, generator=torch.Generator().manual_seed(23)) > 0.3).float(), 0.4, 0.7, 1.3)


def test_helper_equals_the_oracle_loop_z32(golden_threads):
    from oracle import vqvae_oracle as O
    torch.manual_seed(31)
    ref = O.OracleVQVAEz32()
    x = torch.randn(3, 2, 64, 64, generator=torch.Generator().manual_seed(32))
    got = hold(ref, x, None, 0.25)
    assert got["code_counts"].shape == (3, 64) and (got["code_counts"].sum(1) == 256).all()


def test_score_patches_argument_validation():
    """Raised on the host, before anything touches a device."""
    import dynamorph_amd
    from dynamorph_amd.patch_vae import score_patches
    m = dynamorph_amd.VQ_VAE()
    with pytest.raises(AssertionError, match="dimension can only be 4"):
        score_patches(m, np.zeros((2, 128, 128), np.float32))
    with pytest.raises(ValueError, match="masks must be"):
        score_patches(m, np.zeros((3, 2, 128, 128), np.float32), masks=np.ones((2, 1, 128, 128), np.float32))
    with pytest.raises(ValueError, match="masks must be"):
        score_patches(m, np.zeros((3, 2, 128, 128), np.float32), masks=np.ones((3, 3, 128, 128), np.float32))
    with pytest.raises(TypeError, match="not built on the HIP path"):
        score_patches(torch.nn.Linear(2, 2), np.zeros((3, 2, 128, 128), np.float32))
    out = score_patches(m, np.zeros((0, 2, 128, 128), np.float32), return_code_counts=True, return_decoded=True)
    assert out["recon_loss"].shape == (0,) and out["recon_loss_per_channel"].shape == (0, 2)
    assert out["code_counts"].shape == (0, 64) and out["code_counts"].dtype == np.int32
    assert out["decoded"].shape == (0, 2, 128, 128) and out["z_before"].shape == (0, 0) and out["z_after"].shape == (0, 0)
    assert set(out) == {"recon_loss", "recon_loss_per_channel", "commitment_loss", "perplexity", "total_loss", "z_before",
                        "z_after", "code_counts", "decoded"}


def test_signatures_and_exports():
    import dynamorph_amd
    from dynamorph_amd import patch_vae
    assert dynamorph_amd.score_patches is patch_vae.score_patches and "score_patches" in dynamorph_amd.__all__
    for name in ("VQ_VAE", "VQ_VAE_z16", "VQ_VAE_z32", "VectorQuantizer", "ResidualBlock"):
        assert name in dynamorph_amd.__all__
    sig = inspect.signature(patch_vae.score_patches)
    assert list(sig.parameters) == ["model", "patches", "masks", "device", "batch_size", "zscore_on_device", "return_decoded",
                                    "return_code_counts"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, "cuda:0", 1024, False, False, False]
    sig = inspect.signature(patch_vae.score_VAE)
    assert list(sig.parameters) == ["raw_folder", "supp_folder", "sites", "config_", "gpu", "kwargs"]
    assert sig.parameters["gpu"].default == 0 and sig.parameters["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    sh = inspect.signature(patch_vae.score_patches_sharded)
    assert list(sh.parameters)[-2:] == ["group", "dst"]


def test_a_route_without_per_sample_statistics_is_an_error_that_names_it():
    """engine never falls back to batch statistics: slabs that are not grouped by sample raise, naming the route."""
    from dynamorph_amd import engine as E
    E._need_per_sample_slabs(torch.zeros(6, 4, 2, dtype=torch.float64), 3, "residual_forward: 3x3 convolution")
    with pytest.raises(NotImplementedError, match="z32_tail_forward: dec.1 .* no per-sample statistics"):
        E._need_per_sample_slabs(torch.zeros(5, 4, 2, dtype=torch.float64), 2, "z32_tail_forward: dec.1 (ConvTranspose2d 64 -> 32 at 16 x 16)")
    with pytest.raises(NotImplementedError, match="residual_forward"):
        E._need_per_sample_slabs(None, 2, "residual_forward: 1x1 convolution")
