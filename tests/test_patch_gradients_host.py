"""Host: the reference loop of patch_gradients (tests/helpers/patch_grad_reference.py) against plain autograd on the
oracle, patch_gradients' argument errors and its N = 0 return, and the new entry points' argument errors -- no device."""
import copy
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import patch_grad_reference as P  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    return _lib.load()


def _oracle(z32=False, seed=3):
    from oracle import vqvae_oracle as O
    torch.manual_seed(seed)
    return (O.OracleVQVAEz32 if z32 else O.OracleVQVAE)()


@pytest.mark.parametrize("z32", [False, True])
@pytest.mark.parametrize("of", ["total_loss", "recon_loss", "commitment_loss"])
def test_loop_is_the_batch_of_one_call(z32, of):
    """Patch i of the loop is the plain call on patches[i:i+1], to the bit, whatever the other patches are; the loop leaves
    the model it is handed as it was."""
    ref = _oracle(z32)
    x = torch.randn(3, 2, 64, 64, generator=torch.Generator().manual_seed(4))
    mask = (torch.rand(3, 1, 64, 64, generator=torch.Generator().manual_seed(5)) > 0.3).float()
    before = copy.deepcopy(ref.state_dict())
    got, fragile = P.oracle_patch_gradients(ref, x, mask, of, count_fragile=True)
    assert got.shape == x.shape and fragile.shape == (3,)
    for k, v in ref.state_dict().items():
        assert torch.equal(v, before[k]), k
    for i in (0, 2):
        xi = x[i:i + 1].clone().requires_grad_(True)
        copy.deepcopy(ref)(xi, batch_mask=mask[i:i + 1])[1][of].backward()
        assert torch.equal(got[i], xi.grad[0])


def test_loop_in_eval_mode_is_the_batched_gradient():
    """With running statistics the patches of a batch are independent and every loss is a mean over equal-sized patches, so the
    gradient of N x the batched loss is every patch's own gradient: an independent statement of what the loop computes."""
    ref = _oracle()
    x = torch.randn(4, 2, 64, 64, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        ref(x)
    ref.eval()
    for of in ("total_loss", "recon_loss", "commitment_loss"):
        got, _ = P.oracle_patch_gradients(ref, x, None, of, torch.float64)
        xb = x.double().requires_grad_(True)
        (4 * copy.deepcopy(ref).double()(xb)[1][of]).backward()
        assert float((got - xb.grad).abs().max()) <= 1e-12 * float(xb.grad.abs().max()), of


def test_loop_cotangent_forms_and_forced_codes():
    ref = _oracle()
    x = torch.randn(2, 2, 64, 64, generator=torch.Generator().manual_seed(7))
    w = torch.randn(2, 1024, generator=torch.Generator().manual_seed(8))
    shared, _ = P.oracle_patch_gradients(ref, x, None, w[0].numpy())
    per, _ = P.oracle_patch_gradients(ref, x, None, w.numpy())
    assert torch.equal(shared[0], per[0]) and not torch.equal(shared[1], per[1])
    xi = x[1:2].clone().requires_grad_(True)
    (w[1] * copy.deepcopy(ref).enc(xi).reshape(-1)).sum().backward()
    assert torch.equal(per[1], xi.grad[0])
    # forced codes change the patch they are given for, and only that one
    plain, _ = P.oracle_patch_gradients(ref, x, None, "total_loss")
    idx = torch.zeros(1, 8, 8, dtype=torch.int64)
    forced, _ = P.oracle_patch_gradients(ref, x, None, "total_loss", force_idx={1: idx})
    assert torch.equal(plain[0], forced[0]) and not torch.equal(plain[1], forced[1])


def test_yardstick_counts_and_refuses():
    g64 = torch.randn(2, 8, 8, generator=torch.Generator().manual_seed(9)).double()
    g32 = g64.float()
    P.yardstick(g32, g32, g64, 0)
    bad = g32.clone()
    bad[0, 0, 0] += 1e-2 * g64.abs().max().float()
    with pytest.raises(AssertionError):
        P.yardstick(bad, g32, g64, 0)
    P.yardstick(bad, g32, g64, 1)                 # one fragile input admits it ...
    bad[0, 0, 0] += g64.abs().max().float()
    with pytest.raises(AssertionError):
        P.yardstick(bad, g32, g64, 1)             # ... but nothing beyond 5e-2 of the scale


def test_patch_gradients_argument_validation():
    """Raised on the host, before anything touches a device; N = 0 returns an empty array."""
    import dynamorph_amd
    from dynamorph_amd.patch_vae import patch_gradients
    m = dynamorph_amd.VQ_VAE()
    x = np.zeros((3, 2, 128, 128), np.float32)
    with pytest.raises(AssertionError, match="dimension can only be 4"):
        patch_gradients(m, np.zeros((2, 128, 128), np.float32))
    with pytest.raises(ValueError, match="masks must be"):
        patch_gradients(m, x, masks=np.ones((2, 1, 128, 128), np.float32))
    with pytest.raises(ValueError, match="masks must be"):
        patch_gradients(m, x, masks=np.ones((3, 3, 128, 128), np.float32))
    with pytest.raises(TypeError, match="not built on the HIP path"):
        patch_gradients(torch.nn.Linear(2, 2), x)
    with pytest.raises(ValueError, match="of must be one of"):
        patch_gradients(m, x, of="perplexity")
    with pytest.raises(ValueError, match="cotangent on z_before must be"):
        patch_gradients(m, x, of=np.zeros(4095, np.float32))
    with pytest.raises(ValueError, match="cotangent on z_before must be"):
        patch_gradients(m, x, of=np.zeros((2, 4096), np.float32))
    with pytest.raises(ValueError, match="cotangent on z_before must be"):
        patch_gradients(dynamorph_amd.VQ_VAE_z32(), np.zeros((3, 2, 64, 64), np.float32), of=np.zeros(1024, np.float32))   # 16 x 16 x 16 there
    for of in ("total_loss", np.zeros(4096, np.float32), np.zeros((0, 4096), np.float32)):
        out = patch_gradients(m, np.zeros((0, 2, 128, 128), np.float32), of=of)
        assert out.shape == (0, 2, 128, 128) and out.dtype == np.float32


def test_signatures_and_exports():
    import dynamorph_amd
    from dynamorph_amd import patch_vae
    assert dynamorph_amd.patch_gradients is patch_vae.patch_gradients and "patch_gradients" in dynamorph_amd.__all__
    assert dynamorph_amd.patch_gradients_sharded is patch_vae.patch_gradients_sharded and "patch_gradients_sharded" in dynamorph_amd.__all__
    sig = inspect.signature(patch_vae.patch_gradients)
    assert list(sig.parameters) == ["model", "patches", "masks", "of", "device", "batch_size", "zscore_on_device"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [None, "total_loss", "cuda:0", 1024, False]
    assert list(inspect.signature(patch_vae.patch_gradients_sharded).parameters)[-2:] == ["group", "dst"]
    from dynamorph_amd import engine as E
    for fn in (E.encoder_backward, E.residual_backward, E.z32_stem_backward, E.z32_tail_backward, E.z32_encoder_backward,
               E.z32_decoder_backward):
        assert inspect.signature(fn).parameters["want_param_grads"].default is True


def test_power_of_two_runs():
    from dynamorph_amd.patch_vae import _pow2_chunks
    assert _pow2_chunks(11) == [(0, 8), (8, 10), (10, 11)] and _pow2_chunks(1024) == [(0, 1024)] and _pow2_chunks(1) == [(0, 1)]
    for n in range(1, 70):
        ch = _pow2_chunks(n)
        assert ch[0][0] == 0 and ch[-1][1] == n and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all((hi - lo) & (hi - lo - 1) == 0 for lo, hi in ch)


def test_new_entry_points_report_argument_errors_before_any_launch(lib):
    """negative return + message, nothing is enqueued (no device needed)."""
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data                     # a non-NULL address; every call below returns before it would be read
    f = lib.dm_bn_backward_finalize_per_sample
    assert f(None, 8, 1, 16, 256, None, None, None, None, None, None) == -1 and b"NULL" in lib.dm_last_error()
    assert f(p, 8, 1, 16, 256, None, p, None, None, None, None) == -1 and b"NULL" in lib.dm_last_error()
    assert f(p, 8, 3, 16, 256, None, p, None, None, p, None) == -1 and b"not a multiple of slabs_per_group" in lib.dm_last_error()
    assert f(p, 8, 0, 16, 256, None, p, None, None, p, None) == -1
    assert f(p, 8, 2, 16, 0, None, p, None, None, p, None) == -1 and b"bad sizes" in lib.dm_last_error()     # eval(): the batch form
    assert f(p, 0, 1, 16, 256, None, p, None, None, p, None) == -1
    g = lib.dm_channel_stats_per_sample
    assert g(None, None, None, 2, 16, 16, 16, None) == -1 and b"NULL" in lib.dm_last_error()
    assert g(p, None, p, 0, 16, 16, 16, None) == -1 and b"bad sizes" in lib.dm_last_error()
    assert g(p, None, p, 2, 16, 3, 3, None) == -1 and b"multiple of 4" in lib.dm_last_error()
    from dynamorph_amd import _lib
    with pytest.raises(ValueError):
        _lib.check(-1, "dm_channel_stats_per_sample")
    h = lib.dm_latent_tail_backward
    assert h(None, None) == -1 and b"NULL arguments" in lib.dm_last_error()
    args = _lib.LatentTailBwdArgs()
    args.B, args.C, args.CR, args.H, args.W, args.nres = 4, 16, 32, 16, 16, 2
    assert h(ctypes.byref(args), None) == -1 and b"NULL pointer" in lib.dm_last_error()
    for k, v in (("H", 8), ("W", 32), ("C", 64), ("CR", 64), ("nres", 5)):
        bad = _lib.LatentTailBwdArgs()
        bad.B, bad.C, bad.CR, bad.H, bad.W, bad.nres = 4, 16, 32, 16, 16, 2
        setattr(bad, k, v)
        assert h(ctypes.byref(bad), None) == -1 and b"built for 16 channels" in lib.dm_last_error(), k
    for k in ("g_z", "a3", "coef3", "a4", "saved4", "w10", "dy3", "stats3"):
        setattr(args, k, p)
    assert h(ctypes.byref(args), None) == -1 and b"residual layer 0" in lib.dm_last_error()
    assert lib.dm_latent_tail_supported(16, 32, 8, 8, 2) == 0 and lib.dm_latent_tail_supported(16, 32, 32, 32, 2) == 0
