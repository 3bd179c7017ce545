"""`not gpu`: the yardsticks of tests/test_gpu_hparams.py at non-default hyper-parameters.

* The CPU oracle (oracle/vqvae_oracle.py), configured with the same scalars, reproduces the three parts of
  g12_hparams.npz captured from the reference (tests/golden/make_golden_hparams.py): the example configuration of
  VQ_VAE_z32, VQ_VAE / VQ_VAE_z16 with every loss weight away from 1, the quantiser at three commitment costs.  Gates of
  test_oracle.py::test_z32_time_matching_mask_and_gradients.
* FusedTrainer._time_matching, the trainer's torch form of the pairwise term (latent lengths the MFMA kernels do not
  tile), against the reference's expression in float64 over the (w_a, w_t, w_n, margin) grid, pairs exactly on the hinge
  included.
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import vqvae_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from hparams import (A_KW, C_CCS, TM_IDS, TM_PARAMS, check_initial_state, example_batch, example_relations,  # noqa: E402
                     oracle_model, sample, stat, tm_loss_of_sim, unpack_mask)

pytestmark = pytest.mark.usefixtures("golden_threads")


def _f(v):
    return float(v.detach()) if torch.is_tensor(v) else float(v)


def check_grad(got, g, key, rtol=2e-5, atol=2e-7):
    """A whole gradient against the fixture's strided sample of it and the statistics of the whole tensor."""
    np.testing.assert_allclose(sample(got), g[key.replace("_stat/", "/")], rtol=rtol, atol=atol, err_msg=key)
    s, r = stat(got), g[key]
    assert abs(s[0] - r[0]) <= rtol * r[1] + atol, (key, "sum", s[0], r[0])
    for i, what in ((1, "sum |.|"), (2, "sum of squares"), (3, "max |.|")):
        assert abs(s[i] - r[i]) <= 2 * rtol * r[i] + atol, (key, what, s[i], r[i])


def _check_model(m, g, prefix, x, tm, mask):
    dec, ld = m(x, time_matching_mat=tm, batch_mask=mask)
    assert np.array_equal(sample(dec), g[prefix + "decoded"])
    assert np.array_equal(stat(dec), g[prefix + "decoded_stat"])
    for k in ("recon_loss", "commitment_loss", "time_matching_loss", "total_loss", "perplexity"):
        ref = float(g[prefix + "loss/" + k])
        assert abs(_f(ld[k]) - ref) <= 2e-6 * max(1.0, abs(ref)), (prefix, k, _f(ld[k]), ref)
    ld["total_loss"].backward()
    n = 0
    for k, p in m.named_parameters():
        if p.grad is not None:
            check_grad(p.grad, g, prefix + "grad_stat/" + k)
            n += 1
    assert n == sum(1 for k in g if k.startswith(prefix + "grad_stat/"))
    return ld


def test_oracle_example_configuration(golden):
    """Part A: VQ_VAE_z32 at config_example.yml's scalars -- losses, reconstruction, every gradient, every gradient without
    the pairwise term, and the losses after one Adam step (run_training.py:485)."""
    g = golden("g12_hparams.npz")
    assert int(g["A/hinge_live"]) > 0 and int(g["A/hinge_dead"]) > 0
    x = example_batch(golden("g2_input.npz")["x"])
    assert np.array_equal(stat(x), g["A/x_stat"])
    tm, mask = example_relations(), unpack_mask(g["A/mask_bits"], (6, 1, 128, 128))
    assert torch.equal(tm, torch.from_numpy(g["A/tm"]))
    m = oracle_model("A")
    check_initial_state(m, g, "A/sd_stat/")
    m0 = O.OracleVQVAEz32(**dict(A_KW, weight_matching=0))
    m0.load_state_dict(m.state_dict())
    ld = _check_model(m, g, "A/", x, tm, mask)
    assert _f(ld["time_matching_loss"]) * A_KW["weight_matching"] > 0.25 * _f(ld["total_loss"])   # the term matters
    _, ld0 = m0(x, time_matching_mat=tm, batch_mask=mask)
    ld0["total_loss"].backward()
    n = 0
    for k, p in m0.named_parameters():
        if p.grad is not None:
            check_grad(p.grad, g, "A/grad_wm0_stat/" + k)
            n += 1
    assert n == sum(1 for k in g if k.startswith("A/grad_wm0_stat/"))
    opt = O.make_adam(m, 1e-4)
    opt.step()
    m.zero_grad()
    _, ld2 = m(x, time_matching_mat=tm, batch_mask=mask)
    for k in ("recon_loss", "commitment_loss", "time_matching_loss", "total_loss"):
        ref = float(g["A/step2/" + k])
        assert abs(_f(ld2[k]) - ref) <= 2e-6 * max(1.0, abs(ref)), (k, _f(ld2[k]), ref)


@pytest.mark.parametrize("name", ["vqvae", "z16"])
def test_oracle_weighted_losses(golden, name):
    """Part B: commitment_cost 0.4, weight_recon 0.7, weight_commitment 1.3, channel_var [0.5, 1.5], weight_matching 3 (z16:
    w_a 0.8, w_t 0.3, w_n -0.2, margin 0.7); VQ_VAE's relation block with a value of 0.5 and a one-way entry."""
    g = golden("g12_hparams.npz")
    x = torch.from_numpy(golden("g2_input.npz")["x"])
    m = oracle_model("B", name)
    check_initial_state(m, g, f"B/{name}/sd_stat/")
    _check_model(m, g, f"B/{name}/", x, torch.from_numpy(g[f"B/{name}/tm"]), unpack_mask(g["B/mask_bits"], (4, 1, 128, 128)))


@pytest.mark.parametrize("cc", C_CCS)
def test_oracle_quantiser_commitment_costs(golden, cc):
    """Part C: the quantiser alone -- output, loss, perplexity, dz and dw at commitment_cost 0, 0.1, 1."""
    g = golden("g12_hparams.npz")
    vq = O.OracleVQ(16, 64, commitment_cost=cc)
    with torch.no_grad():
        vq.w.weight.copy_(torch.from_numpy(g["C/w"]))
    z = torch.from_numpy(g["C/z"]).requires_grad_(True)
    out, loss, perp = vq(z)
    ((out * torch.from_numpy(g["C/g_out"])).sum() + float(g["C/g_loss"]) * loss).backward()
    p = f"C/cc{cc:g}/"
    assert np.array_equal(out.detach().numpy(), g[p + "out"])
    assert abs(_f(loss) - float(g[p + "loss"])) <= 2e-6 * max(1.0, abs(float(g[p + "loss"])))
    assert abs(_f(perp) - float(g[p + "perplexity"])) <= 2e-6 * float(g[p + "perplexity"])
    np.testing.assert_allclose(z.grad.numpy(), g[p + "dz"], rtol=2e-5, atol=2e-7)
    np.testing.assert_allclose(vq.w.weight.grad.numpy(), g[p + "dw"], rtol=2e-5, atol=2e-7)
    if cc == 0.0:
        assert np.array_equal(g[p + "dz"], g["C/g_out"])         # the straight-through value alone


def _fallback(model, sim, tm, z16):
    from dynamorph_amd.train import FusedTrainer
    return FusedTrainer._time_matching(types.SimpleNamespace(model=model), sim, tm, z16)


def _relations(B, seed, extra=()):
    g = torch.Generator().manual_seed(seed)
    tm = torch.randint(0, 3, (B, B), generator=g).float()
    for (i, j), v in extra:
        tm[i, j] = v
    return tm


@pytest.mark.parametrize("params", TM_PARAMS, ids=TM_IDS)
@pytest.mark.parametrize("B", [5, 37])
def test_trainer_time_matching_fallback(params, B):
    """FusedTrainer._time_matching (weighted hinge, mode 1) on host tensors: loss and d loss / d sim against the reference's
    expression in float64.  Relation values 0.5 and 3 keep themselves as weight; a pair planted exactly on the hinge
    (w_n sim + margin == 0 in fp32 and in float64) passes its gradient as torch.clamp's does at equality."""
    w_a, w_t, w_n, margin = params
    g = torch.Generator().manual_seed(B)
    sim = torch.rand(B, B, generator=g) * 4.0
    sim = (sim + sim.T) / 2
    sim.fill_diagonal_(0.0)
    tm = _relations(B, B + 1, extra=(((0, 1), 0.5), ((1, 0), 3.0)))
    on_hinge = []
    if w_n != 0 and -margin / w_n >= 0:
        s = np.float32(-margin / w_n)
        assert np.float32(s * np.float32(w_n)) + np.float32(margin) == 0.0 and s * w_n + margin == 0.0
        for i, j in ((2, 3), (3, 2), (B - 1, 0)):
            sim[i, j] = float(s)
            tm[i, j] = 0.0
            on_hinge.append((i, j))
    model = types.SimpleNamespace(w_a=w_a, w_t=w_t, w_n=w_n, margin=margin, _z16_loss=True)
    loss, g_sim = _fallback(model, sim, tm, None)
    s64 = sim.double().requires_grad_(True)
    ref = tm_loss_of_sim(s64, tm.double(), 1, w_a, w_t, w_n, margin)
    ref.backward()
    ref = float(ref.detach())
    assert abs(float(loss) - ref) <= 1e-6 * max(1.0, abs(ref)), (float(loss), ref)
    np.testing.assert_allclose(g_sim.double().numpy(), s64.grad.numpy(), rtol=1e-6, atol=1e-12)
    for i, j in on_hinge:
        assert float(g_sim[i, j]) == pytest.approx(w_n / B ** 2, rel=1e-6), (i, j)     # live at v == 0, like clamp
    for i in range(B):                                       # diagonal: tm 0 -> margin alone, live when margin >= 0
        if float(tm[i, i]) == 0.0:
            assert float(g_sim[i, i]) == pytest.approx((w_n / B ** 2) if margin >= 0 else 0.0, rel=1e-6, abs=1e-12)


def test_trainer_time_matching_fallback_sum_form():
    """Mode 0 (VQ_VAE, vq_vae.py:331): sum(sim * tm) with non-integer and one-way entries; the gradient is tm itself."""
    g = torch.Generator().manual_seed(3)
    sim = torch.rand(9, 9, generator=g)
    tm = torch.rand(9, 9, generator=g) * (torch.rand(9, 9, generator=g) < 0.4)
    tm[0, 4], tm[4, 0] = 0.5, 0.0
    loss, g_sim = _fallback(types.SimpleNamespace(_z16_loss=False), sim, tm, None)
    s64 = sim.double().requires_grad_(True)
    ref = tm_loss_of_sim(s64, tm.double(), 0)
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-6 * max(1.0, abs(float(ref)))
    assert torch.equal(g_sim.double(), s64.grad)
