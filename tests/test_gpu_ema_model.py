"""GPU: the EMA codebook mode through the modules, the trainers and the inference drivers.  The yardstick
of a training step is tests/helpers/ema_reference.py::OracleEMA -- the CPU oracle with a frozen codebook, commitment = cc *
e_latent_loss and the update applied after the step -- in fp32 and as a float64 copy, from the same state."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ema_reference as R  # noqa: E402
from conftest import codes_gate, grad_gate, loss_gate  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 1e-3
NAMES = ["VQ_VAE", "VQ_VAE_z16", "VQ_VAE_z32"]
# (biases of convolutions that feed a train-mode BatchNorm: their gradient is identically zero, tests/conftest.py NOISE)
BN_FED = {
    "VQ_VAE": ("enc.1.bias", "enc.4.bias", "enc.7.bias", "enc.10.bias", "enc.12.layers.0.1.bias", "enc.12.layers.0.4.bias",
               "enc.12.layers.1.1.bias", "enc.12.layers.1.4.bias"),
    "VQ_VAE_z32": ("enc.0.bias", "enc.3.bias", "dec.1.bias") + tuple(
        f"{blk}.layers.{i}.{j}.bias" for blk in ("enc.5", "dec.0") for i in (0, 1) for j in (1, 4)),
}
BN_FED["VQ_VAE_z16"] = BN_FED["VQ_VAE"]
EMA_KEYS = ("vq.w.weight", "vq.ema_cluster_size", "vq.ema_w")
_truth = {}


def _model(name, **kw):
    import dynamorph_amd
    kw.setdefault("ema_decay", R.EMA_DECAY)
    kw.setdefault("ema_epsilon", R.EMA_EPSILON)
    return getattr(dynamorph_amd, name)(**kw).to(DEV)


def truth(name):
    """One OracleEMA step in fp32 and float64 from the seed's state, computed once per model family and left unchanged."""
    if name not in _truth:
        ref, x = R.build_oracle(name, R.ONE_STEP_SEEDS[name])
        sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
        o32 = R.OracleEMA(ref)
        o64 = o32.double()
        out = {"x": x, "sd0": sd0}
        for tag, o, xx in (("32", o32, x), ("64", o64, x.double())):
            opt = torch.optim.Adam([p for p in o.model.parameters() if p.requires_grad], lr=LR, betas=(.9, .999))
            losses, z, idx = o.train_step(opt, xx)
            out["loss" + tag] = {k: float(v) for k, v in losses.items() if torch.is_tensor(v)}
            out["grad" + tag] = {k: p.grad.clone() for k, p in o.model.named_parameters() if p.grad is not None}
            out["z" + tag], out["idx" + tag] = z, idx
            out["ema" + tag] = {"vq.w.weight": o.codebook.clone(), "vq.ema_cluster_size": o.N.clone(), "vq.ema_w": o.m.clone()}
            out["e0"] = sd0["vq.w.weight"]
        assert "vq.w.weight" not in out["grad64"]
        assert torch.equal(out["idx32"], out["idx64"])
        _truth[name] = out
    return _truth[name]


def _hip_codes(model, x):
    with torch.no_grad():
        m = copy.deepcopy(model)
        return m.vq.encode_inputs(m.enc(x)).cpu()


@pytest.mark.parametrize("path", ["autograd", "fused-eager", "fused-graph"])
@pytest.mark.parametrize("name", NAMES)
def test_one_step_against_the_ema_oracle(name, path):
    from dynamorph_amd.train import FusedTrainer
    t = truth(name)
    x = t["x"].to(DEV)
    m = _model(name)
    m.load_state_dict(t["sd0"])                       # a checkpoint without the buffers: N = 1, m = e
    assert torch.equal(m.vq.ema_w.cpu(), t["e0"]) and not m.vq.w.weight.requires_grad
    idx = _hip_codes(m, x)
    flips = idx != t["idx64"]
    codes_gate(flips, t["z64"], t["e0"], f"{name} {path}")
    assert int(flips.sum()) == 0                      # the seed was chosen for it (ema_reference.ONE_STEP_SEEDS)
    if path == "autograd":
        opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=LR, betas=(.9, .999))
        _, ld = m(x)
        ld["total_loss"].backward()
        opt.step()
        got = {k: float(ld[k]) for k in ("recon_loss", "commitment_loss", "total_loss", "perplexity")}
        assert m.vq.w.weight.grad is None
    else:
        tr = FusedTrainer(m, lr=LR, use_graph=(path == "fused-graph"))
        vals = tr.step(x).tolist()
        got = dict(zip(("recon_loss", "commitment_loss", "total_loss", "perplexity"), vals))
        tr.expose_grads()
    torch.cuda.synchronize()
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        loss_gate(got[k], t["loss32"][k], f"{name} {path} {k}")
    loss_gate(got["perplexity"], t["loss32"]["perplexity"], f"{name} {path} perplexity", tol=1e-4)
    grad_gate(m, t["grad32"], t["grad64"], skip=BN_FED[name], factor=1.5, floor=2e-4, what=f"{name} {path}")
    sd = m.state_dict()
    for k in EMA_KEYS:
        want = t["ema64"][k]
        scale = max(float(want.abs().max()), 1e-6)
        e_ref = float((t["ema32"][k].double() - want).abs().max())
        e_hip = float((sd[k].detach().cpu().double() - want).abs().max())
        print(f"{name} {path} {k}: hip {e_hip:.3e} fp32 oracle {e_ref:.3e} scale {scale:.3e}")
        assert e_hip <= max(1.5 * e_ref, 2e-4 * scale), (k, e_hip, e_ref, scale)
    # the counts are integers: after one step from N = 1 the buffer is exactly decay + (1 - decay) n up to its one rounding
    n = torch.bincount(t["idx64"].flatten(), minlength=t["e0"].shape[0]).double()
    want_N = (R.EMA_DECAY * 1.0 + (1.0 - R.EMA_DECAY) * n).float()
    assert torch.equal(sd["vq.ema_cluster_size"].cpu(), want_N)


@pytest.mark.parametrize("name", NAMES)
def test_eager_and_captured_steps_are_bit_equal(name):
    from dynamorph_amd.train import FusedTrainer
    t = truth(name)
    ms, trs = [], []
    for use_graph in (False, True):
        m = _model(name)
        m.load_state_dict(t["sd0"])
        ms.append(m)
        trs.append(FusedTrainer(m, lr=LR, use_graph=use_graph))
    for step in range(3):
        x = torch.randn(4, 2, 128, 128, generator=torch.Generator().manual_seed(60 + step)).to(DEV)
        vals = [tr.step(x) for tr in trs]
        assert torch.equal(vals[0], vals[1]), step
    torch.cuda.synchronize()
    assert torch.equal(trs[0].flat, trs[1].flat)
    a, b = ms[0].state_dict(), ms[1].state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["vq.w.weight"].cpu(), t["e0"])              # (and the codebook did move)


def test_frozen_codebook_is_no_adam_parameter():
    from dynamorph_amd.train import FusedTrainer
    on, off = _model("VQ_VAE"), _model("VQ_VAE", ema_decay=None)
    tr_on, tr_off = FusedTrainer(on, use_graph=False), FusedTrainer(off, use_graph=False)
    kd = on.vq.w.weight.numel()
    assert all(p is not on.vq.w.weight for p in tr_on.params) and any(p is off.vq.w.weight for p in tr_off.params)
    for a in ("flat", "grad", "m", "v"):
        assert getattr(tr_off, a).numel() - getattr(tr_on, a).numel() == kd, a
    K, D = on.vq.w.weight.shape
    assert tr_on._ema_stats.numel() == K * (D + 1) and tr_off._ema_stats is None
    assert tr_on._bucket.numel() == tr_on.grad.numel() + K * (D + 1) and tr_off._bucket is tr_off.grad


def test_mode_off_is_untouched():
    """ema_decay=None: one fused step is bit-equal to a step of a model built without the keyword."""
    from dynamorph_amd.train import FusedTrainer
    import dynamorph_amd
    t = truth("VQ_VAE")
    x = t["x"].to(DEV)
    outs = []
    for m in (dynamorph_amd.VQ_VAE(ema_decay=None).to(DEV), dynamorph_amd.VQ_VAE().to(DEV)):
        m.load_state_dict(t["sd0"])
        tr = FusedTrainer(m, lr=LR, use_graph=False)
        vals = tr.step(x)
        outs.append((vals, {k: v.clone() for k, v in m.state_dict().items()}, tr.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][2], outs[1][2])
    assert list(outs[0][1]) == list(outs[1][1])
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k
    assert not torch.equal(outs[0][1]["vq.w.weight"].cpu(), t["e0"])     # the gradient-trained codebook took an Adam step


@pytest.mark.parametrize("name", ["VQ_VAE", "VQ_VAE_z32"])
def test_eval_and_no_grad_forwards_do_not_update(name):
    t = truth(name)
    x = t["x"].to(DEV)
    m = _model(name)
    m.load_state_dict(t["sd0"])
    before = {k: m.state_dict()[k].clone() for k in EMA_KEYS}
    m.eval()
    m(x)
    m.vq(m.enc(x))
    m.train()
    with torch.no_grad():                             # the training loop's validation pass
        m(x)
    m.vq.encode_inputs(m.enc(x))
    torch.cuda.synchronize()
    for k in EMA_KEYS:
        assert torch.equal(m.state_dict()[k], before[k]), k
    m(x)                                              # a training forward does
    assert not torch.equal(m.state_dict()["vq.w.weight"], before["vq.w.weight"])
    # ... and VectorQuantizer.forward on its own as well
    before = {k: m.state_dict()[k].clone() for k in EMA_KEYS}
    m.vq(m.enc(x).detach())
    assert not torch.equal(m.state_dict()["vq.ema_w"], before["vq.ema_w"])


@pytest.mark.parametrize("name", ["VQ_VAE", "VQ_VAE_z32"])
def test_inference_drivers(name):
    """encode_patches and patch_gradients: the results of a gradient-trained model with the same weights, to the bit (the
    input gradient never saw q_latent_loss); score_patches: this mode's commitment, cc * mse, and the total built on it."""
    import dynamorph_amd
    from dynamorph_amd.patch_vae import encode_patches, patch_gradients, score_patches
    t = truth(name)
    x = t["x"]
    m = _model(name, commitment_cost=0.4)
    m.load_state_dict(t["sd0"])
    plain = getattr(dynamorph_amd, name)(commitment_cost=0.4).to(DEV)
    plain.load_state_dict(t["sd0"])
    before = {k: m.state_dict()[k].clone() for k in EMA_KEYS}
    za, zb = encode_patches(copy.deepcopy(m), x, device=DEV), encode_patches(copy.deepcopy(plain), x, device=DEV)
    assert np.array_equal(za[0], zb[0]) and np.array_equal(za[1], zb[1])
    for of in ("total_loss", "commitment_loss"):
        ga = patch_gradients(copy.deepcopy(m), x, of=of, device=DEV)
        gb = patch_gradients(copy.deepcopy(plain), x, of=of, device=DEV)
        assert np.array_equal(ga, gb), of
    out = score_patches(m, x, device=DEV, batch_size=4)
    ref = score_patches(copy.deepcopy(plain), x, device=DEV, batch_size=4)
    wr, wc = (1.0, 1.0) if name == "VQ_VAE_z32" else (float(m.weight_recon), float(m.weight_commitment))
    for i in range(x.shape[0]):
        mse = float(np.mean((out["z_after"][i].astype(np.float64) - out["z_before"][i].astype(np.float64)) ** 2))
        loss_gate(out["commitment_loss"][i], 0.4 * mse, f"{name} ema commitment[{i}]")
        loss_gate(ref["commitment_loss"][i], mse + 0.4 * mse, f"{name} plain commitment[{i}]")
        loss_gate(out["total_loss"][i], wr * float(out["recon_loss"][i]) + wc * 0.4 * mse, f"{name} ema total[{i}]")
    assert np.array_equal(out["recon_loss"], ref["recon_loss"]) and np.array_equal(out["perplexity"], ref["perplexity"])
    for k in EMA_KEYS:                                # a train-mode model: the drivers still update nothing
        assert torch.equal(m.state_dict()[k], before[k]), k


def test_fused_validation_pass_reports_the_mode_and_updates_nothing():
    from dynamorph_amd.train import FusedTrainer
    t = truth("VQ_VAE")
    x = t["x"].to(DEV)
    m = _model("VQ_VAE")
    m.load_state_dict(t["sd0"])
    before = {k: m.state_dict()[k].clone() for k in EMA_KEYS}
    tr = FusedTrainer(m, lr=LR, use_graph=False)
    vals = tr.evaluate(x).tolist()
    loss_gate(vals[1], t["loss32"]["commitment_loss"], "fused validation commitment")
    for k in EMA_KEYS:
        assert torch.equal(m.state_dict()[k], before[k]), k


def test_both_refusals(monkeypatch):
    from dynamorph_amd import dist as D
    from dynamorph_amd.train import GraphedTrainer, _make_optimizer
    m = _model("VQ_VAE")
    with pytest.raises(ValueError, match="EMA"):
        GraphedTrainer(m)
    with pytest.raises(ValueError, match="EMA"):
        _make_optimizer(m, LR, "graph")
    monkeypatch.setattr(D, "world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="EMA codebook update with more than one rank"):
        _make_optimizer(m, LR, False)
