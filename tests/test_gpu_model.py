"""Module-level parity of the HIP path (dynamorph_amd.VQ_VAE & friends, called exactly as
run_training.py / pipeline/patch_VAE.py call the reference) against the golden vectors captured
from the reference and against the CPU oracle on fresh seeded inputs.

Gates (SURVEY.md section 7 "hard parts"):
  * VQ on golden z_before: indices bit-identical (test_gpu_kernels.py).
  * end to end: losses within 1e-5; indices identical except where the reference's own
    best/second-best distance gap is below 1e-4 relative (count reported, must be tiny).
"""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import codes_gate, grad_gate, loss_gate, oracle_truth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# conv biases that feed a train-mode BatchNorm: exact gradient is 0; the reference's autograd returns
# rounding noise (~1e-9) which Adam then amplifies to +-lr.  They cannot (and need not) be matched.
BN_FED_BIASES = ("enc.1.bias", "enc.4.bias", "enc.7.bias", "enc.10.bias",
                 "enc.12.layers.0.1.bias", "enc.12.layers.0.4.bias", "enc.12.layers.1.1.bias", "enc.12.layers.1.4.bias")


def fresh(golden, cls=None, **kw):
    import dynamorph_amd
    cls = cls or dynamorph_amd.VQ_VAE
    m = cls(**kw).to(DEV)
    g1 = golden("g1_state_dict.npz")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in g1.items()})
    return m


def close(a, b, rtol, atol, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max():.3e} (ref max {b.abs().max():.3e})"


def near_tie_mask(z, codebook, rel=1e-4):
    """positions whose reference top-2 distance gap is within `rel` of the best distance"""
    d = ((z.unsqueeze(1) - codebook.reshape(1, *codebook.shape, 1, 1)) ** 2).sum(2)     # (B,K,H,W)
    top2 = torch.topk(-d, 2, dim=1).values
    return (top2[:, 0] - top2[:, 1]).abs() <= rel * top2[:, 0].abs()


def test_encoder_layers_against_reference_activations(golden):
    """Layer-by-layer check of the encoder kernels (localises a failure)."""
    from dynamorph_amd import engine as E
    m = fresh(golden)
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    acts = golden("g3_debug_acts.npz")
    L = E.Layers(m)
    z, cx = E.encoder_forward(L, x)
    close(cx.a1, acts["enc1"], 2e-5, 2e-5, "enc.1 output")
    close(cx.a2, acts["enc4"], 5e-5, 5e-5, "enc.4 output")
    close(cx.a3, acts["enc7"], 1e-4, 1e-4, "enc.7 output")
    close(cx.a4, acts["enc10"], 1e-4, 1e-4, "enc.10 output")
    close(cx.res[0].h_in, acts["enc11"], 1e-4, 1e-4, "enc.11 output")
    close(cx.res[0].ra, acts["res0_1"], 1e-4, 1e-4, "res0 conv3x3")
    close(cx.res[0].rb, acts["res0_4"], 1e-4, 1e-4, "res0 conv1x1")
    close(cx.res[1].rb, acts["res1_4"], 2e-4, 2e-4, "res1 conv1x1")
    close(z, golden("g3_encoder.npz")["z_before"], 2e-4, 2e-4, "z_before")


def test_encoder_batch_statistics_and_running_stats(golden):
    m = fresh(golden)
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    g3 = golden("g3_encoder.npz")
    z = m.enc(x)
    close(z, g3["z_before"], 2e-4, 2e-4, "z_before")
    for k, v in m.state_dict().items():
        if "running" in k:
            close(v, g3["rs_batch/" + k], 1e-5, 1e-6, k)
        if "tracked" in k:
            assert int(v) == int(g3["rs_batch/" + k]), k


def test_process_vae_semantics_per_sample(golden):
    """pipeline/patch_VAE.py:445-452: enc -> vq on batches of one (train-mode BN) == per-sample statistics."""
    from dynamorph_amd.patch_vae import encode_patches
    m = fresh(golden)
    x = torch.from_numpy(golden("g2_input.npz")["x"])
    g3 = golden("g3_encoder.npz")
    zb, za = encode_patches(m, x, device=DEV, batch_size=3)         # ragged last chunk on purpose
    assert zb.shape == (4, 4096) and za.shape == (4, 4096)
    close(zb, g3["z_before_per_sample"].reshape(4, -1), 2e-4, 2e-4, "z_before per sample")
    cb = torch.from_numpy(golden("g4_vq_indices.npz")["codebook"])
    zb_ref = torch.from_numpy(g3["z_before_per_sample"])
    tie = near_tie_mask(zb_ref, cb).unsqueeze(1).expand(-1, 16, -1, -1).reshape(4, -1)
    diff = (torch.from_numpy(za) - torch.from_numpy(g3["z_after_per_sample"]).reshape(4, -1)).abs() > 1e-4
    assert not (diff & ~tie).any(), f"{int((diff & ~tie).sum())} quantized values differ away from ties"
    assert tie.float().mean() < 1e-3
    for k, v in m.state_dict().items():
        if "running" in k:
            close(v, g3["rs_ps/" + k], 1e-4, 1e-5, k)
        if "tracked" in k:
            assert int(v) == int(g3["rs_ps/" + k]), k
    # the same numbers from literal batch-of-one module calls, as the reference loop does it
    m2 = fresh(golden)
    z1 = m2.enc(x[1:2].to(DEV))
    close(z1, g3["z_before_per_sample"][1:2], 2e-4, 2e-4, "batch-of-one call")


def test_vq_module_surface(golden):
    m = fresh(golden)
    g4, g5 = golden("g4_vq_indices.npz"), golden("g5_vq_forward.npz")
    z = torch.from_numpy(g5["z_before"]).to(DEV)
    assert np.array_equal(m.vq.encode_inputs(z).cpu().numpy(), g4["idx"])
    q, loss, perp = m.vq(z)
    assert np.array_equal(q.detach().cpu().numpy().view(np.uint32), g5["quantized"].view(np.uint32))
    assert abs(float(loss) - float(g5["loss"])) <= 1e-6 * float(g5["loss"])
    assert abs(float(perp) - float(g5["perplexity"])) <= 1e-5 * float(g5["perplexity"])
    dq = m.vq.decode_inputs(torch.from_numpy(g4["idx"]).to(DEV))
    assert torch.equal(dq.cpu(), torch.from_numpy(g4["codebook"])[torch.from_numpy(g4["idx"])].permute(0, 3, 1, 2))
    assert m.vq.embeddings is m.vq.w.weight


@pytest.mark.parametrize("masked", [False, True])
def test_forward_losses_and_reconstruction(golden, masked):
    m = fresh(golden)
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    g = golden("g5_forward_masked.npz" if masked else "g5_forward.npz")
    mask = torch.from_numpy(g["mask"]).to(DEV) if masked else None
    dec, ld = m(x, batch_mask=mask)
    assert list(ld.keys()) == ["recon_loss", "commitment_loss", "time_matching_loss", "total_loss", "perplexity"]
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        assert abs(float(ld[k]) - float(g[k])) <= 1e-5, (k, float(ld[k]), float(g[k]))       # north-star tolerance
    assert abs(float(ld["perplexity"]) - float(g["perplexity"])) <= 1e-3 * float(g["perplexity"])
    assert ld["time_matching_loss"] == 0.
    # decoded: identical codes except near-ties -> compare per sample where all codes agree
    idx_ref = golden("g4_vq_indices.npz")["idx"]
    idx = m.vq.encode_inputs(m.enc(x)).cpu().numpy()      # (running stats mutate: irrelevant here)
    same = (idx == idx_ref).reshape(4, -1).all(1)
    codes_gate(idx != idx_ref, golden("g5_vq_forward.npz")["z_before"], golden("g4_vq_indices.npz")["codebook"], "VQ_VAE.forward")
    for b in range(4):
        if same[b]:
            close(dec[b], g["decoded"][b], 5e-4, 5e-4, f"decoded[{b}]")
    if not masked:
        acts = golden("g5_debug_dec_acts.npz")
        from dynamorph_amd import engine as E
        zq = torch.from_numpy(golden("g5_vq_forward.npz")["quantized"]).to(DEV)
        d, cx = E.decoder_forward(E.Layers(m), zq, x)
        close(cx.d0, acts["dec1"], 2e-5, 2e-5, "dec.0+relu")
        close(cx.d2, acts["dec3"], 5e-5, 5e-5, "dec.2+relu")
        assert cx.d4 is None                                   # fused tail: never materialised
        close(E._dec4_forward(E.Layers(m), cx.d2)[:1], acts["dec5"], 1e-4, 1e-4, "dec.4+relu")
        close(d, g["decoded"], 1e-4, 1e-4, "decoded from golden z_after")


def test_gradients_against_reference(golden):
    """G6: every parameter gradient of total_loss.backward() as the REFERENCE computed it (fp32, CPU), judged on the float64
    yardstick: the HIP gradient is as close to the float64 truth (the oracle run in double on the same weights and input)
    as the reference's own fp32 gradient is, x 1.5 -- conftest.grad_gate, in place of a flat share of the tensor's scale."""
    from oracle import vqvae_oracle as O
    m = fresh(golden)
    xh = torch.from_numpy(golden("g2_input.npz")["x"])
    g6, g1 = golden("g6_grads.npz"), golden("g1_state_dict.npz")
    ref = O.OracleVQVAE()
    ref.load_state_dict({k: torch.from_numpy(v) for k, v in g1.items()})
    _, _, g64 = oracle_truth(ref, xh)
    g32 = {k: torch.from_numpy(g6["grad/" + k]) for k in g64}              # the reference's own gradients, not the oracle's
    dec, ld = m(xh.to(DEV))
    ld["total_loss"].backward()
    assert m.channel_var.grad is None
    for k in BN_FED_BIASES:
        p = dict(m.named_parameters())[k]
        assert p.grad.abs().max().item() == 0.0, k                        # exact zero by construction
        assert g32[k].abs().max().item() < 1e-6, k                        # the reference only has rounding noise there
    n = grad_gate(m, g32, g64, skip=BN_FED_BIASES, what="G6 gradients")
    assert n == sum(1 for _, p in m.named_parameters() if p.requires_grad) - len(BN_FED_BIASES)


def test_decoder_and_vq_gradients_in_isolation(golden):
    """dz_after / dz_before of the reference graph, fed the golden z tensors (no encoder noise)."""
    m = fresh(golden)
    g6, g5 = golden("g6_grads.npz"), golden("g5_vq_forward.npz")
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    zb = torch.from_numpy(g5["z_before"]).to(DEV).requires_grad_(True)
    za, closs, _ = m.vq(zb)
    za.retain_grad()
    from dynamorph_amd.vq_vae import _DecoderFn
    from dynamorph_amd import engine as E
    L = E.Layers(m)
    dec, recon = _DecoderFn.apply(za, x, None, L, *L.decoder_params())
    (recon + closs).backward()
    close(za.grad, g6["dz_after"], 2e-4, 1e-9, "dz_after")
    close(zb.grad, g6["dz_before"], 2e-4, 1e-9, "dz_before")
    for k in ("dec.0.weight", "dec.0.bias", "dec.2.weight", "dec.2.bias", "dec.4.weight", "dec.4.bias",
              "dec.6.weight", "dec.6.bias", "vq.w.weight"):
        p = dict(m.named_parameters())[k]
        ref = g6["grad/" + k]
        close(p.grad, ref, 2e-4, 2e-4 * np.abs(ref).max(), k)


def test_adam_steps_with_torch_optimizer(golden):
    """run_training.py:404-408 loop with torch.optim.Adam driving the HIP model (drop-in check)."""
    m = fresh(golden)
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    g7 = golden("g7_adam.npz")
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, betas=(.9, .999))
    m.zero_grad()
    for step in range(3):
        _, ld = m(x)
        ld["total_loss"].backward()
        opt.step()
        m.zero_grad()
        for i, k in enumerate(("recon_loss", "commitment_loss", "total_loss")):
            loss_gate(ld[k], g7["losses"][step][i], f"torch Adam, step {step}, {k}")
        if step == 0:
            for k, v in m.state_dict().items():
                if k in BN_FED_BIASES or "tracked" in k:
                    continue
                # one Adam step moves every weight by ~lr regardless of gradient scale: compare the step
                close(v, g7["step1/" + k], 0, 2.5e-5 if "running" not in k else 1e-5, k)


def test_oracle_parity_fresh_seed_larger_batch():
    """Fresh seeded input + fresh seeded weights, B=16: HIP vs the CPU oracle (not a golden file)."""
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    torch.manual_seed(123)
    ref = O.OracleVQVAE()
    x = torch.randn(16, 2, 128, 128, generator=torch.Generator().manual_seed(1234))
    m = dynamorph_amd.VQ_VAE().to(DEV)
    m.load_state_dict(ref.state_dict())
    dec_r, ld_r = ref(x)
    ld_r["total_loss"].backward()
    dec, ld = m(x.to(DEV))
    ld["total_loss"].backward()
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        assert abs(float(ld[k]) - float(ld_r[k])) <= 1e-5, (k, float(ld[k]), float(ld_r[k]))
    # a code flipped at a near-tie changes the gradient discretely (1 of 4096 positions): allow for it
    ref2 = O.OracleVQVAE()
    ref2.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    idx_ref = ref2.vq.encode_inputs(ref2.enc(x))
    idx = m.vq.encode_inputs(m.enc(x.to(DEV))).cpu()
    codes_gate(idx != idx_ref, ref2.enc(x).detach(), ref2.vq.w.weight.detach(), "fresh-seed model")
    flips = int((idx != idx_ref).sum())
    # The reference's fp32 gradients carry ~3e-3 relative accumulation noise of their own (measured against
    # an fp64 run of the same graph).  Gate: the HIP gradients are as close to the fp64 truth as the
    # reference's fp32 CPU path is (x1.5), or within 2e-4 of the tensor's scale.
    import copy
    torch.manual_seed(123)
    ref64 = O.OracleVQVAE()
    ref64 = copy.deepcopy(ref64).double()
    ref64.zero_grad()
    _, ld64 = ref64(x.double())
    ld64["total_loss"].backward()
    g32, g64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    if flips == 0:
        for k, p in m.named_parameters():
            if p.requires_grad and k not in BN_FED_BIASES:
                truth = g64[k].grad
                scale = max(truth.abs().max().item(), 1e-6)
                e_ref = (g32[k].grad.double() - truth).abs().max().item()
                e_hip = (p.grad.cpu().double() - truth).abs().max().item()
                assert e_hip <= max(1.5 * e_ref, 2e-4 * scale) + 1e-9, (k, e_hip, e_ref, scale)


def test_z16_variant_time_matching(golden):
    import dynamorph_amd
    g = golden("g8_z16_time_matching.npz")
    m = fresh(golden, cls=dynamorph_amd.VQ_VAE_z16, gpu=True)          # patch_VAE.py:431 passes gpu=True
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    dec, ld = m(x, time_matching_mat=torch.from_numpy(g["tm"]).to(DEV))
    assert list(ld.keys()) == ["recon_loss", "commitment_loss", "time_matching_loss", "perplexity", "total_loss"]
    for k in ("recon_loss", "commitment_loss", "time_matching_loss", "total_loss"):
        loss_gate(ld[k], g[k], f"z16 time matching, {k}")
    ld["total_loss"].backward()
    for k in ("enc.10.weight", "enc.4.weight", "dec.0.weight"):
        p = dict(m.named_parameters())[k]
        ref = g["grad/" + k]
        close(p.grad, ref, 0, 3e-3 * np.abs(ref).max(), k)
    g2 = golden("g8_vqvae_time_matching.npz")
    m = fresh(golden)
    dec, ld = m(x, time_matching_mat=torch.from_numpy(g2["tm"]).to(DEV))
    for k in ("time_matching_loss", "total_loss"):
        assert abs(float(ld[k]) - float(g2[k])) <= 1e-4 * max(1.0, abs(float(g2[k]))), (k, float(ld[k]), float(g2[k]))


def test_round_trip_properties_full_size():
    """Size-independent properties at BASELINE config sizes (B=1024 latents): decode(encode(z)) is a fixed
    point of the quantiser, the histogram sums to P, loss == (1+beta)*mse, indices in range."""
    import dynamorph_amd
    from dynamorph_amd import ops
    torch.manual_seed(0)
    vq = dynamorph_amd.VectorQuantizer(16, 64).to(DEV)
    z = torch.randn(1024, 16, 16, 16, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    idx = vq.encode_inputs(z)
    assert idx.min() >= 0 and idx.max() < 64
    q = vq.decode_inputs(idx)
    assert torch.equal(vq.encode_inputs(q), idx)                     # idempotence
    out, loss, perp = vq(z)
    mse = torch.mean((q - z) ** 2)
    assert abs(float(loss) - 1.25 * float(mse)) <= 2e-6 * float(loss)
    _, _, slabs, hist = ops.vq_forward(z, vq.w.weight.detach())
    assert int(hist.sum()) == idx.numel()
    assert torch.equal(hist.cpu(), torch.bincount(idx.flatten().cpu(), minlength=64).int())
    p = hist.double() / idx.numel()
    assert abs(float(perp) - float(torch.exp(-(p * torch.log(p + 1e-10)).sum()))) < 1e-3


def test_cpu_input_raises():
    import dynamorph_amd
    m = dynamorph_amd.VQ_VAE()
    with pytest.raises(RuntimeError):
        m(torch.randn(1, 2, 128, 128))


@pytest.mark.parametrize("use_graph", [False, True])
def test_fused_trainer_matches_reference_adam(golden, use_graph):
    """FusedTrainer.step (flat buffers, fused Adam, optional HIP-graph replay) vs the reference's
    model(x) / backward / torch.optim.Adam.step loop (g7)."""
    from dynamorph_amd.train import FusedTrainer
    m = fresh(golden)
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    g7 = golden("g7_adam.npz")
    tr = FusedTrainer(m, lr=1e-4, use_graph=use_graph)
    for step in range(3):
        vals = tr.step(x).tolist()
        for i, k in enumerate(("recon_loss", "commitment_loss", "total_loss")):
            loss_gate(vals[i], g7["losses"][step][i], f"FusedTrainer(graph={use_graph}), step {step}, {k}")
        if step == 0:
            for k, v in m.state_dict().items():
                if k in BN_FED_BIASES:
                    assert torch.equal(v.cpu(), torch.from_numpy(golden("g1_state_dict.npz")[k])), k   # zero grad: untouched
                elif "tracked" in k:
                    assert int(v) == 1, (k, int(v))
                else:
                    close(v, g7["step1/" + k], 0, 2.5e-5 if "running" not in k else 1e-5, k)
    assert int(m.enc[2].num_batches_tracked) == 3
    # the flat buffer IS the parameter storage
    assert m.enc[0].weight.data_ptr() == tr.flat.data_ptr()


def test_fused_trainer_equals_autograd_path(golden):
    """Same kernels through torch.autograd + torch.optim.Adam and through FusedTrainer: same parameters."""
    from dynamorph_amd.train import FusedTrainer
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    m1, m2 = fresh(golden), fresh(golden)
    opt = torch.optim.Adam(m1.parameters(), lr=1e-4, betas=(.9, .999))
    tr = FusedTrainer(m2, lr=1e-4, use_graph=False)
    for _ in range(2):
        _, ld = m1(x)
        ld["total_loss"].backward()
        opt.step()
        m1.zero_grad()
        tr.step(x)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        close(a, b, 1e-6, 1e-6, k)       # (the two paths differ in their decoder-tail and codebook-gradient kernels)


@pytest.mark.parametrize("use_graph", [False, True])
def test_fused_trainer_join_in_the_quantiser_changes_no_bit(golden, monkeypatch, use_graph):
    """The last residual join inside the quantiser's load path (dm_vq_forward_join, the default) against the join as its
    own launch (train.JOIN_IN_VQ = False): same losses, parameters and BatchNorm buffers bit for bit over three steps."""
    import dynamorph_amd.train as T
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    res = {}
    for join in (True, False):
        monkeypatch.setattr(T, "JOIN_IN_VQ", join)
        m = fresh(golden)
        tr = T.FusedTrainer(m, lr=1e-3, use_graph=use_graph)
        vals = [tr.step(x).tolist() for _ in range(3)]
        vals.append(tr.evaluate(x).tolist())
        res[join] = (vals, {k: v.clone() for k, v in m.state_dict().items()})
    assert res[True][0] == res[False][0]
    for k, v in res[True][1].items():
        assert torch.equal(v, res[False][1][k]), k


@pytest.mark.parametrize("cls_name,kw,hw", [("VQ_VAE", {}, 128), ("VQ_VAE_z32", {}, 128),
                                            ("VQ_VAE", dict(num_inputs=4, num_embeddings=512, channel_var=np.ones(4)), 256)])
def test_fused_backward_kernels_against_the_two_kernel_path(monkeypatch, cls_name, kw, hw):
    """Round 4's one-staging backward kernels (conv1x1 / conv3x3 / conv4x4s2 / transposed) against the data-gradient +
    weight-gradient pairs they replace (engine.FUSED_BACKWARD = False), through the whole model: same losses, every parameter
    gradient equal to accumulation-order tolerance -- on the default 16 x 16 latents (all five kernels), on VQ_VAE_z32 and on
    256-pixel patches (32 x 32 latents: only the shapes they are built for switch over, the rest keeps the pairs)."""
    import dynamorph_amd
    import dynamorph_amd.engine as E
    torch.manual_seed(31)
    m0 = getattr(dynamorph_amd, cls_name)(**kw).to(DEV)
    x = torch.randn(3, m0.num_inputs if hasattr(m0, "num_inputs") else 2, hw, hw, device=DEV)
    grads = {}
    for fused in (True, False):
        monkeypatch.setattr(E, "FUSED_BACKWARD", fused)
        m = copy.deepcopy(m0)
        _, ld = m(x)
        ld["total_loss"].backward()
        grads[fused] = ({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None},
                        [float(ld[k]) for k in ("recon_loss", "commitment_loss", "total_loss")])
    assert grads[True][1] == grads[False][1]
    assert len(grads[True][0]) > 30
    for k, g in grads[True][0].items():
        ref = grads[False][0][k]
        scale = float(ref.abs().max())
        assert float((g - ref).abs().max()) <= 2e-5 * scale + 1e-9, (k, float((g - ref).abs().max()), scale)


def test_fused_trainer_prepare_captures_without_taking_a_step(golden):
    """FusedTrainer.prepare (bench.py keeps the one-off graph capture out of its timed steps with it): parameters,
    BatchNorm buffers and the Adam state are untouched, and the steps that follow equal those of a trainer that captured
    inside its first step."""
    from dynamorph_amd.train import FusedTrainer
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    m1, m2 = fresh(golden), fresh(golden)
    t1, t2 = FusedTrainer(m1, lr=1e-4, use_graph=True), FusedTrainer(m2, lr=1e-4, use_graph=True)
    before = {k: v.clone() for k, v in m1.state_dict().items()}
    buf = t1.prepare(x)
    torch.cuda.synchronize()
    assert buf is not None and buf.shape == x.shape and torch.equal(buf, x)
    for k, v in m1.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert float(t1.m.abs().max()) == 0.0 and float(t1.v.abs().max()) == 0.0
    outs = []
    for _ in range(2):
        outs.append((t1.step(buf).clone(), t2.step(x).clone()))
    for a, b in outs:
        assert torch.equal(a, b)
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k


# ===================================================================================== VQ_VAE_z32
Z32_BN_FED_BIASES = ("enc.0.bias", "enc.3.bias", "dec.1.bias") + tuple(
    f"{blk}.layers.{i}.{j}.bias" for blk in ("enc.5", "dec.0") for i in (0, 1) for j in (1, 4))


def test_z32_forward_against_reference(golden):
    """VQ_VAE_z32 (vae.py:348-474): latents, reconstruction and losses vs the vectors captured from the reference."""
    import dynamorph_amd
    g = golden("g8_z32.npz")
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    m = dynamorph_amd.VQ_VAE_z32().to(DEV)
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd/")})
    zb = m.enc(x)
    close(zb, g["z_before"], 2e-5, 2e-5, "z32 z_before")
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd/")})
    dec, ld = m(x)
    assert list(ld.keys()) == ["recon_loss", "commitment_loss", "time_matching_loss", "perplexity", "total_loss"]
    close(dec, g["decoded"], 1e-4, 1e-4, "z32 decoded")
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        assert abs(float(ld[k]) - float(g[k])) <= 1e-5, (k, float(ld[k]), float(g[k]))
    assert abs(float(ld["perplexity"]) - float(g["perplexity"])) <= 1e-3 * float(g["perplexity"])


def test_z32_time_matching_mask_and_gradients_against_reference(golden):
    """VQ_VAE_z32 forward + backward with a time-matching matrix and a batch mask against the vectors captured from the
    reference (g8_z32_tm.npz): losses within the north star's 1e-5, every gradient within the accumulation noise of fp32."""
    import dynamorph_amd
    g = golden("g8_z32_tm.npz")
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    m = dynamorph_amd.VQ_VAE_z32().to(DEV)
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd/")})
    dec, ld = m(x, time_matching_mat=torch.from_numpy(g["tm"]).to(DEV), batch_mask=torch.from_numpy(g["mask"]).to(DEV))
    close(dec, g["decoded"], 1e-4, 1e-4, "z32 decoded (masked, time matching)")
    for k in ("recon_loss", "commitment_loss", "time_matching_loss", "total_loss"):
        assert abs(float(ld[k]) - float(g[k])) <= 1e-5 * max(1.0, abs(float(g[k]))), (k, float(ld[k]), float(g[k]))
    ld["total_loss"].backward()
    for k, p in m.named_parameters():
        if not p.requires_grad or k in Z32_BN_FED_BIASES:
            continue
        ref = g["grad/" + k]
        scale = max(float(np.abs(ref).max()), 1e-6)
        err = float((p.grad.cpu() - torch.from_numpy(ref)).abs().max())
        assert err <= 4e-3 * scale + 1e-8, (k, err, scale)


def test_z32_extra_loss_against_reference(golden):
    """VQ_VAE_z32(extra_loss={name: fn}, alpha=...) (vae.py:463-469) against the vectors captured from the reference's class
    (g8_z32_extra.npz): the caller's loss functions run in torch on the device latents, their gradient reaches the encoder
    through the quantiser's straight-through backward.  Keys in the reference's order, losses within 1e-5, gradients within
    the accumulation noise of fp32; FusedTrainer declines such a model and train() takes the autograd path for it."""
    import sys
    import dynamorph_amd
    from dynamorph_amd.train import FusedTrainer, _make_optimizer
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
    from extra_losses import EXTRA
    g = golden("g8_z32_extra.npz")
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    m = dynamorph_amd.VQ_VAE_z32(extra_loss=dict(EXTRA), alpha=float(g["alpha"])).to(DEV)
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd/")})
    dec, ld = m(x, labels=torch.from_numpy(g["labels"]).to(DEV), time_matching_mat=torch.from_numpy(g["tm"]).to(DEV))
    assert list(ld.keys()) == [str(k) for k in g["loss_keys"]]
    close(dec, g["decoded"], 1e-4, 1e-4, "z32 decoded (extra losses)")
    for k in ld:
        if k == "perplexity":
            continue
        ref = float(g["loss/" + k])
        assert abs(float(ld[k]) - ref) <= 1e-5 * max(1.0, abs(ref)), (k, float(ld[k]), ref)
    ld["total_loss"].backward()
    for k, p in m.named_parameters():
        if not p.requires_grad or k in Z32_BN_FED_BIASES:
            continue
        ref = g["grad/" + k]
        scale = max(float(np.abs(ref).max()), 1e-6)
        err = float((p.grad.cpu() - torch.from_numpy(ref)).abs().max())
        assert err <= 4e-3 * scale + 1e-8, (k, err, scale)
    # train() has no labels to hand to the extra losses (run_training.py:509-520 passes none): it keeps the autograd path;
    # FusedTrainer itself takes such a model (step(..., labels=...): test_fused_trainer_z32_with_extra_losses_...)
    assert isinstance(_make_optimizer(m, 1e-3, True), torch.optim.Adam)
    # the reference's constructor never sets alpha: without it the attribute is missing there and here
    m2 = dynamorph_amd.VQ_VAE_z32(extra_loss=dict(EXTRA)).to(DEV)
    with pytest.raises(AttributeError, match="alpha"):
        m2(x, labels=torch.from_numpy(g["labels"]).to(DEV))
    with pytest.raises(TypeError):
        dynamorph_amd.VQ_VAE_z32(extra_loss=[EXTRA["class_spread"]])


def test_z32_gradients_against_oracle():
    """Fresh weights and inputs, masked loss + time matching: every gradient vs the fp64 oracle (same gate as the
    16x16 model: as close to the truth as the reference's own fp32 path, x1.5)."""
    import copy
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    torch.manual_seed(77)
    ref = O.OracleVQVAEz32()
    x = torch.randn(6, 2, 128, 128, generator=torch.Generator().manual_seed(78))
    mask = (torch.rand(6, 1, 128, 128, generator=torch.Generator().manual_seed(79)) > 0.3).float()
    tm = torch.randint(0, 3, (6, 6), generator=torch.Generator().manual_seed(80)).float()
    ref64 = copy.deepcopy(ref).double()
    m = dynamorph_amd.VQ_VAE_z32().to(DEV)
    m.load_state_dict(ref.state_dict())
    _, ld_r = ref(x, time_matching_mat=tm, batch_mask=mask)
    ld_r["total_loss"].backward()
    _, ld64 = ref64(x.double(), time_matching_mat=tm.double(), batch_mask=mask.double())
    ld64["total_loss"].backward()
    _, ld = m(x.to(DEV), time_matching_mat=tm.to(DEV), batch_mask=mask.to(DEV))
    ld["total_loss"].backward()
    for k in ("recon_loss", "commitment_loss", "time_matching_loss", "total_loss"):
        assert abs(float(ld[k]) - float(ld_r[k])) <= 1e-5 * max(1.0, abs(float(ld_r[k]))), (k, float(ld[k]), float(ld_r[k]))
    ref2 = O.OracleVQVAEz32()
    ref2.load_state_dict(ref.state_dict())       # BatchNorm buffers moved in the call above: fine for the index check
    g32, g64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    for k, p in m.named_parameters():
        if not p.requires_grad or k in Z32_BN_FED_BIASES:
            continue
        truth = g64[k].grad
        scale = max(truth.abs().max().item(), 1e-6)
        e_ref = (g32[k].grad.double() - truth).abs().max().item()
        e_hip = (p.grad.cpu().double() - truth).abs().max().item()
        assert e_hip <= max(1.5 * e_ref, 5e-4 * scale) + 1e-9, (k, e_hip, e_ref, scale)


@pytest.mark.parametrize("B,nin,hw,masked", [(1, 2, 128, False), (3, 1, 128, True), (5, 3, 128, False), (2, 4, 256, True),
                                             (7, 2, 128, True)])
def test_shape_sweep_losses_and_gradients(B, nin, hw, masked):
    """Odd batches, 1-4 input channels, 128 and 256 pixel patches: losses and a few gradients vs the CPU oracle
    (the unfused decoder tail and the first-layer kernels for every num_inputs are exercised here)."""
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    torch.manual_seed(1000 + B * 10 + nin)
    kw = dict(num_inputs=nin, channel_var=np.linspace(0.5, 1.5, nin))
    ref = O.OracleVQVAE(**kw)
    x = torch.randn(B, nin, hw, hw, generator=torch.Generator().manual_seed(B))
    mask = ((torch.rand(B, 1, hw, hw, generator=torch.Generator().manual_seed(B + 1)) > 0.5).float() if masked else None)
    m = dynamorph_amd.VQ_VAE(**kw).to(DEV)
    m.load_state_dict(ref.state_dict())
    ld_r, g32, g64 = oracle_truth(ref, x, batch_mask=mask)
    dec, ld = m(x.to(DEV), batch_mask=None if mask is None else mask.to(DEV))
    ld["total_loss"].backward()
    assert dec.shape == x.shape
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        loss_gate(ld[k], ld_r[k], k)
    # every parameter gradient against the float64 yardstick (a code chosen differently at a near-tie moves the
    # gradients discretely at these batch sizes: the reference's own fp32-vs-float64 error then widens the gate by itself)
    grad_gate(m, g32, g64, skip=BN_FED_BIASES, floor=5e-4, what=f"shape sweep B={B} nin={nin} hw={hw}")


@pytest.mark.parametrize("nin", [1, 3])
def test_z32_other_input_channel_counts(nin):
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    torch.manual_seed(500 + nin)
    kw = dict(num_inputs=nin, channel_var=np.ones(nin))
    ref = O.OracleVQVAEz32(**kw)
    x = torch.randn(3, nin, 128, 128, generator=torch.Generator().manual_seed(nin))
    m = dynamorph_amd.VQ_VAE_z32(**kw).to(DEV)
    m.load_state_dict(ref.state_dict())
    ld_r, g32, g64 = oracle_truth(ref, x)
    _, ld = m(x.to(DEV))
    ld["total_loss"].backward()
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        loss_gate(ld[k], ld_r[k], k)
    grad_gate(m, g32, g64, skip=Z32_BN_FED_BIASES, floor=5e-4, what=f"z32 nin={nin}")


@pytest.mark.parametrize("B,nin,masked,use_graph,hw", [(5, 1, True, False, 128), (3, 4, True, True, 128), (6, 3, False, True, 128),
                                                       # 256-pixel patches: the decoder tail in 64-column tiles with seam terms,
                                                       # the residual 3 x 3 backward in bands of the 32 x 32 latents
                                                       (2, 4, True, True, 256), (3, 2, False, False, 256)])
def test_fused_trainer_shape_sweep(B, nin, masked, use_graph, hw):
    """FusedTrainer (training tail in one kernel, slab codebook gradient, counted Adam) vs the oracle's
    model(x) / backward / torch.optim.Adam.step for other channel counts, odd batches, masks and patch sizes."""
    import dynamorph_amd
    from dynamorph_amd.train import FusedTrainer
    from oracle import vqvae_oracle as O
    torch.manual_seed(2000 + nin)
    kw = dict(num_inputs=nin, channel_var=np.linspace(0.7, 1.3, nin))
    ref = O.OracleVQVAE(**kw)
    m = dynamorph_amd.VQ_VAE(**kw).to(DEV)
    m.load_state_dict(ref.state_dict())
    x = torch.randn(B, nin, hw, hw, generator=torch.Generator().manual_seed(B))
    mask = ((torch.rand(B, 1, hw, hw, generator=torch.Generator().manual_seed(B + 7)) > 0.4).float() if masked else None)
    opt = O.make_adam(ref, 1e-4)
    tr = FusedTrainer(m, lr=1e-4, use_graph=use_graph)
    xd, md = x.to(DEV), (None if mask is None else mask.to(DEV))
    for step in range(2):
        kw2 = {} if mask is None else {"batch_mask": mask}
        ld_r = O.train_step(ref, opt, x, **kw2)
        vals = tr.step(xd, md).tolist()
        for i, k in enumerate(("recon_loss", "commitment_loss", "total_loss")):
            assert abs(vals[i] - float(ld_r[k])) <= 3e-5 * max(1.0, abs(float(ld_r[k]))), (step, k, vals[i], float(ld_r[k]))
    sd_r = ref.state_dict()
    for k, v in m.state_dict().items():
        if k in BN_FED_BIASES or "tracked" in k:
            continue
        # two Adam steps move every weight by at most 2*lr; compare the positions, not the noise-level directions
        close(v, sd_r[k], 0, 2.5e-4 if "running" not in k else 2e-5, k)


@pytest.mark.parametrize("H,W", [(128, 256), (256, 128)])
def test_non_square_patches(H, W):
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    torch.manual_seed(4242)
    ref = O.OracleVQVAE()
    x = torch.randn(2, 2, H, W, generator=torch.Generator().manual_seed(H + W))
    m = dynamorph_amd.VQ_VAE().to(DEV)
    m.load_state_dict(ref.state_dict())
    with torch.no_grad():
        import copy
        dec_r = copy.deepcopy(ref)(x)[0]
    ld_r, g32, g64 = oracle_truth(ref, x)
    dec, ld = m(x.to(DEV))
    ld["total_loss"].backward()
    close(dec, dec_r, 2e-4, 2e-4, "decoded")
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        loss_gate(ld[k], ld_r[k], k)
    grad_gate(m, g32, g64, skip=BN_FED_BIASES, floor=5e-4, what=f"non-square {H}x{W}")


@pytest.mark.parametrize("nlayers,K", [(1, 64), (3, 100), (0, 7)])
def test_other_residual_depths_and_codebook_sizes(nlayers, K):
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    torch.manual_seed(77 + nlayers)
    kw = dict(num_residual_layers=nlayers, num_embeddings=K)
    ref = O.OracleVQVAE(**kw)
    x = torch.randn(3, 2, 128, 128, generator=torch.Generator().manual_seed(nlayers))
    m = dynamorph_amd.VQ_VAE(**kw).to(DEV)
    m.load_state_dict(ref.state_dict())
    ld_r, g32, g64 = oracle_truth(ref, x)
    _, ld = m(x.to(DEV))
    ld["total_loss"].backward()
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        loss_gate(ld[k], ld_r[k], k)
    skip = tuple(b for b in BN_FED_BIASES if "layers" not in b) + tuple(
        f"enc.12.layers.{i}.{j}.bias" for i in range(nlayers) for j in (1, 4))
    grad_gate(m, g32, g64, skip=skip, floor=5e-4, what=f"{nlayers} residual layers, K={K}")


WIDE = [("VQ_VAE", dict(num_hiddens=32, num_residual_hiddens=32)),
        ("VQ_VAE", dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512)),     # the reference's example config
        ("VQ_VAE", dict(num_hiddens=128, num_residual_hiddens=16, num_embeddings=32)),     # dec.6 without a fused head
        ("VQ_VAE_z32", dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512))]


@pytest.mark.parametrize("name,kw", WIDE, ids=[f"{n}-{k['num_hiddens']}" for n, k in WIDE])
def test_other_channel_widths(name, kw):
    """Widths without an MFMA instantiation run on the generic kernels (conv_generic.hip) with the same results:
    every parameter gradient and the losses against the oracle's autograd."""
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    torch.manual_seed(31 + kw["num_hiddens"])
    # yardstick: the oracle in float64 (the fp32 oracle's own gradients wander by percents from it at these widths,
    # where one ReLU/BatchNorm rounding flips a gate; the HIP path stays within 1e-5 of the float64 result)
    ref = (O.OracleVQVAEz32 if name == "VQ_VAE_z32" else O.OracleVQVAE)(**kw).double()
    m = getattr(dynamorph_amd, name)(**kw).to(DEV)
    m.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    ref.load_state_dict({k: v.double() for k, v in m.state_dict().items()})     # identical (fp32-rounded) weights
    x = torch.randn(2, 2, 128, 128, generator=torch.Generator().manual_seed(8))
    mask = (torch.rand(2, 1, 128, 128, generator=torch.Generator().manual_seed(9)) > 0.3).float()
    # ReLU gates the float64 run decides by less than fp32 rounding can move them: count them (see the gate below)
    near_zero = []
    hooks = [mod.register_forward_hook(lambda _m, a, _o: near_zero.append(int((a[0].abs() < 4e-7 * a[0].abs().max()).sum())))
             for mod in ref.modules() if isinstance(mod, torch.nn.ReLU)]
    dec_r, ld_r = ref(x.double(), batch_mask=mask.double())
    for h in hooks:
        h.remove()
    ld_r["total_loss"].backward()
    dec, ld = m(x.to(DEV), batch_mask=mask.to(DEV))
    ld["total_loss"].backward()
    close(dec, dec_r, 1e-4, 1e-4, "decoded")
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        assert abs(float(ld[k]) - float(ld_r[k])) <= 1e-5 * max(1.0, abs(float(ld_r[k]))), (k, float(ld[k]), float(ld_r[k]))
    g_ref = dict(ref.named_parameters())
    rel = {}
    for k, p in m.named_parameters():
        b = g_ref[k].grad
        if b is None or not p.requires_grad:
            continue
        if b.abs().max().item() < 1e-9:               # bias in front of a train-mode BatchNorm: exactly 0
            assert p.grad is None or p.grad.abs().max().item() < 1e-6, k
            continue
        rel[k] = (p.grad.cpu().double() - b).abs().max().item() / b.abs().max().item()
    assert len(rel) >= 20
    # Exact kernels agree with float64 to ~1e-6: most parameters tight.
    tight = [k for k, e in rel.items() if e <= 2e-4]
    assert len(tight) >= 0.5 * len(rel), sorted(rel.items(), key=lambda kv: -kv[1])[:5]
    # The rest on the float64 yardstick with the reference's own fp32 error as the measure (conftest.grad_gate), floor 1e-3 of
    # the tensor's scale (until round 5 a flat 5e-2, which a dropped tap at B = 2 could hide under).  The one thing that
    # legitimately exceeds it: a ReLU gate whose pre-activation lies within fp32 rounding of zero opens in one fp32
    # implementation and stays shut in float64 (or the reverse), which moves the small-batch gradients upstream of it by up
    # to a percent or two.  The float64 run COUNTS such pre-activations (|x| below 4e-7 of the layer's largest); each of
    # them widens the floor by 5e-3 (the old flat 5e-2 is the cap).
    fragile = sum(near_zero)
    assert len(near_zero) >= 5
    print(f"{name} {kw['num_hiddens']}: {fragile} ReLU inputs within fp32 rounding of zero in the float64 run")
    ref32 = (O.OracleVQVAEz32 if name == "VQ_VAE_z32" else O.OracleVQVAE)(**kw)
    ref32.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    _, ld32 = ref32(x, batch_mask=mask)
    ld32["total_loss"].backward()
    g32 = {k: p.grad for k, p in ref32.named_parameters() if p.grad is not None}
    g64 = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    zero = [k for k, b in g64.items() if b.abs().max().item() < 1e-9]
    grad_gate(m, g32, g64, skip=zero, factor=1.5, floor=min(5e-2, 1e-3 + 5e-3 * fragile), what=f"{name} {kw['num_hiddens']}")


def test_fused_trainer_reference_example_width():
    """FusedTrainer (graph replay, flat Adam) on num_hiddens 64 / K 512: two steps against the oracle + torch Adam."""
    import dynamorph_amd
    from dynamorph_amd.train import FusedTrainer
    from oracle import vqvae_oracle as O
    kw = dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512)
    torch.manual_seed(640)
    ref = O.OracleVQVAE(**kw)
    m = dynamorph_amd.VQ_VAE(**kw).to(DEV)
    m.load_state_dict(ref.state_dict())
    opt = O.make_adam(ref, 1e-4)
    tr = FusedTrainer(m, lr=1e-4, use_graph=True)
    for step in range(2):
        x = torch.randn(2, 2, 128, 128, generator=torch.Generator().manual_seed(50 + step))
        opt.zero_grad()
        _, ld_r = ref(x)
        ld_r["total_loss"].backward()
        opt.step()
        vals = tr.step(x.to(DEV)).tolist()             # (recon, commitment, total, perplexity)
        assert abs(vals[2] - float(ld_r["total_loss"])) <= 5e-5 * max(1.0, abs(float(ld_r["total_loss"])))
    sd, sd_r = m.state_dict(), ref.state_dict()
    for k in ("dec.6.weight", "dec.4.weight", "enc.0.weight", "enc.10.weight", "vq.w.weight"):
        assert (sd[k].cpu() - sd_r[k]).abs().max().item() <= 2.5e-4, k      # at most lr per step where Adam saturates


@pytest.mark.parametrize("z16,use_graph", [(False, False), (True, True)])
def test_fused_trainer_time_matching(z16, use_graph):
    """FusedTrainer with the pairwise time-matching term (always on in the real run_training.py loop):
    vq_vae.py:324-332 / vae.py:322-336 through dm_pair_msd(_backward), vs the oracle's autograd + Adam."""
    import dynamorph_amd
    from dynamorph_amd.train import FusedTrainer
    from oracle import vqvae_oracle as O
    torch.manual_seed(909)
    ref = O.OracleVQVAE(variant="z16") if z16 else O.OracleVQVAE()
    m = (dynamorph_amd.VQ_VAE_z16 if z16 else dynamorph_amd.VQ_VAE)().to(DEV)
    m.load_state_dict(ref.state_dict())
    B = 6
    x = torch.randn(B, 2, 128, 128, generator=torch.Generator().manual_seed(5))
    tm = torch.randint(0, 3, (B, B), generator=torch.Generator().manual_seed(6)).float()
    opt = O.make_adam(ref, 1e-4)
    twin = FusedTrainer(copy.deepcopy(m), lr=1e-4, use_graph=not use_graph)     # the other of eager / captured
    tr = FusedTrainer(m, lr=1e-4, use_graph=use_graph)
    graphed = tr if use_graph else twin
    graphed.prepare(x.to(DEV), None, tm.to(DEV))
    key = ((B, 2, 128, 128), None, (B, B))
    prog = graphed._graphs[key]["train"]
    assert len(prog[0].graphs) == 1 and not prog[0].after          # ONE graph, one replay
    for step in range(2):
        ld_r = O.train_step(ref, opt, x, time_matching_mat=tm)
        out = tr.step(x.to(DEV), None, tm.to(DEV))
        assert torch.equal(out, twin.step(x.to(DEV), None, tm.to(DEV))), step
        vals = out.tolist()
        assert len(vals) == 5
        for i, k in ((0, "recon_loss"), (1, "commitment_loss"), (2, "total_loss"), (4, "time_matching_loss")):
            assert abs(vals[i] - float(ld_r[k])) <= 3e-5 * max(1.0, abs(float(ld_r[k]))), (step, k, vals[i], float(ld_r[k]))
    assert graphed._graphs[key]["train"] is prog                    # prepare() captured what step() replays
    sd_r, sd_t = ref.state_dict(), twin.model.state_dict()
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd_t[k]), k
        if k in BN_FED_BIASES or "tracked" in k:
            continue
        close(v, sd_r[k], 0, 2.5e-4 if "running" not in k else 2e-5, k)
    assert torch.equal(tr.m, twin.m) and torch.equal(tr.v, twin.v)


def test_captured_step_follows_the_relation_matrix_between_sparse_and_dense():
    """The pairwise term chooses its form on the device (related pairs counted per call: sparse up to 32 per row, else the
    dense products), so ONE captured step serves whatever matrix the feed writes into its buffer: a graph replayed with a
    sparse, then a dense, then a sparse matrix again ends bit-equal to the eager trainer on the same sequence."""
    import copy
    import dynamorph_amd
    from dynamorph_amd.train import FusedTrainer
    torch.manual_seed(4)
    m_g = dynamorph_amd.VQ_VAE().to(DEV)
    m_e = copy.deepcopy(m_g)
    B = 72
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(B, 2, 128, 128, generator=g).to(DEV) for _ in range(3)]
    sparse = torch.zeros(B, B)
    for i in range(B - 1):
        if i % 8 != 7:
            sparse[i, i + 1] = sparse[i + 1, i] = 2.0
    dense = (torch.rand(B, B, generator=g) < 0.7).float() * torch.randint(1, 3, (B, B), generator=g).float()    # ~50 per row
    assert int((dense != 0).sum()) > 32 * B >= int((sparse != 0).sum())
    tms = [sparse.to(DEV), dense.to(DEV), sparse.to(DEV)]
    tg, te = FusedTrainer(m_g, lr=1e-4, use_graph=True), FusedTrainer(m_e, lr=1e-4, use_graph=False)
    for x, tm in zip(xs, tms):
        vg, ve = tg.step(x, None, tm), te.step(x, None, tm)
        assert torch.equal(vg, ve), (vg.tolist(), ve.tolist())
    for (k, a), (_, b) in zip(m_g.state_dict().items(), m_e.state_dict().items()):
        assert torch.equal(a, b), k


def test_wide_family_streaming_kernels_against_the_tiled_kernels(tmp_path):
    """The example configuration's step through round 6's kernels (wide_stream.hip, wgrad_wide1_kernel) and through the tiled
    kernels of rounds 1-5 (DM_WIDE_STREAM=0 DM_WIDE_WGRAD1=0; the switches are read once per process, hence two child
    processes): same losses to 1e-6, every gradient and BatchNorm running statistic within the accumulation-order tolerance of
    the fused-against-unfused check -- the tiled kernels stay the reference implementation of the shapes the new ones take."""
    import subprocess
    import sys
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "wide_step.py")
    outs = {}
    for tag, env in (("stream", {}), ("tiled", {"DM_WIDE_STREAM": "0", "DM_WIDE_WGRAD1": "0"})):
        f = str(tmp_path / f"{tag}.pt")
        r = subprocess.run([sys.executable, helper, f], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = torch.load(f)
    a, b = outs["stream"], outs["tiled"]
    for k, v in b["losses"].items():
        assert abs(a["losses"][k] - v) <= 1e-6 * max(1.0, abs(v)), (k, a["losses"][k], v)
    assert len(b["grads"]) >= 40
    for k, g in b["grads"].items():
        scale = float(g.abs().max())
        assert float((a["grads"][k] - g).abs().max()) <= 2e-5 * scale + 1e-9, (k, float((a["grads"][k] - g).abs().max()), scale)
    for k, v in b["buffers"].items():
        assert float((a["buffers"][k] - v).abs().max()) <= 1e-6 * max(1.0, float(v.abs().max())), k


def _states_after_adam_step(m1, m2, step, lr, skip=()):
    """Two optimisers stepping the same model from the same values: after the FIRST step everything agrees to 1e-6 (same
    kernels, same gradients; the optimisers round the update an ulp apart at most).  After that Adam compounds that ulp: an
    element whose gradient nearly cancels moves by a fraction of lr in either direction (a deterministic example at the example
    widths: codebook 1e-7 apart after step 1, a BatchNorm weight 0.4 lr apart after step 2).  Later steps therefore bound the
    walk: no element further than 2.5 lr per step taken, at most 5 % of a tensor (or one element) beyond 2.5e-4."""
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        if "tracked" in k:
            assert int(sd1[k]) == int(sd2[k]) == step + 1, k
        elif k in skip:
            continue
        else:
            d = (sd1[k] - sd2[k]).abs()
            scale = max(1.0, sd1[k].abs().max().item())
            if step == 0:
                assert d.max().item() <= 1e-6 * scale, (k, d.max().item())
            else:
                far = int((d > 2.5e-4 * scale).sum())
                assert d.max().item() <= 2.5 * lr * (step + 1) * scale, (k, d.max().item())
                assert far <= max(0.05 * d.numel(), 1), (k, far, d.numel())


@pytest.mark.parametrize("kw,B,with_tm", [({}, 6, True), (dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512), 3, False)])
def test_graphed_trainer_z32_equals_eager_adam(kw, B, with_tm):
    """GraphedTrainer (the autograd step of VQ_VAE_z32 replayed as a HIP graph, capturable Adam) against the same module
    stepped eagerly with torch.optim.Adam: same losses, same parameters, same BatchNorm buffers after 3 steps, and the
    capture's warm-up leaves no trace."""
    import copy
    import dynamorph_amd
    from dynamorph_amd.train import GraphedTrainer
    torch.manual_seed(4321)
    m1 = dynamorph_amd.VQ_VAE_z32(**kw).to(DEV)
    m2 = copy.deepcopy(m1)
    opt = torch.optim.Adam(m1.parameters(), lr=1e-3)
    tr = GraphedTrainer(m2, lr=1e-3)
    mask = (torch.rand(B, 1, 128, 128, generator=torch.Generator().manual_seed(2)) > 0.4).float().to(DEV)
    for step in range(3):
        x = torch.randn(B, 2, 128, 128, generator=torch.Generator().manual_seed(10 + step)).to(DEV)
        tm = torch.randint(0, 3, (B, B), generator=torch.Generator().manual_seed(20 + step)).float().to(DEV) if with_tm else None
        _, ld = m1(x, time_matching_mat=tm, batch_mask=mask)
        ld["total_loss"].backward()
        opt.step()
        m1.zero_grad()
        vals = tr.step(x, mask, tm).tolist()
        tol = 1e-5 if step == 0 else 5e-4                  # (see _states_after_adam_step)
        for i, k in enumerate(("recon_loss", "commitment_loss", "total_loss", "perplexity")):
            assert abs(vals[i] - float(ld[k])) <= tol * max(1.0, abs(float(ld[k]))), (step, k, vals[i], float(ld[k]))
        _states_after_adam_step(m1, m2, step, 1e-3)


def test_fused_trainer_z32_against_reference_vectors(golden):
    """FusedTrainer's VQ_VAE_z32 path (no autograd: the kernels in order on flat gradient views, one slab reduction) on
    the vectors captured from the reference (g8_z32_tm.npz: mask + time matching): losses within 1e-5, every gradient
    within the accumulation noise of fp32 -- the gates of test_z32_time_matching_mask_and_gradients_against_reference."""
    import dynamorph_amd
    from dynamorph_amd.train import FusedTrainer
    g = golden("g8_z32_tm.npz")
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    m = dynamorph_amd.VQ_VAE_z32().to(DEV)
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd/")})
    tr = FusedTrainer(m, lr=1e-4, use_graph=False)
    vals = tr.forward_backward(x, torch.from_numpy(g["mask"]).to(DEV), torch.from_numpy(g["tm"]).to(DEV)).tolist()
    for i, k in ((0, "recon_loss"), (1, "commitment_loss"), (2, "total_loss"), (4, "time_matching_loss")):
        assert abs(vals[i] - float(g[k])) <= 1e-5 * max(1.0, abs(float(g[k]))), (k, vals[i], float(g[k]))
    assert abs(vals[3] - float(g["perplexity"])) <= 1e-3 * float(g["perplexity"])
    tr.expose_grads()
    n = 0
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        if k in Z32_BN_FED_BIASES:
            assert float(p.grad.abs().max()) == 0.0, k              # never written: exactly zero
            continue
        ref = g["grad/" + k]
        scale = max(float(np.abs(ref).max()), 1e-6)
        err = float((p.grad.cpu() - torch.from_numpy(ref)).abs().max())
        assert err <= 4e-3 * scale + 1e-8, (k, err, scale)
        n += 1
    assert n >= 30


@pytest.mark.parametrize("family,masked,with_tm", [("VQ_VAE", False, False), ("VQ_VAE", True, True), ("VQ_VAE_z16", True, True),
                                                   ("VQ_VAE_z32", True, True)])
def test_gradient_with_respect_to_the_input_patches(family, masked, with_tm):
    """d(total_loss) / d(inputs) -- what autograd answers on the reference when a caller asks (saliency maps; its training never
    does): the encoder's path (the data gradient of the first convolution) plus the reconstruction loss' own dependence on
    the inputs, against the oracle's autograd on the float64 yardstick."""
    import copy
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    torch.manual_seed(91)
    ref = (O.OracleVQVAEz32 if family == "VQ_VAE_z32" else O.OracleVQVAE)(**({"variant": "z16"} if family == "VQ_VAE_z16" else {}))
    B = 3
    x = torch.randn(B, 2, 128, 128, generator=torch.Generator().manual_seed(92))
    kw = {}
    if masked:
        kw["batch_mask"] = (torch.rand(B, 1, 128, 128, generator=torch.Generator().manual_seed(93)) > 0.35).float()
    if with_tm:
        kw["time_matching_mat"] = torch.tensor([[2., 1., 0.], [1., 2., 1.], [0., 1., 2.]])
    m = getattr(dynamorph_amd, family)().to(DEV)
    m.load_state_dict(ref.state_dict())
    # a code that differs at a reference near-tie (conftest.codes_gate admits nothing else) changes the gradient around that
    # position discretely: the yardsticks are then evaluated with the HIP path's codes (OracleVQ.force_idx)
    with torch.no_grad():
        probe, mp = copy.deepcopy(ref), copy.deepcopy(m)
        z_r = probe.enc(x)
        idx_r = probe.vq.encode_inputs(z_r)
        idx = mp.vq.encode_inputs(mp.enc(x.to(DEV))).cpu()
    codes_gate(idx != idx_r, z_r, probe.vq.w.weight.detach(), f"{family}, input gradient")
    if bool((idx != idx_r).any()):
        ref.vq.force_idx = idx.clone()
    grads = {}
    near_zero = []                                      # ReLU inputs the float64 run decides by less than fp32 rounding can move
    for tag, model, cast in (("f32", ref, torch.float32), ("f64", copy.deepcopy(ref).double(), torch.float64)):
        hooks = [mod.register_forward_hook(lambda _m, a, _o: near_zero.append(int((a[0].abs() < 4e-7 * a[0].abs().max()).sum())))
                 for mod in model.modules() if isinstance(mod, torch.nn.ReLU)] if tag == "f64" else []
        xi = x.detach().clone().to(cast).requires_grad_(True)
        _, ld = model(xi, **{k: v.to(cast) for k, v in kw.items()})
        for h in hooks:
            h.remove()
        ld["total_loss"].backward()
        grads[tag] = xi.grad
    xd = x.detach().to(DEV).requires_grad_(True)
    _, ld = m(xd, **{k: v.to(DEV) for k, v in kw.items()})
    ld["total_loss"].backward()
    assert xd.grad is not None and xd.grad.shape == x.shape
    truth = grads["f64"]
    scale = truth.abs().max().item()
    e_ref = (grads["f32"].double() - truth).abs().max().item()
    e_hip = (xd.grad.cpu().double() - truth).abs().max().item()
    fragile = sum(near_zero)
    err = (xd.grad.cpu().double() - truth).abs()
    tight = max(1.5 * e_ref, 2e-4 * scale) + 1e-12
    off = int((err > tight).sum())
    print(f"{family}: input gradient scale {scale:.2e}, error of the HIP path {e_hip:.2e}, of the fp32 reference {e_ref:.2e}; "
          f"{off} of {err.numel()} elements beyond {tight:.1e}, {fragile} ReLU inputs within fp32 rounding of zero")
    # everything tight -- except around a ReLU gate that fp32 rounding can flip (the float64 run counts the candidates): such a
    # gate changes the input gradient inside ITS receptive field only (at most 64 x 64 pixels x 2 channels) and by a few percent
    assert scale > 0 and off <= 8192 * fragile and e_hip <= (5e-2 * scale if fragile else tight), (family, e_hip, e_ref, scale, off, fragile)
    # and the parameters' gradients are what they are without the input gradient
    m2 = getattr(dynamorph_amd, family)().to(DEV)
    m2.load_state_dict(ref.state_dict())
    _, ld2 = m2(x.to(DEV), **{k: v.to(DEV) for k, v in kw.items()})
    ld2["total_loss"].backward()
    for (k, p), (_, q) in zip(m.named_parameters(), m2.named_parameters()):
        if p.grad is not None:
            assert torch.equal(p.grad, q.grad), k


@pytest.mark.parametrize("family", ["VQ_VAE", "VQ_VAE_z16", "VQ_VAE_z32"])
def test_backward_in_eval_mode(family):
    """model.eval(); total_loss.backward() -- the reference's training never leaves train mode (run_training.py:522-531 even
    validates in it), autograd there would answer: every BatchNorm normalises with its running statistics, whose backward is
    dx = gamma / sqrt(running_var + eps) * dy with the usual weight / bias sums (dm_bn_backward_finalize, count 0).  Against
    the oracle in eval() mode on the float64 yardstick, running statistics moved off their initial values by two training
    forwards first; the running statistics stay what they were."""
    import copy
    import dynamorph_amd
    from conftest import grad_gate, loss_gate, oracle_truth
    from oracle import vqvae_oracle as O
    torch.manual_seed(95)
    ref = (O.OracleVQVAEz32 if family == "VQ_VAE_z32" else O.OracleVQVAE)(**({"variant": "z16"} if family == "VQ_VAE_z16" else {}))
    B = 4
    gen = torch.Generator().manual_seed(96)
    with torch.no_grad():
        for _ in range(2):
            ref(torch.randn(B, 2, 128, 128, generator=gen) * 1.3 + 0.2)
    x = torch.randn(B, 2, 128, 128, generator=gen)
    ref.eval()
    m = getattr(dynamorph_amd, family)().to(DEV)
    m.load_state_dict(ref.state_dict())
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items() if "running" in k or "num_batches" in k}
    with torch.no_grad():
        probe = copy.deepcopy(ref)
        z_r = probe.enc(x)
        idx_r = probe.vq.encode_inputs(z_r)
        idx = m.vq.encode_inputs(m.enc(x.to(DEV))).cpu()
    codes_gate(idx != idx_r, z_r, probe.vq.w.weight.detach(), f"{family}, eval mode")
    if bool((idx != idx_r).any()):
        ref.vq.force_idx = idx.clone()
    ld_ref, g32, g64 = oracle_truth(ref, x)
    _, ld = m(x.to(DEV))
    ld["total_loss"].backward()
    for k in ("recon_loss", "commitment_loss", "total_loss"):
        loss_gate(ld[k], ld_ref[k], f"{family} eval {k}")
    n = grad_gate(m, g32, g64, what=f"{family}, eval mode", factor=2.0)
    assert n >= 30
    for k, v in m.state_dict().items():
        if k in before:
            assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("use_graph", [False, True])
def test_fused_trainer_z32_with_extra_losses_against_reference_vectors(golden, use_graph):
    """FusedTrainer on a VQ_VAE_z32 with extra_loss (vae.py:463-469): the caller's torch functions run on z_after between the
    forward and the backward half of the step (two captured graphs with use_graph) -- losses and every gradient against the
    vectors captured from the reference's class (g8_z32_extra.npz); then run_one_batch with the labels in model_kwargs, the
    way train_with_loader hands them over (run_training.py:596-599)."""
    import os
    import sys
    import dynamorph_amd
    from dynamorph_amd.train import FusedTrainer, run_one_batch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
    from extra_losses import EXTRA
    g = golden("g8_z32_extra.npz")
    x = torch.from_numpy(golden("g2_input.npz")["x"]).to(DEV)
    labels, tm = torch.from_numpy(g["labels"]).to(DEV), torch.from_numpy(g["tm"]).to(DEV)
    m = dynamorph_amd.VQ_VAE_z32(extra_loss=dict(EXTRA), alpha=float(g["alpha"])).to(DEV)
    m.load_state_dict({k[3:]: torch.from_numpy(np.asarray(v)) for k, v in g.items() if k.startswith("sd/")})
    tr = FusedTrainer(m, lr=1e-4, use_graph=use_graph)
    m2 = dynamorph_amd.VQ_VAE_z32(extra_loss=dict(EXTRA), alpha=float(g["alpha"])).to(DEV)
    m2.load_state_dict(m.state_dict())
    twin = FusedTrainer(m2, lr=1e-4, use_graph=not use_graph)     # the other of eager / captured
    graphed = tr if use_graph else twin
    graphed.prepare(x, None, tm)
    key = (tuple(x.shape), None, tuple(tm.shape))
    prog = graphed._graphs[key]["train"]
    assert len(prog[0].graphs) == 2                               # cut once, at the extra losses
    for rep in range(2):                                    # (the second call replays the captured pair)
        tr.grad.zero_()
        twin.grad.zero_()
        out = tr._step_with_extra_losses(x, None, tm, labels)
        assert torch.equal(out, twin._step_with_extra_losses(x, None, tm, labels)), rep
        assert torch.equal(tr.grad, twin.grad), rep
        for name in EXTRA:
            assert torch.equal(tr.last_extra_losses[name], twin.last_extra_losses[name]), (rep, name)
        vals = out.tolist()
        for i, k in ((0, "recon_loss"), (1, "commitment_loss"), (2, "total_loss"), (4, "time_matching_loss")):
            loss_gate(vals[i], float(g["loss/" + k]), f"fused extra-loss step {k}")
        for name in EXTRA:
            loss_gate(float(tr.last_extra_losses[name]), float(g["loss/" + name]), f"fused extra-loss step {name}")
        tr.expose_grads()
        n = 0
        for k, p in m.named_parameters():
            if not p.requires_grad or k in Z32_BN_FED_BIASES:
                continue
            ref = g["grad/" + k]
            scale = max(float(np.abs(ref).max()), 1e-6)
            err = float((p.grad.cpu() - torch.from_numpy(ref)).abs().max())
            assert err <= 4e-3 * scale + 1e-8, (rep, k, err, scale)
            n += 1
        assert n >= 30
    assert graphed._graphs[key]["train"] is prog                  # prepare() captured what the steps replay
    for k, b in m2.state_dict().items():
        assert torch.equal(m.state_dict()[k], b), k
    losses = {}
    run_one_batch(m, x, losses, model_kwargs={"labels": labels, "time_matching_mat": tm}, optimizer=tr, training=True)
    assert list(losses.keys()) == [str(k) for k in g["loss_keys"]]          # vae.py:456-469: ..., total_loss, then one entry per extra loss
    with pytest.raises(AttributeError, match="alpha"):
        FusedTrainer(dynamorph_amd.VQ_VAE_z32(extra_loss=dict(EXTRA)).to(DEV))


@pytest.mark.parametrize("kw,B,with_tm,use_graph", [({}, 6, True, False), ({}, 5, True, True),
                                                    (dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512), 3, True, True)])
def test_fused_trainer_z32_equals_eager_adam(kw, B, with_tm, use_graph):
    """FusedTrainer on VQ_VAE_z32 (default widths and the reference's example widths 64 / 64 / 512) against the same module
    stepped through autograd + torch.optim.Adam (run_training.py:404-408, 485), with a mask and the time-matching matrix, 3 steps
    at lr 1e-3.  The first step is held tightly: same losses (1e-5) and the same parameters / BatchNorm buffers to 1e-6 -- both
    paths run the same kernels on the same values.  After that Adam compounds what separates them: the two optimisers round the
    codebook's first update 1 ulp apart (1e-7), and a BatchNorm weight whose gradient nearly cancels turns that into 0.4 lr one
    step later (found as a DETERMINISTIC case once the large-codebook gradient stopped varying from launch to launch; before, the
    atomic order rolled the dice and one run in ten failed).  Steps 2-3 therefore bound the walk instead: no element further than
    2.5 lr per step taken, at most 5 % of a tensor (or one element) beyond 2.5e-4, losses within 5e-4."""
    import copy
    import dynamorph_amd
    from dynamorph_amd.train import FusedTrainer
    torch.manual_seed(4321)
    lr = 1e-3
    m1 = dynamorph_amd.VQ_VAE_z32(weight_matching=1.0, **kw).to(DEV)
    m2 = copy.deepcopy(m1)
    opt = torch.optim.Adam(m1.parameters(), lr=lr)
    tr = FusedTrainer(m2, lr=lr, use_graph=use_graph)
    mask = (torch.rand(B, 1, 128, 128, generator=torch.Generator().manual_seed(2)) > 0.4).float().to(DEV)

    for step in range(3):
        x = torch.randn(B, 2, 128, 128, generator=torch.Generator().manual_seed(10 + step)).to(DEV)
        tm = torch.randint(0, 3, (B, B), generator=torch.Generator().manual_seed(20 + step)).float().to(DEV) if with_tm else None
        _, ld = m1(x, time_matching_mat=tm, batch_mask=mask)
        ld["total_loss"].backward()
        opt.step()
        m1.zero_grad()
        vals = tr.step(x, mask, tm).tolist()
        tol = 1e-5 if step == 0 else 5e-4
        for i, k in enumerate(("recon_loss", "commitment_loss", "total_loss", "perplexity")):
            assert abs(vals[i] - float(ld[k])) <= tol * max(1.0, abs(float(ld[k]))), (step, k, vals[i], float(ld[k]))
        if with_tm:
            assert abs(vals[4] - float(ld["time_matching_loss"])) <= tol * max(1.0, abs(float(ld["time_matching_loss"])))
        _states_after_adam_step(m1, m2, step, lr, skip=Z32_BN_FED_BIASES)
