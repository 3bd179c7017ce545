#!/usr/bin/env python3
"""Generate tests/golden/g12_hparams.npz by importing the reference (build container only; same rules as make_golden.py).

Every other fixture runs the reference's DEFAULT scalars.  This one holds the values its example configuration trains with
and a set of non-default loss weights, so that a scalar that is dropped, fixed or swapped on the HIP path fails a test:

  A/  VQ_VAE_z32 at config_example.yml:156-167 (64 / 64 / 512 codes, weight_matching 100, margin 1, w_a 1, w_t 0.5,
      w_n -0.5; passed through run_training.py:886-897) with vq_vae_supp.py:22's channel variances, 6 patches, a batch
      mask and a relation block shaped like reorder_with_trajectories' (a 3-frame and a 2-frame trajectory).  At the
      seeded initialisation every unrelated pair sits at sim ~ 1.8, inside the hinge (live while sim <= margin / -w_n =
      2): one patch is shifted and the codebook scaled by 1.07, so that sample's pairs lie beyond the threshold and the
      others inside it -- both sides of the hinge occur, every pair at least 0.05 from it (counts stored and asserted).
      Losses, decoded, every gradient; every gradient again with weight_matching = 0 (grad_wm0/); the losses of a second
      step after one torch.optim.Adam(lr=1e-4) step built as run_training.py:485 builds it.
  B/  vq_vae.VQ_VAE (sum form, vq_vae.py:324-332) and vae.VQ_VAE_z16 (weighted hinge, vae.py:322-336) at default widths
      with commitment_cost 0.4, weight_recon 0.7, weight_commitment 1.3, channel_var [0.5, 1.5], weight_matching 3
      (z16: w_a 0.8, w_t 0.3, w_n -0.2, margin 0.7) on g2_input.npz's patches with a mask and a relation block (VQ_VAE's
      holds a non-integer value and an entry that goes one way only).
  C/  vq_vae.VectorQuantizer (K 64, D 16) alone at commitment_cost 0, 0.1 and 1: output, loss, perplexity, dz under an
      upstream gradient and dw.

What is stored small: the patches are built from g2_input.npz (tests/helpers/hparams.py: example_batch), the masks as bits,
the initial weights as the seeds of the reference's own initialisation (which the oracle reproduces bit for bit) with
per-tensor statistics to hold the rebuilt state against; every decoded image and gradient as a fixed strided sample of at
most 1024 elements plus float64 statistics of the whole tensor (sum, sum of |.|, sum of squares, max |.|).

    DYNAMORPH_REFERENCE=<reference checkout> python3 tests/golden/make_golden_hparams.py [OUTPUT_DIR]
"""
import copy
import os
import sys
import types

REF = os.environ.get("DYNAMORPH_REFERENCE")
if not REF:
    sys.exit("make_golden_hparams.py: set DYNAMORPH_REFERENCE to a checkout of the reference")
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
sys.modules.setdefault("cv2", types.ModuleType("cv2"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import HiddenStateExtractor.vae as ref_vae  # noqa: E402
import HiddenStateExtractor.vq_vae as ref_vq  # noqa: E402
from hparams import (A_CODEBOOK_SCALE, A_KW, A_SEED, B_KW, B_SEEDS, B_Z16_KW, C_CCS, example_batch,  # noqa: E402
                     example_relations, pack_mask, sample, stat)

torch.set_num_threads(8)

def f32(t):
    return t.detach().cpu().numpy().astype(np.float32, copy=True)


def sd_stats(prefix, m):
    return {f"{prefix}{k}": stat(v) for k, v in m.state_dict().items()}


def losses(prefix, ld):
    return {f"{prefix}{k}": np.float32(float(v.detach() if torch.is_tensor(v) else v)) for k, v in ld.items()}


def grads(prefix, m):
    """grad/<name>: strided sample; grad_stat/<name>: statistics of the whole tensor."""
    out = {}
    for k, p in m.named_parameters():
        if p.grad is not None:
            out[f"{prefix}/{k}"] = sample(p.grad)
            out[f"{prefix}_stat/{k}"] = stat(p.grad)
    return out


def image(prefix, t):
    return {prefix: sample(t), prefix + "_stat": stat(t)}


arrs = {}
x4 = torch.from_numpy(np.load(os.path.join(HERE, "g2_input.npz"))["x"])             # (4, 2, 128, 128)

# ---------------------------------------------------------------- A: the example configuration
x = example_batch(x4)                   # 6 patches; with the scaled codebook the last one lies beyond the others' hinge
tm = example_relations()
mask = (torch.rand(6, 1, 128, 128, generator=torch.Generator().manual_seed(1201)) > 0.35).float()
torch.manual_seed(A_SEED)
m = ref_vae.VQ_VAE_z32(device="cpu", **A_KW)
with torch.no_grad():
    m.vq.w.weight.mul_(A_CODEBOOK_SCALE)
sd0 = sd_stats("A/sd_stat/", m)
with torch.no_grad():                   # which side of the hinge each unrelated pair lies on (a copy: BatchNorm buffers stay)
    probe = copy.deepcopy(m)
    za = probe.vq(probe.enc(x))[0].reshape(6, -1)
    sim = ((za.reshape(1, 6, -1) - za.reshape(6, 1, -1)) ** 2).mean(2)
    unrelated = (tm == 0) & ~torch.eye(6, dtype=torch.bool)
    v = sim * A_KW["w_n"] + A_KW["margin"]
    live = (v >= 0) & unrelated
    n_live, n_dead = int(live.sum()), int((unrelated & ~live).sum())
assert n_live > 0 and n_dead > 0, ("both sides of the hinge must occur", n_live, n_dead)
assert float(v[unrelated].abs().min()) > 0.05, "an unrelated pair within rounding reach of the hinge's threshold"
m_wm0 = ref_vae.VQ_VAE_z32(device="cpu", **dict(A_KW, weight_matching=0))
m_wm0.load_state_dict(m.state_dict())
dec, ld = m(x, time_matching_mat=tm, batch_mask=mask)
ld["total_loss"].backward()
_, ld0 = m_wm0(x, time_matching_mat=tm, batch_mask=mask)
ld0["total_loss"].backward()
arrs.update({"A/x_stat": stat(x), "A/tm": f32(tm), "A/mask_bits": pack_mask(mask),
             "A/hinge_live": np.int64(n_live), "A/hinge_dead": np.int64(n_dead)})
arrs.update(image("A/decoded", dec))
arrs.update(losses("A/loss/", ld))
arrs.update(grads("A/grad", m))
arrs.update(grads("A/grad_wm0", m_wm0))
arrs.update(sd0)
opt = torch.optim.Adam(m.parameters(), lr=1e-4, betas=(.9, .999))                  # run_training.py:485
opt.step()
m.zero_grad()
_, ld2 = m(x, time_matching_mat=tm, batch_mask=mask)
arrs.update(losses("A/step2/", ld2))
print("A: losses", {k: float(v) for k, v in ld.items()}, "hinge live / dead", n_live, n_dead,
      "step 2 total", float(ld2["total_loss"]))

# ---------------------------------------------------------------- B: the weighted losses at default widths
mask4 = (torch.rand(4, 1, 128, 128, generator=torch.Generator().manual_seed(1202)) > 0.3).float()
tm_sum = torch.tensor([[0., 2., 0.5, 0.], [2., 0., 1., 0.], [0.5, 1., 0., 0.], [1., 0., 0., 0.]])     # (3, 0): one way only
tm_z16 = torch.tensor([[0., 2., 1., 0.], [2., 0., 2., 0.], [1., 2., 0., 0.], [0., 0., 0., 0.]])
arrs.update({"B/mask_bits": pack_mask(mask4)})              # (the patches: g2_input.npz)
for name, cls, kw, t in (("vqvae", ref_vq.VQ_VAE, B_KW, tm_sum), ("z16", ref_vae.VQ_VAE_z16, dict(B_KW, **B_Z16_KW), tm_z16)):
    torch.manual_seed(B_SEEDS[name])
    mb = cls(device="cpu", **kw)
    arrs.update(sd_stats(f"B/{name}/sd_stat/", mb))
    dec, ld = mb(x4, time_matching_mat=t, batch_mask=mask4)
    ld["total_loss"].backward()
    arrs.update({f"B/{name}/tm": f32(t)})
    arrs.update(image(f"B/{name}/decoded", dec))
    arrs.update(losses(f"B/{name}/loss/", ld))
    arrs.update(grads(f"B/{name}/grad", mb))
    print(f"B {name}: losses", {k: float(v) for k, v in ld.items()})

# ---------------------------------------------------------------- C: the quantiser alone
gen = torch.Generator().manual_seed(1220)
z = torch.randn(3, 16, 8, 8, generator=gen) * 0.8
g_out = torch.randn(3, 16, 8, 8, generator=gen)
G_LOSS = 0.7                                            # upstream gradient of the loss: d(sum(out * g_out) + 0.7 loss)
torch.manual_seed(1221)
w0 = ref_vq.VectorQuantizer(16, 64, 0.25, device="cpu").w.weight.detach().clone()
arrs.update({"C/z": f32(z), "C/g_out": f32(g_out), "C/g_loss": np.float32(G_LOSS), "C/w": f32(w0)})
for cc in C_CCS:
    vq = ref_vq.VectorQuantizer(16, 64, cc, device="cpu")
    with torch.no_grad():
        vq.w.weight.copy_(w0)
    zi = z.clone().requires_grad_(True)
    out, loss, perp = vq(zi)
    ((out * g_out).sum() + G_LOSS * loss).backward()
    p = f"C/cc{cc:g}/"
    arrs.update({p + "out": f32(out), p + "loss": np.float32(float(loss)), p + "perplexity": np.float32(float(perp)),
                 p + "dz": f32(zi.grad), p + "dw": f32(vq.w.weight.grad)})
    print(f"C cc {cc:g}: loss {float(loss):.6f} perplexity {float(perp):.4f}")

path = os.path.join(OUT, "g12_hparams.npz")
np.savez_compressed(path, **arrs)
print(f"g12_hparams.npz {os.path.getsize(path) / 1024:.1f} KiB, {len(arrs)} arrays")
