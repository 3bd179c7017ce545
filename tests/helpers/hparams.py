"""The scalar grids of the non-default-hyper-parameter tests (tests/test_hparams_host.py, tests/test_gpu_hparams.py) and the
float64 expression of the pairwise term they are held against.  The model configurations are those of
tests/golden/make_golden_hparams.py (g12_hparams.npz)."""
import numpy as np
import torch

# g12_hparams.npz, part A: config_example.yml:156-167 (VQ_VAE_z32) with vq_vae_supp.py:22's channel variances
A_KW = dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512, commitment_cost=0.25, weight_matching=100,
            margin=1, w_a=1, w_t=0.5, w_n=-0.5, channel_var=np.array([0.0475, 0.0394]))
# part B: VQ_VAE / VQ_VAE_z16 at default widths with every loss weight away from 1
B_KW = dict(commitment_cost=0.4, weight_recon=0.7, weight_commitment=1.3, channel_var=np.array([0.5, 1.5]), weight_matching=3)
B_Z16_KW = dict(w_a=0.8, w_t=0.3, w_n=-0.2, margin=0.7)
# part C: the quantiser alone
C_CCS = (0.0, 0.1, 1.0)

# Initial weights: the reference's own initialisation after torch.manual_seed(seed).  The oracle's modules are created in the
# reference's order with the reference's shapes, so the same seed gives the same state bit for bit; the fixture keeps only
# per-tensor statistics of it (sd_stat/), which the tests hold the rebuilt state against exactly.
A_SEED, A_CODEBOOK_SCALE = 1200, 1.07      # scaled codebook: unrelated pairs on both sides of the hinge (see the maker)
B_SEEDS = {"vqvae": 1210, "z16": 1211}
SAMPLES = 1024                             # elements kept per tensor: a fixed stride through the flattened tensor


def example_batch(x4):
    """Part A's 6 patches from g2_input.npz's 4: two flipped copies appended, the last one shifted by -6 (with the scaled
    codebook its latent lands beyond the hinge of the other samples)."""
    x4 = torch.as_tensor(x4)
    x = torch.cat([x4, x4[0:1].flip(-1), x4[1:2].flip(-2)], 0).contiguous()
    x[5] = x[5] - 6.0
    return x


def example_relations():
    """Part A's relation block as reorder_with_trajectories lays it out: a 3-frame and a 2-frame trajectory (adjacent
    frames 2, others 1), zeros elsewhere, the diagonal included."""
    tm = torch.zeros(6, 6)
    for a, b, v in ((0, 1, 2.), (1, 2, 2.), (0, 2, 1.), (3, 4, 2.)):
        tm[a, b] = tm[b, a] = v
    return tm


def oracle_model(part, name=None):
    """The fp32 oracle of part "A" or of part "B" (name "vqvae" / "z16") in the fixture's initial state: seeded
    construction, as the maker builds the reference's model."""
    from oracle import vqvae_oracle as O
    if part == "A":
        torch.manual_seed(A_SEED)
        m = O.OracleVQVAEz32(**A_KW)
        with torch.no_grad():
            m.vq.w.weight.mul_(A_CODEBOOK_SCALE)
        return m
    torch.manual_seed(B_SEEDS[name])
    return O.OracleVQVAE(**(dict(B_KW, variant="z16", **B_Z16_KW) if name == "z16" else B_KW))


def check_initial_state(model, g, prefix):
    """Every tensor of the state dict has exactly the statistics the reference's initial state had."""
    sd = model.state_dict()
    assert len(sd) == sum(1 for k in g if k.startswith(prefix))
    for k, v in sd.items():
        assert np.array_equal(stat(v), g[prefix + k]), k


def sample(a):
    """A fixed strided subset (at most SAMPLES elements) of the flattened array."""
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).reshape(-1)
    return a[::max(1, a.size // SAMPLES)].copy()


def stat(a):
    """(sum, sum of |a|, sum of a^2, max |a|) in float64, summed in one fixed order."""
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).reshape(-1).astype(np.float64)
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum(), np.abs(a).max()], dtype=np.float64)


def pack_mask(mask):
    return np.packbits(np.asarray(mask.cpu().numpy() if torch.is_tensor(mask) else mask) != 0)


def unpack_mask(bits, shape):
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(bits)[:n].reshape(shape).astype(np.float32))


# (w_a, w_t, w_n, margin) of the weighted-hinge form (vae.py:327-336)
TM_SETS = [
    ((1.1, 0.1, -0.5, 0.5), "default"),
    ((1.0, 0.5, -0.5, 1.0), "example"),
    ((1.0, 0.5, -0.5, 0.0), "margin0"),
    ((1.0, 0.5, -0.5, -0.2), "margin_neg"),
    ((0.3, 0.2, 0.4, 0.5), "w_n_pos"),          # every hinge live: the far-block map is dense
    ((0.0, 0.5, -0.5, 1.0), "w_a0"),
]
TM_PARAMS = [s for s, _ in TM_SETS]
TM_IDS = [i for _, i in TM_SETS]


def tm_weights(tm, w_a, w_t, w_n):
    """vae.py:327-330: relation 2 / 1 / 0 -> w_a / w_t / w_n, any other value is its own weight."""
    return torch.where(tm == 2, torch.full_like(tm, w_a),
                       torch.where(tm == 1, torch.full_like(tm, w_t), torch.where(tm == 0, torch.full_like(tm, w_n), tm)))


def tm_loss_of_sim(sim, tm, mode, w_a=0.0, w_t=0.0, w_n=0.0, margin=0.0):
    """The reference's loss on the (B, B) distance matrix: vq_vae.py:331 (mode 0) / vae.py:327-336 (mode 1)."""
    if mode == 0:
        return (sim * tm).sum()
    val = sim * tm_weights(tm, w_a, w_t, w_n)
    val = torch.where(tm == 0, torch.clamp(val + margin, min=0), val)
    return val.mean()


def tm_reference(z, tm, mode, w_a=0.0, w_t=0.0, w_n=0.0, margin=0.0, rows=None):
    """float64, differences first as the reference takes them: (loss, d loss / d z, d loss / d sim).  rows (r0, R): the
    loss is the rows' share sum_{i in rows, j} v_ij (mode 1: over B * B) instead, and the gradients are of that share."""
    B, n = z.shape
    zr = z.detach().double().cpu().requires_grad_(True)
    sim = (zr.reshape(1, B, n) - zr.reshape(B, 1, n)).pow(2).mean(2)
    sim.retain_grad()
    t = tm.detach().double().cpu()
    if rows is None:
        loss = tm_loss_of_sim(sim, t, mode, w_a, w_t, w_n, margin)
    else:
        r0, R = rows
        if mode == 0:
            v = sim * t
        else:
            v = sim * tm_weights(t, w_a, w_t, w_n)
            v = torch.where(t == 0, torch.clamp(v + margin, min=0), v) / float(B * B)
        loss = v[r0:r0 + R].sum()
    loss.backward()
    return float(loss), zr.grad, sim.grad
