"""The EMA codebook update ("Neural Discrete Representation Learning", appendix A.1) restated twice for the
tests: in numpy float64 from the raw arrays, and as a wrapper that turns the CPU oracle (oracle/vqvae_oracle.py, imported and
left as it is) into an EMA model -- frozen codebook, commitment_loss = cc * e_latent_loss, the update applied after the step
from the oracle's own latents.  Neither shares code with dynamorph_amd."""
import copy
import types

import numpy as np
import torch
import torch.nn.functional as F

# The seeds of tests/test_gpu_ema_model.py's one-step test (B = 4 on 2 x 128 x 128; torch.manual_seed(seed) builds the oracle,
# the batch is randn from a generator seeded with seed + 1): chosen on the CPU, by tests/helpers/ema_reference.py::seed_is_clean,
# so that the oracle's own fp32 and float64 codes agree at every position and no position is a near-tie at rel = 1e-4 -- one
# flipped position among the ~16 a code holds moves that code's mean by several percent, which is no rounding question.
ONE_STEP_SEEDS = {"VQ_VAE": 4102, "VQ_VAE_z16": 4200, "VQ_VAE_z32": 4318}      # (the first clean ones from 4100 / 4200 / 4300)
ONE_STEP_BATCH = 4
EMA_DECAY, EMA_EPSILON = 0.9, 1e-5


def ema_statistics_f64(z, idx, K):
    """z (B, D, H, W), idx (B, H, W) -> (n (K,), s (K, D)) in float64: counts and per-code sums of the assigned vectors, as a
    one-hot product."""
    z = np.asarray(z, dtype=np.float64)
    idx = np.asarray(idx).reshape(-1)
    D = z.shape[1]
    zf = np.transpose(z, (0, 2, 3, 1)).reshape(-1, D)
    onehot = np.zeros((idx.size, K), dtype=np.float64)
    onehot[np.arange(idx.size), idx] = 1.0
    return onehot.sum(0), onehot.T @ zf


def ema_apply_f64(n, s, N, m, decay, eps):
    """The update from the statistics: (N', m', e') in float64.  The formulae of the definition, in its order."""
    n, s, N, m = (np.asarray(a, dtype=np.float64) for a in (n, s, N, m))
    K = N.shape[0]
    N2 = decay * N + (1.0 - decay) * n
    m2 = decay * m + (1.0 - decay) * s
    tot = N2.sum()
    Nt = (N2 + eps) / (tot + K * eps) * tot
    with np.errstate(divide="ignore", invalid="ignore"):
        e2 = m2 / Nt[:, None]
    return N2, m2, e2


def ema_update_f64(z, idx, N, m, e, decay, eps):
    """(z, idx, N, m, e, decay, eps) -> (n, s, N', m', e'), everything float64 (e only fixes K)."""
    K = np.asarray(e).shape[0]
    n, s = ema_statistics_f64(z, idx, K)
    return (n, s) + ema_apply_f64(n, s, N, m, decay, eps)


def _ema_vq_forward(self, z):
    """OracleVQ.forward with the EMA mode's loss: the same indices, straight-through value and perplexity; the loss is
    commitment_cost * mse(q.detach(), z).  Keeps the step's (z, idx) for the update."""
    idx = self.encode_inputs(z) if self.force_idx is None else self.force_idx
    q = self.decode_inputs(idx)
    out = z + (q - z).detach()
    loss = self.commitment_cost * F.mse_loss(q.detach(), z)
    flat = idx.flatten()
    onehot = torch.zeros(flat.shape[0], self.num_embeddings)
    onehot.scatter_(1, flat.unsqueeze(1), 1)
    p = onehot.mean(0)
    perplexity = torch.exp(-(p * torch.log(p + 1e-10)).sum())
    self.last_z, self.last_idx = z.detach(), idx.detach()
    return out, loss, perplexity


class OracleEMA:
    """An oracle model (OracleVQVAE / OracleVQVAEz32) in the EMA codebook mode, in the model's own dtype: fp32 as built,
    float64 after .double()."""

    def __init__(self, model, decay=EMA_DECAY, eps=EMA_EPSILON):
        self.model, self.decay, self.eps = model, float(decay), float(eps)
        model.vq.w.weight.requires_grad_(False)
        model.vq.forward = types.MethodType(_ema_vq_forward, model.vq)
        w = model.vq.w.weight.detach()
        self.N = torch.ones(w.shape[0], dtype=w.dtype)
        self.m = w.clone()

    def double(self):
        other = copy.copy(self)
        other.model = copy.deepcopy(self.model).double()
        other.N, other.m = self.N.double(), self.m.double()
        return other

    @property
    def codebook(self):
        return self.model.vq.w.weight.detach()

    def state_dict(self):
        sd = dict(self.model.state_dict())
        sd["vq.ema_cluster_size"], sd["vq.ema_w"] = self.N.clone(), self.m.clone()
        return sd

    def update(self):
        """The definition's steps 1-5 from the last forward's own z and indices, in the model's dtype."""
        vq = self.model.vq
        z, idx = vq.last_z, vq.last_idx.flatten()
        K, D = vq.w.weight.shape
        zf = z.permute(0, 2, 3, 1).reshape(-1, D)
        n = torch.bincount(idx, minlength=K).to(z.dtype)
        s = torch.zeros(K, D, dtype=z.dtype).index_add_(0, idx, zf)
        g = self.decay
        self.N = g * self.N + (1.0 - g) * n
        self.m = g * self.m + (1.0 - g) * s
        tot = self.N.sum()
        Nt = (self.N + self.eps) / (tot + K * self.eps) * tot
        with torch.no_grad():
            vq.w.weight.copy_(self.m / Nt[:, None])

    def train_step(self, optimizer, batch, **model_kwargs):
        """One step of the reference's loop (run_training.py:404-408) in this mode; the gradients stay in .grad.  Returns
        (loss dict, z_before, idx) of the step."""
        self.model.zero_grad()
        _, losses = self.model(batch, **model_kwargs)
        losses["total_loss"].backward()
        if optimizer is not None:
            optimizer.step()
        vq = self.model.vq
        z, idx = vq.last_z, vq.last_idx
        self.update()
        return losses, z, idx


def near_ties(z, codebook, rel=1e-4):
    """Positions whose two best squared distances are within rel of each other (tests/conftest.py::codes_gate's notion),
    evaluated in float64: bool (B, H, W)."""
    z, codebook = torch.as_tensor(z).double(), torch.as_tensor(codebook).double()
    B, D, H, W = z.shape
    d = torch.cdist(z.permute(0, 2, 3, 1).reshape(-1, D), codebook).pow(2)
    top2 = torch.topk(d, 2, dim=1, largest=False).values
    return ((top2[:, 1] - top2[:, 0]) <= rel * top2[:, 0]).reshape(B, H, W)


def build_oracle(name, seed):
    """The oracle of model family `name` as torch.manual_seed(seed) initialises it, and the seed's batch."""
    from oracle import vqvae_oracle as O
    torch.manual_seed(seed)
    if name == "VQ_VAE_z32":
        ref = O.OracleVQVAEz32()
    else:
        ref = O.OracleVQVAE(variant="z16" if name == "VQ_VAE_z16" else "vq_vae")
    x = torch.randn(ONE_STEP_BATCH, 2, 128, 128, generator=torch.Generator().manual_seed(seed + 1))
    return ref, x


def seed_is_clean(name, seed, rel=1e-4):
    """The criterion ONE_STEP_SEEDS were chosen by (CPU only): fp32 and float64 oracle codes agree everywhere and the float64
    latents hold no near-tie at `rel`."""
    ref, x = build_oracle(name, seed)
    ref64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        z32, z64 = ref.enc(x), ref64.enc(x.double())
        i32, i64 = ref.vq.encode_inputs(z32), ref64.vq.encode_inputs(z64)
    return bool((i32 == i64).all()) and not bool(near_ties(z64, ref64.vq.w.weight.detach(), rel).any())
