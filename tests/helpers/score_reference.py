"""Float64 reference of the per-patch scores (dynamorph_amd.patch_vae.score_patches): what the reference's
`model(x[i:i+1], batch_mask=m[i:i+1])` puts into its loss dict, from the tensors of that call.  Restated from
HiddenStateExtractor/vq_vae.py:74-82 (the quantiser's loss and perplexity) and :320-323, 333 (masked reconstruction loss,
total) -- nothing here calls the library.  Pure CPU; tests/test_score_host.py holds it to the oracle's own batch-of-one loop.
"""
import numpy as np
import torch


def score_ref(decoded, x, mask, channel_var, z, idx, codebook, cc, weight_recon=1.0, weight_commitment=1.0):
    """decoded, x (N, C, H, W); mask None, (N, 1, H, W) or (N, C, H, W); channel_var C values; z (N, D, h, w) the latents
    before the quantiser; idx (N, h, w) its codes; codebook (K, D).  Returns a dict of float64 / int64 numpy arrays:
    recon_loss (N,), recon_loss_per_channel (N, C), commitment_loss (N,), mse (N,), perplexity (N,), total_loss (N,),
    code_counts (N, K)."""
    d = lambda t: torch.as_tensor(np.asarray(t.detach().cpu()) if torch.is_tensor(t) else np.asarray(t)).double()   # noqa: E731
    dec, X, Z, cb = d(decoded), d(x), d(z), d(codebook)
    var = d(channel_var).reshape(1, -1, 1, 1)
    M = torch.ones_like(dec) if mask is None else d(mask).expand_as(dec)
    idx = torch.as_tensor(np.asarray(idx.cpu()) if torch.is_tensor(idx) else np.asarray(idx)).long()
    N, K = dec.shape[0], cb.shape[0]
    t = dec * M - X * M
    per_channel = (t * t / var).mean((2, 3))
    recon = per_channel.mean(1)
    q = cb[idx].permute(0, 3, 1, 2)
    mse = ((q - Z) ** 2).mean((1, 2, 3))
    commit = mse + cc * mse
    counts = torch.stack([torch.bincount(idx[i].reshape(-1), minlength=K) for i in range(N)], 0)
    p = counts.double() / idx[0].numel()
    perplexity = torch.exp(-(p * torch.log(p + 1e-10)).sum(1))
    total = weight_recon * recon + weight_commitment * commit
    out = dict(recon_loss=recon, recon_loss_per_channel=per_channel, commitment_loss=commit, mse=mse, perplexity=perplexity,
               total_loss=total, code_counts=counts)
    return {k: v.numpy() for k, v in out.items()}


def oracle_loop(ref, x, mask=None):
    """The oracle's batch-of-one loop in the mode `ref` is in: per patch the loss dict of ref(x[i:i+1], batch_mask=...), and
    the tensors of that call (decoded, z_before, idx) re-evaluated alongside.  Returns (dict of (N,) float64 arrays,
    decoded (N, C, H, W), z_before (N, D, h, w), idx (N, h, w)).  In train mode the running statistics advance by the N calls
    (the re-evaluation runs on a copy)."""
    import copy
    keys = ("recon_loss", "commitment_loss", "total_loss", "perplexity")
    rows = {k: [] for k in keys}
    decs, zs, ids = [], [], []
    with torch.no_grad():
        for i in range(x.shape[0]):
            m = None if mask is None else mask[i:i + 1]
            twin = copy.deepcopy(ref)
            dec, ld = ref(x[i:i + 1], batch_mask=m)
            z = twin.enc(x[i:i + 1])
            for k in keys:
                rows[k].append(float(ld[k]))
            decs.append(dec)
            zs.append(z)
            ids.append(twin.vq.encode_inputs(z))
    return ({k: np.asarray(v, np.float64) for k, v in rows.items()}, torch.cat(decs, 0), torch.cat(zs, 0), torch.cat(ids, 0))
