"""Latent-encoding driver: mirror of pipeline/patch_VAE.py::process_VAE (VQ branch, lines 343-462).

The reference encodes one patch at a time (batch-of-one `model.enc` -> `model.vq` calls with the model
left in train mode, two device->host copies per patch).  Here whole batches run through the HIP
encoder with PER-SAMPLE BatchNorm statistics, which is arithmetically the same thing
 and keeps samples independent -- the property that lets the path shard over GPUs
with no collective (dynamorph_amd.dist.shard_range).
"""
import os
import pickle

import numpy as np
import torch

from . import engine as E
from .train_utils import zscore_patch


def _patch_encoder(model, L, **route):
    """encode(x) -> (z_before, cx, join) for `model` and its engine.layers_of (None: a foreign module): the HIP encoder on a
    device batch with PER-SAMPLE BatchNorm statistics; join (or None) is the pending running-statistics replay the caller joins
    after its next launches.  route: encoder_forward's latents_only=True (cx holds nothing to differentiate through) or
    replay_as_latents=True (it does)."""
    if L is None:                           # any other module: the reference's batch-of-one loop as it is
        return lambda x: (torch.cat([model.enc(x[j:j + 1]) for j in range(x.shape[0])], 0), None, None)
    if L.latent_after_vq:                   # VQ_VAE_z32: no route to choose, and its residual stack flushes the replay itself
        return lambda x: E.z32_encoder_forward(L, x, per_sample=True) + (None,)
    e1 = None                               # composite first-layer weights: once per call (the weights do not change here)

    def encode(x):
        nonlocal e1
        if e1 is None:
            e1 = E.e1_operands(L)
        z, cx = E.encoder_forward(L, x, per_sample=True, e1=e1, join=False, **route)
        return z, cx, cx.join
    return encode


def _pipelined(inputs, in_dtypes, step, device, batch_size):
    """The three-stage pinned pipeline of the inference drivers.  inputs: host tensors with the same first dimension N > 0;
    in_dtypes: the dtype each reaches the device in; step(batch tensors on the device) -> tuple of device tensors with first
    dimension n, enqueued on the current stream.  Returns one host tensor (N, ...) per output, in input order.

    Three stages in flight: batch i+1 crosses PCIe on a copy stream while batch i is computed, and the outputs of batch
    i-1 go back on a second copy stream straight into the result arrays (a synchronous .cpu() per batch would leave the
    GPU idle for both transfers: at 2 M patches/s one batch of 1024 is 0.5 ms of kernels against 134 MB in and 33 MB
    out).  Measured on the MI355X host (tools/exp/host_alloc_probe.py): DMA from / to pinned memory 53-56 GB/s, from
    pageable memory 10 GB/s, into freshly allocated pageable memory 5 GB/s (first-touch page faults).  Hence: hand
    over PINNED patches for the full rate (process_VAE does: 365 k patches/s host to host, the PCIe limit); pageable
    patches of the right dtype are copied by the runtime's own staging (this thread blocks, the queued kernels do
    not: 120 k patches/s); patches that need a dtype conversion go through two pinned staging buffers.  The result
    arrays are allocated pinned (25 GB/s to allocate) unless they exceed DM_PINNED_RESULT_BYTES (default 16 GiB; then
    pageable, pre-faulted by a parallel fill, and written by blocking copies on a helper thread)."""
    from concurrent.futures import ThreadPoolExecutor
    N = inputs[0].shape[0]
    bs = int(min(batch_size, N))
    pin_cap = int(os.environ.get("DM_PINNED_RESULT_BYTES", str(16 << 30)))
    res = None
    with torch.no_grad(), torch.cuda.device(device), ThreadPoolExecutor(1) as helper:   # (non-zero gpu ids: patch_VAE.py:422)
        compute = torch.cuda.current_stream()
        s_in, s_out = torch.cuda.Stream(), torch.cuda.Stream()
        shapes = [(bs,) + tuple(t.shape[1:]) for t in inputs]
        x_dev = [[torch.empty(sh, dtype=dt, device=device) for sh, dt in zip(shapes, in_dtypes)] for _ in range(2)]
        convert = [t.dtype != dt for t, dt in zip(inputs, in_dtypes)]
        in_pin = [[torch.empty(sh, dtype=dt, pin_memory=True) if cv else None for sh, dt, cv in zip(shapes, in_dtypes, convert)]
                  for _ in range(2)]
        ev_in = [torch.cuda.Event() for _ in range(2)]          # the batch has reached x_dev[k]
        ev_done = [torch.cuda.Event() for _ in range(2)]        # the kernels reading x_dev[k] have finished
        sent = [None, None]                                     # helper's future for the batch that last used slot k

        def hand_back(lo, n, outs, ev):
            with torch.cuda.device(device), torch.cuda.stream(s_out):
                s_out.wait_event(ev)
                for r, o in zip(res, outs):
                    r[lo:lo + n].copy_(o, non_blocking=True)    # asynchronous into pinned results; into pageable ones it
                                                                # blocks, but only this helper thread

        for it, lo in enumerate(range(0, N, bs)):
            k = it & 1
            n = min(bs, N - lo)
            if sent[k] is not None:
                sent[k].result()                                # at most two batches of outputs wait on the device
            srcs = [t[lo:lo + n] for t in inputs]
            if any(convert):
                ev_in[k].synchronize()                          # staging buffer k has left for the device
                for q, cv in enumerate(convert):
                    if cv:
                        in_pin[k][q][:n].copy_(srcs[q])         # host: the reference's .float() (patch_VAE.py:419)
                        srcs[q] = in_pin[k][q][:n]
            with torch.cuda.stream(s_in):
                s_in.wait_event(ev_done[k])                     # x_dev[k] is no longer being read (no-op the first time)
                for q, src in enumerate(srcs):
                    x_dev[k][q][:n].copy_(src, non_blocking=True)   # (pageable source: blocks this thread until it has left)
                ev_in[k].record(s_in)
            compute.wait_event(ev_in[k])
            outs = step(*[xd[:n] for xd in x_dev[k]])
            ev_done[k].record(compute)
            outs = tuple(o.reshape(n, -1) if o.dim() == 1 else o for o in outs)
            if res is None:
                pinned = sum(N * o[0].numel() * o.element_size() for o in outs) <= pin_cap
                res = []
                for o in outs:
                    shape = (N,) + tuple(o.shape[1:])
                    if pinned:
                        try:
                            res.append(torch.empty(shape, dtype=o.dtype, pin_memory=True))
                            continue
                        except RuntimeError:                    # the host refuses to pin that much: pageable results
                            pinned = False
                    res.append(torch.empty(shape, dtype=o.dtype).fill_(0))
            for o in outs:
                o.record_stream(s_out)
            sent[k] = helper.submit(hand_back, lo, n, outs, ev_done[k])
        for f in sent:
            if f is not None:
                f.result()
        s_out.synchronize()
    return res


def encode_patches(model, patches, device="cuda:0", batch_size=1024, zscore_on_device=False):
    """patches: (N, C, H, W) float tensor/array on the host.  Returns (z_before, z_after) as float32
    numpy arrays of shape (N, D*H/8*W/8), in input order (patch_VAE.py:454,459).
    zscore_on_device: `patches` are the RAW (float64) patches; each batch is z-scored per patch and channel on
    the GPU (dm_zscore_patch, double arithmetic) instead of on the host (patch_VAE.py:413-419)."""
    from . import ops
    patches = torch.as_tensor(patches)
    if patches.dim() != 4:
        raise AssertionError("dataset tensor dimension can only be 4, not {}".format(patches.dim()))
    encode, codebook = _patch_encoder(model, E.layers_of(model), latents_only=True), model.vq.w.weight
    device = torch.device(device)
    if patches.shape[0] == 0:
        return np.zeros((0, 0), np.float32), np.zeros((0, 0), np.float32)

    def step(x):
        if zscore_on_device:
            x = ops.zscore_patch(x)
        z_b, _, join = encode(x)
        z_a, _, _ = E.vq_forward(codebook, z_b, float(model.commitment_cost), want_scalars=False)
        if join is not None:
            join()                                              # the running-statistics replay ran beside the quantiser
        n = x.shape[0]
        return z_b.reshape(n, -1), z_a.reshape(n, -1)
    z_b, z_a = _pipelined([patches], [patches.dtype if zscore_on_device else torch.float32], step, device, batch_size)
    return z_b.numpy(), z_a.numpy()


SCORE_KEYS = ("recon_loss", "recon_loss_per_channel", "commitment_loss", "perplexity", "total_loss", "z_before", "z_after")


def score_patches(model, patches, masks=None, device="cuda:0", batch_size=1024, zscore_on_device=False,
                  return_decoded=False, return_code_counts=False):
    """What the reference's `model(patches[i:i+1], batch_mask=masks[i:i+1])` returns in its loss dict, for every patch, in
    batched passes (plot_scripts/recon_loss.py loops that call over 5000 single patches; process_VAE(save_output=True) over
    20).  The model is in the mode it is handed: train mode = every BatchNorm with the patch's own statistics (running
    statistics advance as N batch-of-one calls), eval mode = running statistics, as in encode_patches.
    patches (N, C, H, W) and masks (N, 1 or C, H, W) or None: host tensors / arrays.  Returns a dict of numpy arrays in input
    order: recon_loss (N,), recon_loss_per_channel (N, C), commitment_loss (N,), perplexity (N,), total_loss (N,) =
    weight_recon * recon + weight_commitment * commitment (VQ_VAE_z32: recon + commitment; a batch of one carries no
    time-matching term), z_before / z_after (N, D*h*w) exactly as encode_patches returns them, code_counts (N, K) int32
    (return_code_counts) and decoded (N, C, H, W) (return_decoded).  Every value of a patch is the same to the bit whatever
    batch_size, its position and its neighbours."""
    from . import ops
    patches = torch.as_tensor(patches)
    if patches.dim() != 4:
        raise AssertionError("dataset tensor dimension can only be 4, not {}".format(patches.dim()))
    N, C, H, W = patches.shape
    if masks is not None:
        masks = torch.as_tensor(masks)
        if masks.dim() != 4 or masks.shape[0] != N or masks.shape[1] not in (1, C) or tuple(masks.shape[2:]) != (H, W):
            raise ValueError("score_patches: masks must be (N, 1 or C, H, W) for patches (N, C, H, W); got {} for {}".format(
                tuple(masks.shape), tuple(patches.shape)))
    L = E.layers_of(model, "score_patches")
    if N == 0:
        out = {k: np.zeros((0, C) if k == "recon_loss_per_channel" else ((0, 0) if k.startswith("z_") else (0,)), np.float32)
               for k in SCORE_KEYS}
        if return_code_counts:
            out["code_counts"] = np.zeros((0, model.vq.w.weight.shape[0]), np.int32)
        if return_decoded:
            out["decoded"] = np.zeros((0, C, H, W), np.float32)
        return out
    encode, codebook = _patch_encoder(model, L, latents_only=True), L.codebook.weight
    device = torch.device(device)
    cc = float(model.commitment_cost)
    w_recon, w_commit = L.loss_weights

    def step(x, m=None):
        if zscore_on_device:
            x = ops.zscore_patch(x)
        n = x.shape[0]
        z_b, _, join = encode(x)
        z_a, idx, _ = E.vq_forward(codebook, z_b, cc, want_scalars=False)
        # (a model in the EMA codebook mode reports that mode's commitment, cc * mse, and the total built on it)
        vqs, counts = ops.vq_patch_scalars(z_b, idx, codebook.detach(), cc, want_counts=return_code_counts, ema=model.vq.ema)
        if L.latent_after_vq:    # VQ_VAE_z32: a decoder with BatchNorm, per sample; the default one scores in its fused tail
            decoded, _ = E.z32_decoder_forward(L, z_a, per_sample=True)
            sums = ops.recon_loss_per_sample(decoded, x, m, model.channel_var.detach().reshape(-1))
        else:
            decoded, sums = E.decoder_score(L, z_a, x, m, want_decoded=return_decoded)
        out = ops.score_finalize(sums, vqs, w_recon, w_commit, C * H * W)
        if join is not None:
            join()
        outs = [out, z_b.reshape(n, -1), z_a.reshape(n, -1)]
        if return_code_counts:
            outs.append(counts)
        if return_decoded:
            outs.append(decoded)
        return tuple(outs)
    inputs, dtypes = [patches], [patches.dtype if zscore_on_device else torch.float32]
    if masks is not None:
        inputs.append(masks)
        dtypes.append(torch.float32)
    res = [r.numpy() for r in _pipelined(inputs, dtypes, step, device, batch_size)]
    sc = res[0]
    out = {"recon_loss": sc[:, 0].copy(), "commitment_loss": sc[:, 1].copy(), "total_loss": sc[:, 2].copy(),
           "perplexity": sc[:, 3].copy(), "recon_loss_per_channel": sc[:, 4:].copy(), "z_before": res[1], "z_after": res[2]}
    rest = res[3:]
    if return_code_counts:
        out["code_counts"], rest = rest[0], rest[1:]
    if return_decoded:
        out["decoded"] = rest[0]
    return out


GRADIENT_KEYS = ("total_loss", "recon_loss", "commitment_loss")


def _pow2_chunks(n):
    """[(lo, hi), ...]: 0 .. n cut into runs whose lengths are the powers of two of n's binary expansion, largest first."""
    out, lo = [], 0
    while lo < n:
        size = 1 << ((n - lo).bit_length() - 1)
        out.append((lo, lo + size))
        lo += size
    return out


def patch_gradients(model, patches, masks=None, of="total_loss", device="cuda:0", batch_size=1024, zscore_on_device=False):
    """The gradient of every patch's own loss with respect to its pixels, in batched passes: patch i's array is what the
    reference's batch-of-one call leaves in x.grad for x = patches[i:i+1].requires_grad_() after
    model(x, batch_mask=masks[i:i+1])[1][of].backward().  The model is in the mode it is handed, as in score_patches: train
    mode = every BatchNorm with the patch's own statistics, forward and backward (running statistics advance as N
    batch-of-one calls), eval mode = running statistics.
    of: "total_loss" (VQ_VAE_z32: recon + commitment, as score_patches), "recon_loss", "commitment_loss", or a cotangent on
    z_before -- an array (D*h*w,) shared by all patches or (N, D*h*w) in encode_patches' flattened layout: the result is then
    the gradient of <of_i, z_before(x_i)>, the encoder alone (neither quantiser nor decoder runs).
    zscore_on_device: `patches` are the raw patches and the gradient is with respect to the z-scored patch.
    Returns float32 (N, C, H, W) in input order.  No parameter and no .grad of the model is touched; every patch's gradient is
    the same to the bit whatever batch_size, its position and its neighbours."""
    from . import ops
    from .vq_vae import _GradBag
    patches = torch.as_tensor(patches)
    if patches.dim() != 4:
        raise AssertionError("dataset tensor dimension can only be 4, not {}".format(patches.dim()))
    N, C, H, W = patches.shape
    if masks is not None:
        masks = torch.as_tensor(masks)
        if masks.dim() != 4 or masks.shape[0] != N or masks.shape[1] not in (1, C) or tuple(masks.shape[2:]) != (H, W):
            raise ValueError("patch_gradients: masks must be (N, 1 or C, H, W) for patches (N, C, H, W); got {} for {}".format(
                tuple(masks.shape), tuple(patches.shape)))
    L = E.layers_of(model, "patch_gradients")
    D, h, w = int(model.num_hiddens), H // L.latent_stride, W // L.latent_stride        # of z_before
    cot = None
    if isinstance(of, str):
        if of not in GRADIENT_KEYS:
            raise ValueError("patch_gradients: of must be one of {} or a cotangent on z_before; got {!r}".format(GRADIENT_KEYS, of))
    else:
        cot = torch.as_tensor(of)
        if tuple(cot.shape) not in ((D * h * w,), (N, D * h * w)):
            raise ValueError("patch_gradients: a cotangent on z_before must be ({0},) or (N, {0}) for patches {1}; got {2}".format(
                D * h * w, tuple(patches.shape), tuple(cot.shape)))
    if N == 0:
        return np.zeros((0, C, H, W), np.float32)
    device = torch.device(device)
    cc = float(model.commitment_cost)
    z32 = L.latent_after_vq                 # VQ_VAE_z32
    codebook = L.codebook.weight
    w_recon, w_commit = L.loss_weights
    if cot is None and of == "recon_loss":
        w_recon, w_commit = 1.0, 0.0
    elif cot is None and of == "commitment_loss":
        w_recon, w_commit = 0.0, 1.0
    var = model.channel_var.detach().reshape(1, -1, 1, 1)
    shared_cot = None
    if cot is not None and cot.dim() == 1:
        shared_cot = cot.to(device=device, dtype=torch.float32).reshape(1, D, h, w)
    encode = _patch_encoder(model, L, replay_as_latents=True)
    scalars = {}

    def scalar(v):
        """The 1-element device tensor holding v (one fill per distinct value and call)."""
        if v not in scalars:
            scalars[v] = torch.full((1,), v, dtype=torch.float32, device=device)
        return scalars[v]

    def loss_gradient(z_b, x, m, decode):
        """d(sum_i loss_i) / d z_before and the part of d / d x that does not pass through the encoder.  Per batch of n
        patches the scalar is n x the batched mean, so the loss kernels take n * weight; they form (2 / count) * scale in
        fp32, which is the same number for every n that is a power of two, so they run on power-of-two runs of the batch."""
        z_a, idx, _ = E.vq_forward(codebook, z_b, cc, want_scalars=False)
        n = x.shape[0]
        chunks = _pow2_chunks(n)
        g_zq = g_dir = None
        if w_recon != 0.0:
            g_zq, g_dir = decode(z_a, x, m, chunks)
        if w_commit == 0.0:
            return g_zq, g_dir                                  # the quantiser's straight-through gradient as it is
        g_z = torch.empty_like(z_b)
        for lo, hi in chunks:
            g_z[lo:hi], _ = ops.vq_backward_slabs(z_b[lo:hi], codebook.detach(), idx[lo:hi], None if g_zq is None else g_zq[lo:hi],
                                                  scalar((hi - lo) * w_commit), cc)
        return g_z, g_dir

    def direct(x, decoded, m):
        """d(recon_loss_i) / d x_i at fixed decoded: vq_vae.py:320-322 has the patch itself in the loss."""
        g = (x - decoded) * (2.0 / (C * H * W))
        if m is not None:
            g = g * (m * m)
        return (g / var) * scalar(w_recon).reshape(())

    def decode_default(z_a, x, m, chunks):
        g_zq, g_dir = torch.empty_like(z_a), torch.empty_like(x)
        for lo, hi in chunks:                                   # (no BatchNorm in this decoder: a run of patches is a batch)
            mm = None if m is None else m[lo:hi]
            decoded, dcx = E.decoder_forward(L, z_a[lo:hi], x[lo:hi], mm)
            g_zq[lo:hi] = E.decoder_backward(L, dcx, scalar((hi - lo) * w_recon), None, _GradBag())
            g_dir[lo:hi] = direct(x[lo:hi], decoded, mm)
        return g_zq, g_dir

    def decode_z32(z_a, x, m, chunks):
        decoded, dcx = E.z32_decoder_forward(L, z_a, per_sample=True)   # (BatchNorm per sample: the whole batch at once)
        g = torch.empty_like(decoded)
        for lo, hi in chunks:                                   # only the loss gradient runs per power-of-two run
            g[lo:hi], _ = ops.recon_loss_backward(decoded[lo:hi], x[lo:hi], None if m is None else m[lo:hi], dcx.var,
                                                  scalar((hi - lo) * w_recon))
        return E.z32_decoder_backward(L, dcx, None, g, None, want_param_grads=False), direct(x, decoded, m)

    def step(x, *rest):
        rest = list(rest)
        m = rest.pop(0) if masks is not None else None
        wt = rest.pop(0) if (cot is not None and shared_cot is None) else None
        if zscore_on_device:
            x = ops.zscore_patch(x)
        n = x.shape[0]
        z_b, cx, join = encode(x)
        g_dir = None
        if cot is not None:
            g_z = (shared_cot.expand(n, D, h, w) if wt is None else wt.reshape(n, D, h, w)).contiguous()
        else:
            g_z, g_dir = loss_gradient(z_b, x, m, decode_z32 if z32 else decode_default)     # a decoder with / without BatchNorm
        if join is not None:
            join()                                              # the running-statistics replay ran beside the loss kernels
        # (the family's encoder stage, as in _patch_encoder)
        dx = (E.z32_encoder_backward if z32 else E.encoder_backward)(L, cx, g_z, None, want_dx=True, want_param_grads=False)
        if g_dir is not None:
            dx += g_dir
        return (dx,)
    inputs, dtypes = [patches], [patches.dtype if zscore_on_device else torch.float32]
    if masks is not None:
        inputs.append(masks)
        dtypes.append(torch.float32)
    if cot is not None and shared_cot is None:
        inputs.append(cot)
        dtypes.append(torch.float32)
    return _pipelined(inputs, dtypes, step, device, batch_size)[0].numpy()


def patch_gradients_sharded(model, patches, masks=None, of="total_loss", device="cuda:0", batch_size=1024,
                            zscore_on_device=False, group=None, dst=0):
    """patch_gradients over a torch.distributed group, the twin of score_patches_sharded: rank r takes the contiguous shard
    dist.shard_range(N, r, world) (a patch's gradient does not depend on the batch it ran in; a per-patch cotangent is cut the
    same way) with no collective on the data path, and the arrays are handed over on the host to rank `dst` in rank order =
    input order; the other ranks return None."""
    from . import dist as D
    import torch.distributed as tdist
    patches = torch.as_tensor(patches)
    world = D.world_size(group)
    rank = tdist.get_rank(group) if world > 1 else 0
    N = patches.shape[0]
    lo, hi = D.shard_range(N, rank, world)
    if not isinstance(of, str):
        of = torch.as_tensor(of)
        if of.dim() == 2 and of.shape[0] == N:
            of = of[lo:hi]
    out = patch_gradients(model, patches[lo:hi], masks=None if masks is None else torch.as_tensor(masks)[lo:hi], of=of,
                          device=device, batch_size=batch_size, zscore_on_device=zscore_on_device)
    return D.gather_shards((out,), group=group, dst=dst)[0] if world > 1 else out


def encode_patches_sharded(model, patches, device="cuda:0", batch_size=1024, zscore_on_device=False, group=None, dst=0):
    """encode_patches over a torch.distributed group: patches are independent (per-sample BatchNorm statistics), so rank r
    encodes the contiguous shard dist.shard_range(N, r, world) with no collective on the data path, and the (N, D*h*w)
    results are handed over on the host to rank `dst` (the one that writes the pickles) in rank order = input order
    (patch_VAE.py:454,459 stack in file-path order); the other ranks return None.
    BatchNorm running statistics advance per rank by that rank's shard only (they are not part of the outputs)."""
    from . import dist as D
    import torch.distributed as tdist
    patches = torch.as_tensor(patches)
    world = D.world_size(group)
    rank = tdist.get_rank(group) if world > 1 else 0
    lo, hi = D.shard_range(patches.shape[0], rank, world)
    z_b, z_a = encode_patches(model, patches[lo:hi], device=device, batch_size=batch_size, zscore_on_device=zscore_on_device)
    return D.gather_shards((z_b, z_a), group=group, dst=dst) if world > 1 else (z_b, z_a)


def score_patches_sharded(model, patches, masks=None, device="cuda:0", batch_size=1024, zscore_on_device=False,
                          return_decoded=False, return_code_counts=False, group=None, dst=0):
    """score_patches over a torch.distributed group, the twin of encode_patches_sharded: rank r scores the contiguous shard
    dist.shard_range(N, r, world) (per-patch values do not depend on the batch they ran in) and the arrays are handed over on
    the host to rank `dst` in rank order = input order; the other ranks return None."""
    from . import dist as D
    import torch.distributed as tdist
    patches = torch.as_tensor(patches)
    world = D.world_size(group)
    rank = tdist.get_rank(group) if world > 1 else 0
    lo, hi = D.shard_range(patches.shape[0], rank, world)
    out = score_patches(model, patches[lo:hi], masks=None if masks is None else torch.as_tensor(masks)[lo:hi], device=device,
                        batch_size=batch_size, zscore_on_device=zscore_on_device, return_decoded=return_decoded,
                        return_code_counts=return_code_counts)
    if world == 1:
        return out
    keys = sorted(out)
    full = D.gather_shards(tuple(out[k] for k in keys), group=group, dst=dst)
    return None if full is None else dict(zip(keys, full))


def _load_well(raw_folder, sites, on_dev):
    """(well, file paths, patches) as process_VAE reads them: z-scored on the host into pinned fp32 memory, or -- on_dev --
    the raw float64 patches for dm_zscore_patch."""
    assert len(set(site[:2] for site in sites)) == 1, "Sites should be from a single well/condition"
    well = sites[0][:2]
    with open(os.path.join(raw_folder, '%s_file_paths.pkl' % well), 'rb') as f:
        fs = pickle.load(f)
    with open(os.path.join(raw_folder, '%s_static_patches.pkl' % well), 'rb') as f:
        dataset = pickle.load(f)
    if on_dev:
        dataset = torch.from_numpy(np.ascontiguousarray(np.squeeze(dataset)))       # raw float64; z-scored per batch on the GPU
    else:
        dataset = torch.from_numpy(zscore_patch(np.squeeze(dataset)))
        try:                                        # the .float() of patch_VAE.py:419, into pinned memory: the drivers
            dataset = torch.empty(dataset.shape, dtype=torch.float32, pin_memory=True).copy_(dataset)   # then run at the PCIe rate
        except RuntimeError:
            dataset = dataset.float()
    assert dataset.dim() == 4, "dataset tensor dimension can only be 4, not {}".format(dataset.dim())
    assert len(fs) == dataset.shape[0]
    return well, fs, dataset


def _load_model(config_, num_inputs, device, network_module=None):
    le = config_.latent_encoding
    if 'VAE' not in le.network:
        raise ValueError('Network {} is not available'.format(le.network))
    if network_module is None:
        from . import vq_vae as network_module
    model = getattr(network_module, le.network)(num_inputs=num_inputs,
                                                num_hiddens=le.num_hiddens,
                                                num_residual_hiddens=le.num_residual_hiddens,
                                                num_residual_layers=2,
                                                num_embeddings=le.num_embeddings,
                                                gpu=True).to(device)
    try:
        model.load_state_dict(torch.load(os.path.join(le.weights, 'model.pt'), map_location=device))
    except Exception as ex:
        print(ex)
        raise ValueError("Error in loading model weights for VQ-VAE")
    return model


def score_VAE(raw_folder, supp_folder, sites, config_, gpu=0, **kwargs):
    """Per-patch losses and code usage of a well: reads what process_VAE reads (<raw>/<well>_file_paths.pkl,
    <well>_static_patches.pkl, <weights>/model.pt) plus, with use_mask=True, <raw>/<well>_static_patches_mask.pkl (the
    training pipeline's batch_mask source); writes <raw>/<model_name>/<well>_patch_scores.pkl: score_patches' dict of arrays
    (protocol 4).  kwargs: use_mask, batch_size, zscore_on_device, return_decoded, return_code_counts, network_module."""
    le = config_.latent_encoding
    assert len(le.channels) > 0, "At least one channel must be specified"
    output_dir = os.path.join(raw_folder, os.path.basename(le.weights))
    os.makedirs(output_dir, exist_ok=True)
    on_dev = bool(kwargs.get("zscore_on_device", False))
    well, fs, dataset = _load_well(raw_folder, sites, on_dev)
    masks = None
    if kwargs.get("use_mask", False):
        with open(os.path.join(raw_folder, '%s_static_patches_mask.pkl' % well), 'rb') as f:
            masks = np.asarray(pickle.load(f))
        masks = torch.from_numpy(np.ascontiguousarray(masks.reshape((masks.shape[0], -1) + tuple(dataset.shape[2:])))).float()
    device = torch.device('cuda:%d' % gpu)
    model = _load_model(config_, dataset.shape[1], device, kwargs.get("network_module"))
    scores = score_patches(model, dataset, masks=masks, device=device, batch_size=kwargs.get("batch_size", 1024),
                           zscore_on_device=on_dev, return_decoded=bool(kwargs.get("return_decoded", False)),
                           return_code_counts=bool(kwargs.get("return_code_counts", False)))
    with open(os.path.join(output_dir, '%s_patch_scores.pkl' % well), 'wb') as f:
        pickle.dump(scores, f, protocol=4)
    return scores


def process_VAE(raw_folder, supp_folder, sites, config_, gpu=0, network_module=None, **kwargs):
    """Same contract as the reference: reads <raw>/<well>_file_paths.pkl and <well>_static_patches.pkl,
    loads <weights>/model.pt, writes <raw>/<model_name>/<well>_latent_space[_after].pkl (protocol 4)."""
    le = config_.latent_encoding
    channels = le.channels
    network = le.network
    weights_dir = le.weights
    assert len(channels) > 0, "At least one channel must be specified"
    model_path = os.path.join(weights_dir, 'model.pt')
    model_name = os.path.basename(weights_dir)
    output_dir = os.path.join(raw_folder, model_name)
    os.makedirs(output_dir, exist_ok=True)
    assert len(set(site[:2] for site in sites)) == 1, "Sites should be from a single well/condition"
    well = sites[0][:2]

    with open(os.path.join(raw_folder, '%s_file_paths.pkl' % well), 'rb') as f:
        fs = pickle.load(f)
    with open(os.path.join(raw_folder, '%s_static_patches.pkl' % well), 'rb') as f:
        dataset = pickle.load(f)
    on_dev = bool(kwargs.get("zscore_on_device", False))
    if on_dev:
        dataset = torch.from_numpy(np.ascontiguousarray(np.squeeze(dataset)))       # raw float64; z-scored per batch on the GPU
    else:
        dataset = torch.from_numpy(zscore_patch(np.squeeze(dataset)))
        try:                                        # the .float() of patch_VAE.py:419, into pinned memory: encode_patches
            dataset = torch.empty(dataset.shape, dtype=torch.float32, pin_memory=True).copy_(dataset)   # then runs at the PCIe rate
        except RuntimeError:
            dataset = dataset.float()
    assert dataset.dim() == 4, "dataset tensor dimension can only be 4, not {}".format(dataset.dim())
    assert len(fs) == dataset.shape[0]
    device = torch.device('cuda:%d' % gpu)
    if 'VAE' not in network:
        raise ValueError('Network {} is not available'.format(network))
    if network_module is None:
        from . import vq_vae as network_module
    model = getattr(network_module, network)(num_inputs=dataset.shape[1],
                                             num_hiddens=le.num_hiddens,
                                             num_residual_hiddens=le.num_residual_hiddens,
                                             num_residual_layers=2,
                                             num_embeddings=le.num_embeddings,
                                             gpu=True).to(device)
    try:
        model.load_state_dict(torch.load(model_path, map_location=device))
    except Exception as ex:
        print(ex)
        raise ValueError("Error in loading model weights for VQ-VAE")
    z_b, z_a = encode_patches(model, dataset, device=device, batch_size=kwargs.get("batch_size", 1024),
                              zscore_on_device=on_dev)
    for name, dats in (('%s_latent_space.pkl' % well, z_b), ('%s_latent_space_after.pkl' % well, z_a)):
        with open(os.path.join(output_dir, name), 'wb') as f:
            pickle.dump(dats, f, protocol=4)
    if getattr(le, "save_output", False):
        save_recon_samples(model, dataset, output_dir, device, zscored=not on_dev)
    return z_b, z_a


def save_recon_samples(model, dataset, output_dir, device, zscored=True, n_samples=20):
    """patch_VAE.py:464-489 (`save_output`): 20 samples drawn with np.random.seed(0), each reconstructed by a batch-of-one
    `model(sample)[0]` (train mode, like every call of this path) on the HIP pipeline.  The arrays go to
    <output_dir>/recon_<i>.npz (sample, output); the 2 x 2 figure recon_<i>.jpg of the reference is drawn from them when
    matplotlib is importable (plotting itself is outside the hot path: same layout, a percentile stretch for contrast)."""
    np.random.seed(0)
    random_inds = np.random.randint(0, len(dataset), (n_samples,))
    written = []
    for i in random_inds:
        sample = dataset[i:(i + 1)]
        if not zscored:                                        # raw float64 patches were handed over: z-score this one
            sample = torch.from_numpy(zscore_patch(sample.numpy()))
        sample = sample.float().to(device)
        with torch.no_grad():
            output = model(sample)[0]
        a, b = sample[0].cpu().numpy(), output[0].detach().cpu().numpy()
        path = os.path.join(output_dir, 'recon_%d.npz' % i)
        np.savez(path, sample=a, output=b)
        written.append(path)
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except Exception:
            continue

        def stretch(im, tol=1):                                # contrast limits at the tol / 100 - tol percentiles
            lo, hi = np.percentile(im, [tol, 100 - tol])
            return np.clip((im - lo) / max(hi - lo, 1e-12), 0, 1)
        fig, ax = plt.subplots(2, 2, squeeze=False)
        fig.set_size_inches((15, 10))
        ims = [a[0], b[0], a[min(1, a.shape[0] - 1)], b[min(1, b.shape[0] - 1)]]
        for axis, im, name in zip(ax.flatten(), ims, ['phase', 'phase_recon', 'im_retard', 'retard_recon']):
            axis.imshow(stretch(im), cmap='gray')
            axis.axis('off')
            axis.set_title(name, fontsize=12)
        fig.savefig(os.path.join(output_dir, 'recon_%d.jpg' % i), dpi=100, bbox_inches='tight')
        plt.close(fig)
    return written
