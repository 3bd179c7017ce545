"""Training step of the VQ-VAE path.

Two ways to train, same kernels underneath:

  * drop-in (reference call pattern, run_training.py:404-408):
        _, loss_dict = model(batch, **kwargs); loss_dict['total_loss'].backward(); optimizer.step()
    with any torch optimizer -- goes through torch.autograd (dynamorph_amd.vq_vae).

  * FusedTrainer.step(batch): the MI355X-first path.  All 43 trainable tensors are views of ONE flat
    fp32 buffer, their gradients views of a second one, so a step is
        forward kernels -> backward kernels (write straight into the flat gradient buffer)
        -> ONE RCCL all-reduce of that buffer (data parallel, one process per GPU)
        -> ONE fused Adam launch,
    no autograd bookkeeping, no host synchronisation, and the forward+backward launch sequence is
    captured into a HIP graph and replayed (hipGraph instead of a tracing compiler).

    Every route (plain, global time-matching term, extra losses, synchronized BatchNorm) is ONE step body,
    FusedTrainer._train_body: _forward | _backward_to_latent | _pairwise | _backward_from_latent.  Host work in
    the middle of the step (a collective, the caller's torch code) is a cut: inline in an eager step, left out
    in the warm-up, the end of a graph segment in the capture (_Segments).

`run_one_batch` / `train` mirror run_training.py:377-417 / :455-551 (same arguments and loop).
"""
import contextlib
import os
import types

import numpy as np
import torch

from . import dist as D
from . import engine as E
from . import ops
from .train_utils import EarlyStopping

LOSS_KEYS = ("recon_loss", "commitment_loss", "total_loss", "perplexity")
JOIN_IN_VQ = True     # False: the last residual join as its own launch (dm_apply); two tests in test_gpu_model.py monkeypatch it


class _Marks:
    """Four (stream event, host clock) pairs around the parts of one FusedTrainer.step (measurement only)."""

    def __init__(self):
        self.ev, self.t = [], []

    def __call__(self):
        import time
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append(e)
        self.t.append(time.perf_counter())


class FusedTrainer:
    """Adam(lr, betas=(.9,.999), eps=1e-8) exactly as run_training.py:485 builds it, fused."""

    def __init__(self, model, lr=1e-3, betas=(.9, .999), eps=1e-8, process_group=None, use_graph=True,
                 global_time_matching=False, sync_batchnorm=False):
        if E.layers_of(model) is None:
            raise TypeError("FusedTrainer is built for VQ_VAE / VQ_VAE_z16 / VQ_VAE_z32; train other modules with a torch optimizer")
        # (a VQ_VAE_z32 with extra_loss, vae.py:463-469: the caller's torch code runs on z_after in the middle of the step,
        # _train_body; it needs the labels: step(..., labels=...))
        self._extra = getattr(model, "extra_loss", None) is not None
        if self._extra and not hasattr(model, "alpha"):
            raise AttributeError("FusedTrainer: extra_loss needs model.alpha (vae.py:467; pass alpha= to VQ_VAE_z32)")
        self.model = model
        self._z32 = model._layers_class.latent_after_vq      # the pairwise term's latent: z_after (VQ_VAE_z32), else z_before
        self.lr, self.betas, self.eps = lr, betas, eps
        self.group = process_group
        self.world = D.world_size(process_group)
        params = [p for p in model.parameters() if p.requires_grad]
        if params[0].device.type != "cuda":
            raise RuntimeError("FusedTrainer: move the model to the GPU first (no CPU fallback)")
        # EMA codebook mode (read from the model): the codebook is frozen -- no Adam parameter, no slot in the
        # flat buffers -- and the quantiser's backward leaves the update's statistics, K * D sums and K counts, in a tail of
        # the gradient bucket: they ride the step's one all-reduce as plain sums (neither grad_weight nor Adam's 1 / world
        # touches them) and the update is one launch next to Adam.  fp32 counts: exact up to 2^24 positions per code and step.
        self._ema = bool(model.vq.ema)
        K, Dm = model.vq.w.weight.shape
        self.fp = D.FlatParams(params, tail=K * (Dm + 1) if self._ema else 0)
        self.params, self.flat, self.grad = self.fp.params, self.fp.flat, self.fp.grad
        self._bucket, self._ema_stats = self.fp.bucket, self.fp.tail
        dev, n = self.flat.device, self.flat.numel()
        self.m = torch.zeros(n, device=dev)
        self.v = torch.zeros(n, device=dev)
        self.step_dev = torch.zeros(2, device=dev)        # completed-step counter, ping-ponged between the two words
        self._step_slot = 0
        # (VQ_VAE_z32 has no loss weights besides weight_matching: total = recon + commitment + matching, vae.py:456-470)
        self.w_recon = torch.tensor([float(getattr(model, "weight_recon", 1.0))], device=dev)
        self.w_commit = torch.tensor([float(getattr(model, "weight_commitment", 1.0))], device=dev)
        self.use_graph = use_graph
        # global_time_matching: the pairwise term over the whole global batch (each rank: its rows against every sample,
        # after one all-gather of the latents per step) instead of over the rank's own shard; nothing changes in one process
        self.global_tm = bool(global_time_matching) and self.world > 1
        if self.global_tm and self._extra:
            raise ValueError("FusedTrainer: global_time_matching is not available together with extra_loss")
        self._tm_gscale = torch.ones(1, device=dev)       # world / grad_weight: the rows' gradient through the exchange
        # sync_batchnorm: every training-mode BatchNorm normalises with the statistics of the global batch (one all-reduced
        # payload per layer and direction) instead of the rank's shard; nothing changes in one process
        self.sync_bn = bool(sync_batchnorm) and self.world > 1
        if self.sync_bn and self._extra:
            raise ValueError("FusedTrainer: sync_batchnorm is not available together with extra_loss")
        self._bn_w = torch.ones(2, dtype=torch.float64, device=dev)     # [forward weight, gradient weight] of those exchanges
        self._graphs = {}            # input shapes -> {inputs: static (x, mask, tm); train / eval: (_Segments, static output)}
        self._static_x = None        # input tensor of the program replayed last
        self._labels = None          # the extra losses' labels of the step being taken
        # same replica everywhere (the frozen codebook of the EMA mode is in neither the flat buffer nor the buffers)
        D.broadcast_(self.flat, list(model.buffers()) + ([model.vq.w.weight.data] if self._ema else []), group=self.group)

    # ------------------------------------------------------------------------------------------
    def G(self, p):
        return self.fp.gview(p)

    def expose_grads(self):
        """Make p.grad point at the flat gradient views (for inspection / torch tooling)."""
        self.fp.expose_grads()

    def latent_numel(self, sample_shape):
        """Elements of one sample's latent the time-matching term acts on, for samples of shape (C, H, W): z_before (VQ_VAE,
        VQ_VAE_z16: three stride-2 convolutions) or z_after (VQ_VAE_z32: two)."""
        f = self.model._layers_class.latent_stride
        return int(self.model.num_hiddens) * (int(sample_shape[-2]) // f) * (int(sample_shape[-1]) // f)

    # ------------------------------------------------------------------------------------------ the parts of a step
    def _forward(self, x, mask, for_backward=True):
        """The forward of either family: the same kernels as the autograd path (dynamorph_amd.vq_vae) called in order, no
        autograd bookkeeping.  VQ_VAE / VQ_VAE_z16: encoder (its last residual join in the quantiser's load path,
        dm_vq_forward_join), VectorQuantizer, decoder -- with for_backward its tail (dec.4, dec.6, loss) runs inside the
        decoder's backward, fused with it.  VQ_VAE_z32 (vae.py:430-470): two-conv stem + residual stack, VectorQuantizer,
        residual stack + BatchNorm tail.  Returns the state the other parts read: the finalize arguments (vqs, cx.loss_slabs,
        n, w) and lat, the (B, n) latents the pairwise term acts on (z_before, vq_vae.py:324-332; z_after for VQ_VAE_z32,
        vae.py:441-455, whose gradient reaches z through the straight-through value)."""
        m = self.model
        B, NIN, H, W = x.shape
        st = types.SimpleNamespace(cc=float(m.commitment_cost), n=B * NIN * H * W)
        st.L = L = E.layers_of(m)
        st.cb, st.w = L.codebook.weight, L.loss_weights
        if self._z32:           # the latent sits behind the quantiser
            st.z, st.ecx = E.z32_encoder_forward(L, x)
            lat, st.idx, st.vqs = E.vq_forward(st.cb, st.z, st.cc, defer_scalars=True)
            _, st.cx = E.z32_decoder_forward(L, lat, x, mask)
        else:                   # ... before it; the default-only routes: the last residual join in the quantiser, the deferred tail
            z, st.ecx = E.encoder_forward(L, x, defer_last_join=st.cb.shape[0] if JOIN_IN_VQ else 0)
            if z is None:       # the last residual join runs in the quantiser's load path (dm_vq_forward_join), which writes z
                z, zq, st.idx, st.vqs = E.vq_forward_joined(st.cb, st.ecx.pending_join, st.cc)
            else:
                zq, st.idx, st.vqs = E.vq_forward(st.cb, z, st.cc, defer_scalars=True)
            _, st.cx = E.decoder_forward(L, zq, x, mask, defer_tail=for_backward)
            st.z = lat = z
        st.lat = lat.reshape(B, -1)
        return st

    def _backward_to_latent(self, st):
        """The gradient at st.lat (shaped like the latent): the decoder's backward and, for VQ_VAE / VQ_VAE_z16, the
        quantiser's straight-through backward.  The slabs of every weight / bias / codebook gradient collect in st.pending."""
        st.pending = []
        if self._z32:           # the latent sits behind the quantiser: its backward runs in _backward_from_latent
            return E.z32_decoder_backward(st.L, st.cx, self.w_recon, None, self.G, pending=st.pending, zero_fed_biases=False)
        g_zq = E.decoder_backward(st.L, st.cx, self.w_recon, None, self.G, pending=st.pending)
        # codebook gradient as slabs, added in the encoder's single slab reduction: nothing to zero, no global atomics
        # (K <= 64: an ordered one-hot product on the matrix cores, bit-reproducible; larger K: LDS adds in arrival order)
        dz, cb_seg = self._vq_backward(st, g_zq)
        st.pending.insert(0, cb_seg)
        return dz

    def _vq_backward(self, st, g):
        """The quantiser's backward: (dz, the (slabs, destination) pair for the step's one slab reduction) -- the codebook
        gradient, or in the EMA mode the update's statistics (dm_vq_backward_stats: the same dz, another slab payload)."""
        if self._ema:
            dz, slabs = ops.vq_backward_stats(st.z, st.cb.detach(), st.idx, g, self.w_commit, st.cc)
            return dz, (slabs, self._ema_stats)
        dz, slabs = ops.vq_backward_slabs(st.z, st.cb.detach(), st.idx, g, self.w_commit, st.cc)
        return dz, (slabs, self.G(st.cb))

    def _backward_from_latent(self, st, g):
        """From the gradient at the latent: the rest of the backward (VQ_VAE_z32: the quantiser's straight-through backward,
        then the encoder) and ONE slab reduction for every weight / bias / codebook gradient of the step.  The flat gradient
        buffer starts at zero and nothing ever writes the BatchNorm-fed conv biases' slots (zero_fed_biases=False)."""
        backward = E.encoder_backward
        if self._z32:           # the latent sits behind the quantiser: its backward first, its segment behind the decoder's
            g, cb_seg = self._vq_backward(st, g)
            st.pending.append(cb_seg)
            backward = E.z32_encoder_backward
        backward(st.L, st.ecx, g, self.G, zero_fed_biases=False, pending_extra=st.pending)

    def _pairwise(self, st, tm, g=None, zg=None):
        """The pass's scalars (recon, commitment, total, perplexity[, time matching]) with the pairwise term on st.lat (tm: the
        relation block, None: no term); when training (g: the gradient at the latent) also g plus the term's gradient,
        summed in the kernel's store.  Returns (scalars, g, part):
          * local, latent lengths the MFMA kernels tile: the term's slabs finalized with the other scalars in one launch;
          * local, other lengths: distances from dm_pair_msd, the B x B weighting in torch (_time_matching);
          * global (zg: the gathered (Bg, n) latents of the whole batch): this rank's rows -- rows r0 .. r0 + B - 1 of zg --
            against every sample; the scalars leave the term out and part is the rows' share (float64, 1 element), which
            _with_global sums over the ranks."""
        m = self.model
        fin = (st.vqs.slabs, st.vqs.ws, st.vqs.K, st.vqs.D, st.vqs.positions, st.vqs.cc, st.cx.loss_slabs, st.n) + st.w
        ema = {"ema": True} if self._ema else {}          # (the EMA mode's commitment, cc * mse, from the same launch)
        if tm is None:
            return ops.vq_loss_finalize(*fin, **ema), g, None
        B, n = st.lat.shape
        wm, args = float(m.weight_matching), _tm_args(m, self._z32)
        tm = tm.to(torch.float32).contiguous()
        if zg is not None:
            r0, _ = D.shard_range(zg.shape[0], D.get_rank(self.group), self.world)
            part, S = ops.time_matching_forward_rows(zg, tm, r0, B, *args)
            if g is not None:
                # the bucket is multiplied by grad_weight = B * world / Bg before the exchange and by 1 / world in Adam's
                # load: the rows' gradient carries world / grad_weight (self._tm_gscale), so what arrives is the global term's
                g = ops.time_matching_backward_rows(zg, S, self._tm_gscale, wm, add=g).reshape(g.shape)
            return ops.vq_loss_finalize(*fin, **ema), g, part
        if ops.time_matching_supported(B, n):
            tm_slabs, S = ops.time_matching_forward(st.lat, tm, *args, want_slabs=True)
            if g is not None:
                g = ops.time_matching_backward(st.lat, S, None, wm, add=g).reshape(g.shape)
            return ops.vq_loss_finalize_tm(*fin, tm_slabs, wm, **ema), g, None
        tml, g_sim = self._time_matching(ops.pair_msd(st.lat), tm, args[0] == 1)
        if g is not None:
            g = g + ops.pair_msd_backward(st.lat, (g_sim * wm).contiguous()).reshape(g.shape)
        return _with_matching(ops.vq_loss_finalize(*fin, **ema), tml, wm), g, None

    def _time_matching(self, sim, tm, z16_form=None):
        """(loss, d loss / d sim) of the pairwise term on the (B, B) matrix of mean-squared latent distances:
        vq_vae.py:330-331 (sum of sim * matrix) or, for VQ_VAE_z16 / VQ_VAE_z32 (z16_form), vae.py:327-336 (weights,
        hinge, mean).  Only for latent lengths the MFMA kernels do not tile (n % 32 != 0)."""
        model = self.model
        if z16_form is None:
            z16_form = getattr(model, "_z16_loss", False)
        if not z16_form:
            return (sim * tm).sum(), tm
        wts = torch.where(tm == 2, torch.full_like(tm, model.w_a),
                          torch.where(tm == 1, torch.full_like(tm, model.w_t),
                                      torch.where(tm == 0, torch.full_like(tm, model.w_n), tm)))
        val = sim * wts
        hinge = tm == 0
        live = torch.where(hinge, (val + model.margin >= 0).to(sim.dtype), torch.ones_like(sim))
        val = torch.where(hinge, torch.clamp(val + model.margin, min=0), val)
        return val.mean(), wts * live / float(sim.numel())

    def _extra_losses(self, zq, out=None):
        """The caller's extra losses (vae.py:463-469) on z_after, as torch code in the middle of the step, with the step's
        labels (self._labels): returns d(sum of alpha * loss) / d z_after (written into out when given); the sum as a device
        scalar in self._extra_total, {name: loss} in self.last_extra_losses."""
        m = self.model
        leaf = zq.detach().requires_grad_(True)
        flat = leaf.reshape((leaf.shape[0], -1))
        total, named = None, {}
        with torch.enable_grad():
            for name, fn in m.extra_loss.items():
                loss, _frac_pos = fn(self._labels, flat)
                named[name] = loss.detach()
                total = loss * m.alpha if total is None else total + loss * m.alpha
            total.backward()
        self._extra_total, self.last_extra_losses = total.detach(), named
        g = (leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)).contiguous()
        return g if out is None else out.copy_(g)

    def _bn_context(self, cut):
        """With sync_batchnorm: every BatchNorm exchange of the launches enqueued inside is an all-reduce behind cut."""
        return E.bn_sync(E.BnSync(self._bn_w, lambda payload: cut(lambda _: D.allreduce_payload_(payload, self.group)))
                         if self.sync_bn else None)

    def _train_body(self, x, mask, tm, cut):
        """One forward + backward on this trainer's route.  Host work in the middle of the step sits behind cut(action,
        shape) -- the gather of the latents for the global term, the caller's extra losses, each BatchNorm exchange with
        sync_batchnorm -- so the same body is the eager step (_inline), the warm-up (_skip) and the capture (_Segments.cut).
        Returns (scalars, the rows' share of the global term or None)."""
        with self._bn_context(cut):
            st = self._forward(x, mask)
            g = self._backward_to_latent(st)
            zg = None
            if self.global_tm and tm is not None:
                Bg = tm.shape[0]
                zg = cut(lambda out: D.all_gather_rows(st.lat, Bg, self.group, out=out), (Bg, st.lat.shape[1]))
            scalars, g, part = self._pairwise(st, tm, g, zg)
            if self._extra:
                shape = g.shape
                g = g + cut(lambda out: self._extra_losses(st.lat.view(shape), out), shape)
            self._backward_from_latent(st, g)
        return scalars, part

    def forward_backward(self, x, mask=None, time_matching_mat=None):
        """One forward + backward of the rank's own shard (no collective, no extra losses); returns the device tensor
        (recon, commitment, total, perplexity[, time matching])."""
        st = self._forward(x, mask)
        scalars, g, _ = self._pairwise(st, time_matching_mat, self._backward_to_latent(st))
        self._backward_from_latent(st, g)
        return scalars

    def forward_only(self, x, mask=None, time_matching_mat=None):
        """The validation pass (run_training.py:522-531: forward with the module left in train mode, so BatchNorm uses
        batch statistics and advances its running statistics; no backward, no step).  Same kernels as forward_backward;
        returns the same device tensor (recon, commitment, total, perplexity[, time matching])."""
        tm = time_matching_mat
        st = self._forward(x, mask, for_backward=False)
        zg = D.all_gather_rows(st.lat, tm.shape[0], self.group) if self.global_tm and tm is not None else None
        scalars, _, part = self._pairwise(st, tm, zg=zg)
        return self._with_global(scalars, part)

    # ------------------------------------------------------------------------------------------ collectives
    def _global_total(self, part):
        """Sum over ranks of the rows' shares: the global-batch value of the term on every rank (ONE 8-byte all-reduce)."""
        tot = part.clone()
        torch.distributed.all_reduce(tot, op=torch.distributed.ReduceOp.SUM, group=self.group)
        return tot

    def _with_global(self, scalars, part):
        if part is None:
            return scalars
        return _with_matching(scalars, self._global_total(part).float(), float(self.model.weight_matching))

    def _join_without_data(self, global_rows):
        """A rank with an empty shard in a global_time_matching step: it still takes part in the gather of the latents and
        the all-reduce of the term (global_rows = (Bg, latent elements per sample)), so the collectives stay in step."""
        Bg, n = global_rows
        D.all_gather_rows(torch.empty((0, n), device=self.flat.device), Bg, self.group)
        self._global_total(torch.zeros(1, dtype=torch.float64, device=self.flat.device))

    def _bn_without_data(self, sample_shape, global_rows, training):
        """A rank whose shard is empty in a sync_batchnorm step (training) or validation pass: it runs the pass on one zero
        placeholder sample with forward and gradient weight 0 -- its payloads are zeros, its BatchNorm buffers still take
        the global statistics -- so it joins every exchange in the others' order.  global_rows: see step_without_data (it
        presents 0 rows to the gather).  The caller drops the placeholder's gradient."""
        if sample_shape is None:
            raise ValueError("FusedTrainer: with sync_batchnorm a rank without data needs sample_shape to join the exchanges")
        x = torch.zeros((1,) + tuple(sample_shape), device=self.flat.device)
        self._bn_w.zero_()
        with self._bn_context(_inline):
            if not training:
                self.forward_only(x)
            else:
                st = self._forward(x, None)
                g = self._backward_to_latent(st)
                if global_rows is not None:
                    D.all_gather_rows(torch.empty((0, global_rows[1]), device=x.device), global_rows[0], self.group)
                self._pairwise(st, None)
                self._backward_from_latent(st, g)
        if global_rows is not None:
            if training:
                self._global_total(torch.zeros(1, dtype=torch.float64, device=x.device))
            else:
                self._join_without_data(global_rows)

    def _allreduce(self, weight=1.0):
        """SUM over ranks of the flat gradient bucket: ONE collective and nothing behind it -- the "x 1 / world" of the mean
        is applied by the optimizer's load (_adam, dm_adam_counted_scaled), so after the exchange the bucket holds the sum.
        Every loss is a mean over the LOCAL batch, so with equal shards the mean of the per-rank gradients is the gradient
        of the global-batch mean loss; a rank whose shard of a ragged batch is smaller passes weight = n_local * world /
        n_global (0 for an empty shard)."""
        if self.world == 1:
            return
        if weight != 1.0:
            self.grad.mul_(float(weight))                 # (the gradients only: the EMA statistics behind them are plain sums)
        torch.distributed.all_reduce(self._bucket, op=torch.distributed.ReduceOp.SUM, group=self.group)

    def _adam(self):
        a, b = self._step_slot, 1 - self._step_slot
        ops.adam_counted(self.flat, self.grad, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps,
                         self.step_dev[a:a + 1], self.step_dev[b:b + 1], grad_scale=1.0 / self.world)
        self._step_slot = b
        if self._ema:            # the codebook's own update, from the global batch's statistics (after the exchange)
            self.model.vq.ema_apply(self._ema_stats)

    # ------------------------------------------------------------------------------------------ public steps
    def _fwd_bwd(self, x, mask, tm, grad_weight=1.0, labels=None, replay=True):
        """One forward + backward on this trainer's route: eagerly, or as the captured program of the input shape (with
        replay=False: only captured).  Returns the step's scalars -- with the global term summed over the ranks, with
        alpha * extra losses in total_loss (vae.py:467)."""
        if self.global_tm and tm is not None:
            Bg = tm.shape[0]
            lo, hi = D.shard_range(Bg, D.get_rank(self.group), self.world)
            if hi - lo != x.shape[0]:
                raise ValueError(f"FusedTrainer: global_time_matching needs the ({Bg}, {Bg}) relation block of the global "
                                 f"batch whose shard this rank's {x.shape[0]} samples are")
            self._tm_gscale.fill_(self.world / float(grad_weight))
        if self.sync_bn:
            self._bn_w[0].fill_(1.0)
            self._bn_w[1].fill_(float(grad_weight))
        self._labels = labels
        if not self.use_graph:
            scalars, part = self._train_body(x, mask, tm, _inline)
        else:
            segs, (scalars, part) = self._program("train", x, mask, tm)
            if not replay:
                return None
            segs.replay()
        scalars = self._with_global(scalars, part)
        if self._extra:
            scalars = scalars.clone()
            scalars[2] += self._extra_total
        return scalars

    def _step_with_extra_losses(self, x, mask, tm, labels):
        """The forward + backward of a VQ_VAE_z32 with extra_loss, without the exchange and Adam: the scalars with
        total_loss including the extra terms; self.last_extra_losses = {name: device scalar}."""
        return self._fwd_bwd(x, mask, tm, labels=labels)

    def step_without_data(self, global_rows=None, sample_shape=None):
        """This rank's shard of a ragged global batch is empty: it contributes a zero gradient to the exchange and takes
        the same Adam step as the others.  global_rows = (Bg, latent elements per sample) when the other ranks take a
        global_time_matching step (with a relation block): this rank joins its collectives too.  sample_shape = (C, H, W)
        of the others' samples: with sync_batchnorm this rank joins every BatchNorm exchange (_bn_without_data)."""
        with torch.cuda.device(self.flat.device):
            if self.sync_bn:
                self._bn_without_data(sample_shape, global_rows, training=True)
            elif self.global_tm and global_rows is not None:
                self._join_without_data(global_rows)
            self._bucket.zero_()         # (with the EMA mode's statistics: this rank adds nothing and still applies the update)
            self._allreduce()
            self._adam()

    def step(self, x, mask=None, time_matching_mat=None, grad_weight=1.0, timers=None, labels=None):
        """One optimisation step on a device batch; returns the device tensor of LOSS_KEYS values (+ the time-matching
        loss as a fifth entry when a matrix is given).  grad_weight: see _allreduce.  labels: the extra losses' (extra_loss).
        timers: a list -> this step appends (events, host_times): four events on the launch stream and four
        time.perf_counter() readings around its three parts (forward+backward | gradient exchange | Adam); read them with
        FusedTrainer.timer_summary after a synchronize.  Measurement only: the default path records nothing."""
        if not x.is_cuda:
            raise RuntimeError("FusedTrainer.step: batch must be on the GPU")
        if x.device != self.flat.device:
            raise RuntimeError(f"FusedTrainer.step: batch on {x.device}, model on {self.flat.device}")
        x = x.contiguous()
        with torch.cuda.device(self.flat.device):       # graph capture / replay and the streams are the model's device's
            mark = _Marks() if timers is not None else None
            if mark: mark()
            out = self._fwd_bwd(x, mask, time_matching_mat, grad_weight, labels)
            if mark: mark()
            self._allreduce(grad_weight)
            if mark: mark()
            self._adam()
            if mark:
                mark()
                timers.append(mark)
        return out

    @staticmethod
    def timer_summary(timers):
        """Averages (microseconds) over the steps recorded with step(..., timers=list): device time between the stream
        events and host time between the enqueue points, for forward+backward (graph replay), the gradient exchange and
        the fused Adam launch."""
        torch.cuda.synchronize()
        n = max(len(timers), 1)
        out = {}
        for i, part in enumerate(("fwd_bwd", "allreduce", "adam")):
            out[part + "_us"] = round(sum(m.ev[i].elapsed_time(m.ev[i + 1]) for m in timers) * 1e3 / n, 2)
            out[part + "_host_us"] = round(sum(m.t[i + 1] - m.t[i] for m in timers) * 1e6 / n, 2)
        out["steps"] = len(timers)
        return out

    def evaluate_without_data(self, global_rows=None, sample_shape=None):
        """The validation counterpart of step_without_data: a rank with an empty shard joins the collectives of a
        global_time_matching / sync_batchnorm validation pass (nothing to do otherwise)."""
        if self.sync_bn:
            with torch.cuda.device(self.flat.device):
                self._bn_without_data(sample_shape, global_rows, training=False)
        elif self.global_tm and global_rows is not None:
            with torch.cuda.device(self.flat.device):
                self._join_without_data(global_rows)

    def evaluate(self, x, mask=None, time_matching_mat=None):
        """forward_only through a captured HIP graph (one per input shape); returns the device tensor of loss values.  With
        sync_batchnorm or the global term the pass runs eagerly: its collectives sit inside the forward."""
        if not x.is_cuda or x.device != self.flat.device:
            raise RuntimeError(f"FusedTrainer.evaluate: batch on {x.device}, model on {self.flat.device}")
        x = x.contiguous()
        with torch.cuda.device(self.flat.device):
            if not self.use_graph or self.sync_bn or (self.global_tm and time_matching_mat is not None):
                if self.sync_bn:
                    self._bn_w[0].fill_(1.0)
                with self._bn_context(_inline):
                    return self.forward_only(x, mask, time_matching_mat)
            segs, out = self._program("eval", x, mask, time_matching_mat)
            segs.replay()
            return out

    def prepare(self, x, mask=None, time_matching_mat=None):
        """Capture the program step() replays for this input shape WITHOUT taking a step (the capture's warm-up run has its
        BatchNorm side effects put back, parameters and Adam state are untouched): a caller that times steps can keep the
        one-off capture out of its timed region.  Returns the program's input buffer (fill it in place to skip the copy)."""
        if not self.use_graph:
            return None
        with torch.cuda.device(self.flat.device):
            self._fwd_bwd(x.contiguous(), mask, time_matching_mat, replay=False)
        return self._static_x

    # ------------------------------------------------------------------------------------------ captured programs
    def static_inputs(self, x_shape, mask_shape=None, tm_shape=None):
        """(x, mask, matrix) buffers every program of this input shape reads: a loader that fills them in place and passes
        them to step() / evaluate() skips every copy (dynamorph_amd.feed writes its gathered batches here).  Allocated on
        first use, shared by the training and the validation program of the shape; nothing is captured here."""
        return self._entry(x_shape, mask_shape, tm_shape)["inputs"]

    def _entry(self, x_shape, mask_shape, tm_shape):
        key = tuple(None if s is None else tuple(s) for s in (x_shape, mask_shape, tm_shape))
        ent = self._graphs.get(key)
        if ent is None:
            dev = self.flat.device
            ent = self._graphs[key] = {"inputs": tuple(None if s is None else torch.zeros(s, device=dev) for s in key),
                                       "train": None, "eval": None}
        return ent

    def _program(self, kind, x, mask, tm):
        """The captured program ("train": _train_body, "eval": forward_only) of this input shape, captured on first use
        (a ragged last batch gets its own, captured once, not once per epoch), its static inputs holding x, mask, tm:
        (_Segments, static output)."""
        ent = self._entry(x.shape, None if mask is None else mask.shape, None if tm is None else tm.shape)
        _fill_static(ent["inputs"], (x, mask, tm))
        sx, smask, stm = ent["inputs"]
        self._static_x = sx
        if ent[kind] is None:
            body = ((lambda cut: self._train_body(sx, smask, stm, cut)) if kind == "train" else
                    (lambda cut: self.forward_only(sx, smask, stm)))
            # warm-up (allocator, lazy init) with every cut's host work left out: ranks may capture at different steps (a
            # ragged shard's shape), so nothing here may wait for another rank
            _warm_up(lambda: body(_skip), self.model.buffers())
            segs = _Segments()
            with segs.capture():
                out = body(segs.cut)
            ent[kind] = (segs, out)
        return ent[kind]

    def input_buffer(self):
        """Input tensor of the program replayed last (None before the first step): fill it in place to skip the copy."""
        return self._static_x


def _inline(action, shape=None):
    """cut() of an eager step: the host work runs in place (action(None) allocates what it returns)."""
    return action(None)


def _skip(action, shape=None):
    """cut() of a warm-up: the host work is left out; zeros stand in for what it would return."""
    return None if shape is None else torch.zeros(shape, device="cuda")


class _Segments:
    """A step captured as HIP graphs cut where host work must run (a collective, the caller's torch code): replay() is
    seg0 | after0 | seg1 | ... | segK, the host work between two replays on the launch stream (none is captured).  All
    segments allocate from the first one's memory pool, so a tensor one segment writes and a later one reads keeps its
    address.  A step without cuts is ONE graph."""

    def __init__(self):
        self.graphs, self.after = [], []

    @contextlib.contextmanager
    def capture(self):
        torch.cuda.synchronize()                 # (no collective of this process in flight while a stream captures)
        with torch.cuda.stream(torch.cuda.Stream()):
            self._begin()
            try:
                yield self
            finally:
                self.graphs[-1].capture_end()            # (also on an error: the stream must not stay in capture mode)

    def _begin(self):
        g = torch.cuda.CUDAGraph()
        if self.graphs:
            g.capture_begin(pool=self.graphs[0].pool())
        else:
            g.capture_begin()
        self.graphs.append(g)

    def cut(self, action, shape=None):
        """End the current segment; action(out) runs after its replay, before the next segment's.  shape: out is a buffer
        of that shape (returned here) which the action fills and later segments read."""
        out = None if shape is None else torch.empty(shape, device="cuda")
        self.graphs[-1].capture_end()
        self.after.append(lambda: action(out))
        self._begin()
        return out

    def replay(self):
        for i, g in enumerate(self.graphs):
            g.replay()
            if i < len(self.after):
                self.after[i]()


def _warm_up(run, tensors):
    """run() once on a side stream before a capture (allocator, lazy initialisation).  It really executes, so the tensors
    it advances (BatchNorm running statistics, ...) are put back afterwards: only replays count as steps."""
    tensors = list(tensors)
    saved = [t.detach().clone() for t in tensors]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for t, sv in zip(tensors, saved):
            t.copy_(sv)


def _tm_args(model, z32=False):
    """(mode, w_a, w_t, w_n, margin) of dm_time_matching_forward for this model family (vq_vae.py:330-331 / vae.py:327-336)."""
    z16 = z32 or getattr(model, "_z16_loss", False)
    return (1 if z16 else 0, float(getattr(model, "w_a", 0.0)), float(getattr(model, "w_t", 0.0)),
            float(getattr(model, "w_n", 0.0)), float(getattr(model, "margin", 0.0)))


def _with_matching(scalars, tml, wm):
    """(recon, commitment, total, perplexity) + the pairwise term -> the five values of a step with a relation matrix."""
    tml = tml.reshape(1)
    return torch.cat([scalars[:2], scalars[2:3] + wm * tml, scalars[3:4], tml])


def _fill_static(static, inputs):
    """Copy the caller's (x, mask, matrix) into a captured program's static inputs (a loader may have written them there)."""
    for dst, src in zip(static, inputs):
        if src is not None and src.data_ptr() != dst.data_ptr():
            dst.copy_(src)


class GraphedTrainer:
    """Any of the modules (VQ_VAE_z32 in particular, which FusedTrainer does not cover): the reference's step --
    model(x) / total_loss.backward() / Adam.step() (run_training.py:404-408, 485) -- recorded once per input shape into a HIP
    graph through autograd and replayed.  Same arithmetic as the eager loop with torch.optim.Adam (capturable form: the
    step count lives on the device); what goes away is the per-launch host work.  Measured on VQ_VAE_z32 the GPU is already
    the limit of the eager loop (no gain at B = 256..2048), so train() uses it only on request (fused="graph"): it is for
    small batches and busy hosts.  Single process (no gradient exchange)."""

    def __init__(self, model, lr=1e-3, betas=(.9, .999), eps=1e-8):
        if _ema_mode(model):
            raise ValueError("GraphedTrainer: the EMA codebook update is not built into the captured autograd step (its "
                             "in-place update of the frozen codebook sits between forward and backward); train an EMA model "
                             "with FusedTrainer (fused=True) or the eager autograd route (fused=False)")
        params = [p for p in model.parameters() if p.requires_grad]
        if not params or params[0].device.type != "cuda":
            raise RuntimeError("GraphedTrainer: move the model to the GPU first (no CPU fallback)")
        self.model = model
        self.opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps, capturable=True, foreach=True)
        self._graphs = {}            # input shapes -> (graph, static x, static mask, static matrix, static output)

    def _eager(self, x, mask, tm):
        self.opt.zero_grad(set_to_none=True)      # backward then assigns fresh gradients (from the graph's pool on replay)
        _, ld = self.model(x, time_matching_mat=tm, batch_mask=mask)
        ld["total_loss"].backward()
        self.opt.step()
        vals = [ld[k].detach().reshape(()) for k in LOSS_KEYS]
        if tm is not None:
            vals.append(ld["time_matching_loss"].detach().reshape(()))
        return torch.stack(vals)

    def _capture(self, x, mask, tm):
        sx = x.clone()
        smask = mask.clone() if mask is not None else None
        stm = tm.clone().float() if tm is not None else None
        # the warm-up (also the lazy state of the optimizer) puts parameters and buffers back; the optimizer state it
        # touched is put back here
        had_state = len(self.opt.state) > 0
        opt_saved = [{k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in self.opt.state[p].items()}
                     for g in self.opt.param_groups for p in g["params"]] if had_state else None
        _warm_up(lambda: [self._eager(sx, smask, stm) for _ in range(2)],
                 list(self.model.parameters()) + list(self.model.buffers()))
        with torch.no_grad():
            i = 0
            for g in self.opt.param_groups:
                for p in g["params"]:
                    for k, v in self.opt.state[p].items():
                        if torch.is_tensor(v):
                            v.copy_(opt_saved[i][k]) if had_state else v.zero_()
                    i += 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = self._eager(sx, smask, stm)
        return g, sx, smask, stm, out

    def step(self, x, mask=None, time_matching_mat=None):
        """One optimisation step; returns the device tensor of LOSS_KEYS values (+ the time-matching loss when given)."""
        if not x.is_cuda:
            raise RuntimeError("GraphedTrainer.step: batch must be on the GPU")
        tm = time_matching_mat
        key = (tuple(x.shape), None if mask is None else tuple(mask.shape), None if tm is None else tuple(tm.shape))
        with torch.cuda.device(x.device):
            if key not in self._graphs:
                self._graphs[key] = self._capture(x.contiguous(), mask, tm)       # (a ragged last batch gets its own graph)
            else:
                _fill_static(self._graphs[key][1:4], (x, mask, tm))
            g, _, _, _, out = self._graphs[key]
            g.replay()
        return out


# ================================================================ reference-style loop mirrors
def _augment(batch):
    """run_training.py:396-403: a random flip (none / up-down / left-right) and a random multiple of 90 degrees per
    sample, drawn from numpy's global generator in the reference's order (flip, rotation, flip, rotation, ...: a caller's
    np.random.seed reproduces the reference's augmentation, ops.augment_codes) -- applied by ONE kernel instead of the
    O(B) loop."""
    flips, rots = ops.augment_codes(len(batch))
    flips = torch.from_numpy(flips).to(batch.device)
    rots = torch.from_numpy(rots).to(batch.device)
    return ops.augment(batch.contiguous(), flips, rots)


def run_one_batch(model, batch, train_loss, model_kwargs=None, optimizer=None, transform=None, training=True,
                  grad_weight=1.0):
    """run_training.py:377-417.  `optimizer` may be a torch optimizer (autograd path), a FusedTrainer or a GraphedTrainer.
    grad_weight scales this rank's gradient before the data-parallel mean (FusedTrainer._allreduce); 1 in one process."""
    model_kwargs = model_kwargs or {}
    if transform is not None:
        batch = _augment(batch)
    if isinstance(optimizer, (FusedTrainer, GraphedTrainer)) and training:
        # (train_with_loader hands the labels of the extra losses through model_kwargs, run_training.py:596-599)
        kw = {"grad_weight": grad_weight, "labels": model_kwargs.get("labels")} if isinstance(optimizer, FusedTrainer) else {}
        vals = optimizer.step(batch, model_kwargs.get("batch_mask"), model_kwargs.get("time_matching_mat"), **kw)
        vals = vals.tolist()                                           # one device sync per step (reference: five)
        loss_dict = dict(zip(LOSS_KEYS, vals))
        loss_dict["time_matching_loss"] = vals[4] if len(vals) > 4 else 0.
        loss_dict = _in_model_order(model, loss_dict)
        if getattr(optimizer, "_extra", False):                        # vae.py:469: one entry per extra loss, after total_loss
            loss_dict.update({k: float(v) for k, v in optimizer.last_extra_losses.items()})
    else:
        _, loss_dict = model(batch, **model_kwargs)
        if training:
            loss_dict['total_loss'].backward()
            params = [p for p in model.parameters() if p.requires_grad]
            if grad_weight != 1.0:
                for p in params:
                    if p.grad is not None:
                        p.grad.mul_(float(grad_weight))
            D.allreduce_grads_(params)                          # data parallel: one flat bucket (no-op in one process)
            optimizer.step()
            model.zero_grad()
    for key, loss in loss_dict.items():
        train_loss.setdefault(key, []).append(float(loss))
    return model, train_loss


def _step_without_data(model, optimizer, global_rows=None, sample_shape=None):
    """A rank whose shard of a ragged global batch is empty still joins the gradient exchange (with zeros) and the step
    (global_rows, sample_shape: see FusedTrainer.step_without_data)."""
    if isinstance(optimizer, FusedTrainer):
        optimizer.step_without_data(global_rows, sample_shape)
        return
    params = [p for p in model.parameters() if p.requires_grad]
    for p in params:
        p.grad = torch.zeros_like(p)
    D.allreduce_grads_(params)
    optimizer.step()
    model.zero_grad()


def get_relation_tensor(relation_mat, sample_ids, device='cuda:0'):
    """run_training.py:335-355: the (B, B) block of the symmetric sample-relation matrix (scipy sparse or dense) for
    this batch as a float32 tensor -- the `time_matching_mat` argument of VQ_VAE.forward."""
    if relation_mat is None:
        return None
    block = relation_mat[sample_ids, :][:, sample_ids]
    if hasattr(block, "todense"):
        block = block.todense()
    out = torch.from_numpy(np.ascontiguousarray(np.asarray(block), dtype=np.float32))
    return out.to(device) if device else out


def get_mask(mask, sample_ids, device='cuda:0'):
    """run_training.py:358-374: cell masks of this batch.  `mask` is a TensorDataset-like object whose first tensor is
    (N, 2, H, W) in {-1, 1}; the second channel (the large mask) is kept and mapped to {0, 1} -> (B, 1, H, W), the
    `batch_mask` argument of VQ_VAE.forward."""
    if mask is None:
        return None
    m = mask[sample_ids][0][:, 1:2, :, :]
    m = (m + 1.) / 2.
    return m.to(device)


class _EpochLosses:
    """Epoch value of every entry of the loss dict.

    One process: the reference's aggregation, run_training.py:538-543 -- sum(per-batch values) / number of batches.
    Data parallel (world > 1): every rank sees only its shard of a batch, so the per-key sums of (local loss x local
    samples) and the sample count are exchanged ONCE per phase and every rank holds the same sample-weighted means (and
    takes the same early-stopping decision).  With a ragged last batch that differs slightly from the mean of batch
    values, and for the pairwise time-matching term (a sum over the LOCAL pairs, vq_vae.py:331) it is a different
    quantity altogether: documented deviation, there is no multi-device behaviour in the reference to match.
    The exchanged vector has the same length on every rank: the key list is rank 0's (rank 0 holds the first shard of
    every batch, dist.shard_range, so it has data whenever any rank has); a rank that had no data in the whole phase
    contributes zeros."""

    def __init__(self, device, world=1):
        self.values, self.sums, self.count, self.device, self.world = {}, {}, 0.0, device, world

    def add(self, batch_losses, n):
        for key, values in batch_losses.items():
            v = float(values[-1])
            self.values.setdefault(key, []).append(v)
            self.sums[key] = self.sums.get(key, 0.0) + v * n
        self.count += n

    def means(self):
        if self.world == 1:
            return {k: sum(v) / len(v) for k, v in self.values.items()}
        keys = D.broadcast_object(list(self.sums))
        tot = D.allreduce_sum_host([self.sums.get(k, 0.0) for k in keys] + [self.count], device=self.device)
        return {k: v / max(tot[-1], 1.0) for k, v in zip(keys, tot[:-1])}


def _ema_mode(model):
    """The model's quantiser learns its codebook by the EMA update (VectorQuantizer(ema_decay=...))."""
    return bool(getattr(getattr(model, "vq", None), "ema", False))


def _make_optimizer(model, lr, fused, global_time_matching=False, sync_batchnorm=False):
    from .vq_vae import VQ_VAE
    from .vq_vae import VQ_VAE_z32
    # (a model with caller-supplied extra losses, vae.py:463-469, runs arbitrary torch code per step: the autograd path)
    fusable = isinstance(model, (VQ_VAE, VQ_VAE_z32)) and getattr(model, "extra_loss", None) is None
    if _ema_mode(model) and fused == "graph":
        raise ValueError("fused='graph' (GraphedTrainer) does not take a model with the EMA codebook update; use fused=True "
                         "(FusedTrainer) or, in one process, fused=False")
    if _ema_mode(model) and D.world_size() > 1 and not (fused and fusable):
        raise ValueError("the EMA codebook update with more than one rank needs the fused step (FusedTrainer: fused=True and a "
                         "VQ_VAE / VQ_VAE_z16 / VQ_VAE_z32 without extra_loss): the autograd route forms the update's "
                         "statistics on each rank's shard only")
    if global_time_matching and not (fused and fused != "graph" and fusable):
        raise ValueError("global_time_matching=True needs the fused step (FusedTrainer: fused=True and a VQ_VAE / VQ_VAE_z16 / "
                         "VQ_VAE_z32 without extra_loss); the autograd route forms the time-matching term on each rank's "
                         "shard only")
    if sync_batchnorm and not (fused and fused != "graph" and fusable):
        raise ValueError("sync_batchnorm=True needs the fused step (FusedTrainer: fused=True and a VQ_VAE / VQ_VAE_z16 / "
                         "VQ_VAE_z32 without extra_loss); the autograd route normalises with each rank's shard only")
    if D.world_size() > 1 and not (fused and fused != "graph" and fusable):
        # FusedTrainer broadcasts its flat buffer itself; any other module: same replica everywhere before the first step
        for t in list(model.parameters()) + list(model.buffers()):
            torch.distributed.broadcast(t.data, src=0)
    if fused == "graph" and D.world_size() == 1:
        return GraphedTrainer(model, lr=lr)               # any module: the autograd step as a replayed HIP graph
    if fused and fusable:
        return FusedTrainer(model, lr=lr, global_time_matching=global_time_matching, sync_batchnorm=sync_batchnorm)
    return torch.optim.Adam(model.parameters(), lr=lr, betas=(.9, .999))


class _LossLog:
    """Per-batch loss values of one phase, kept on the device: a step's values are copied into a row (stream-ordered,
    the captured step overwrites its output tensor on the next replay) and the whole phase is read back ONCE, instead of
    the reference's float(loss) per key and step (run_training.py:409-414), which stalls the host on every step."""

    def __init__(self, device, n_batches, width=8, model=None):
        self.buf = torch.zeros((max(n_batches, 1), width), device=device)
        self.meta = []                      # (keys, number of values, samples) per logged batch
        self.model = model

    def add(self, keys, vals, n):
        k = vals.numel()
        self.buf[len(self.meta), :k].copy_(vals.detach().reshape(-1), non_blocking=True)
        self.meta.append((keys, k, n))

    def rows(self):
        """[(dict key -> float, samples)] in batch order; the one device synchronisation of the phase."""
        host = self.buf[:max(len(self.meta), 1)].tolist()
        out = []
        for (keys, k, n), row in zip(self.meta, host):
            d = dict(zip(keys, row[:k]))
            d.setdefault("time_matching_loss", 0.)
            out.append((_in_model_order(self.model, d) if self.model is not None else d, n))
        return out


_FUSED_KEYS = LOSS_KEYS + ("time_matching_loss",)


def loss_key_order(model):
    """Key order of the loss dict the model's forward returns -- what run_one_batch's `for key, loss in
    train_loss_dict.items()` (run_training.py:409) and with it the order of the epoch's writer.add_scalar rows follow:
    vq_vae.py:333-338 (VQ_VAE: ..., total_loss, perplexity) and vae.py:337-342, 456-470 (VQ_VAE_z16 / VQ_VAE_z32: ...,
    perplexity, total_loss).  The fused steps return a flat vector of values; their rows are put back in this order."""
    z16 = getattr(model, "_z16_loss", False) or type(model).__name__ == "VQ_VAE_z32"
    tail = ("perplexity", "total_loss") if z16 else ("total_loss", "perplexity")
    return ("recon_loss", "commitment_loss", "time_matching_loss") + tail


def _in_model_order(model, d):
    order = loss_key_order(model)
    out = {k: d[k] for k in order if k in d}
    out.update((k, v) for k, v in d.items() if k not in out)        # (extra_loss entries keep their place at the end)
    return out


def _device_step(model, optimizer, x, kw, training, grad_weight):
    """One batch that is already on the device -> (loss keys, device tensor of their values); nothing here waits for the
    GPU.  Same arithmetic as run_one_batch for every kind of optimizer."""
    mask, tm = kw.get("batch_mask"), kw.get("time_matching_mat")
    if isinstance(optimizer, FusedTrainer):
        vals = (optimizer.step(x, mask, tm, grad_weight=grad_weight) if training else optimizer.evaluate(x, mask, tm))
        return _FUSED_KEYS[:vals.numel()], vals
    if isinstance(optimizer, GraphedTrainer) and training:
        vals = optimizer.step(x, mask, tm)
        return _FUSED_KEYS[:vals.numel()], vals
    with torch.enable_grad() if training else torch.no_grad():
        _, loss_dict = model(x, **kw)
        if training:
            loss_dict['total_loss'].backward()
            params = [p for p in model.parameters() if p.requires_grad]
            if grad_weight != 1.0:
                for p in params:
                    if p.grad is not None:
                        p.grad.mul_(float(grad_weight))
            D.allreduce_grads_(params)
            optimizer.step()
            model.zero_grad()
    keys = tuple(k for k, v in loss_dict.items() if torch.is_tensor(v))      # (a float entry is the constant 0. of :382)
    return keys, torch.stack([loss_dict[k].detach().reshape(()).float() for k in keys])


def train(model, dataset, output_dir, relation_mat=None, mask=None, n_epochs=10, lr=0.001, batch_size=16,
          device='cuda:0', shuffle_data=False, transform=None, val_split_ratio=0.15, patience=20,
          get_relation_tensor=None, get_mask=None, writer=None, fused=True, feed="auto", stats=None, probe=None,
          global_time_matching=False, sync_batchnorm=False):
    """The training loop of run_training.py:455-551 -- Adam, a contiguous validation block at a random start, epoch and
    batch loops, TensorBoard-style scalars, EarlyStopping checkpoint of the state_dict to <output_dir>/model.pt -- made
    data parallel (one process per GPU, torch.distributed initialised by the launcher):

      * one process: split, shuffles, augmentation codes and epoch losses exactly as the reference draws / aggregates them
        (numpy's global generator in the reference's order, mean of the per-batch values);
      * world > 1: the validation split and every shuffle come from ONE seed drawn on rank 0, so all ranks walk the same
        batches;
      * each global batch of `batch_size` samples is cut into contiguous per-rank shards (dist.shard_range); a rank
        weights its gradient by n_local * world / n_global before the single all-reduce, so the averaged gradient is the
        global-batch mean loss's (by default BatchNorm statistics and the pairwise time-matching term stay rank-local;
        the reference has no multi-device behaviour to match);
      * global_time_matching=True: the time-matching term is the global batch's -- every rank builds the relation block of
        the batch's GLOBAL ids, gathers the latents (one collective per step) and forms its rows against the whole batch,
        so the exchanged gradient is that of the one-process term and the epoch records print the one-process value
        (fused step only: any other route raises ValueError);
      * sync_batchnorm=True: every training-mode BatchNorm normalises with the statistics of the global batch and every
        rank's running statistics are the global batch's (nn.SyncBatchNorm's arithmetic, one small all-reduce per layer and
        direction); a rank with an empty shard joins those exchanges on a zero-weight placeholder sample.
        Validation runs through the trainer, eagerly.  Together with global_time_matching=True a W-rank step computes
        what one process computes on the whole batch (fused step only: any other route raises ValueError);
      * epoch losses are exchanged once per epoch, the early-stopping decision is therefore the same everywhere;
      * rank 0 alone writes model.pt (atomically), the others wait at a barrier.

    feed (dynamorph_amd.feed): where a batch comes from.  "auto": the dataset, its masks and the CSR relation matrix are
    uploaded once and stay in HBM when they fit ("resident": a batch is one gather + augment launch into the captured
    step's input buffer, losses are read back once per phase, the host never waits inside an epoch), else "stream"
    (pinned staging, copy stream, two device slots: PCIe-bound); "sync": the reference's loop as it is (host gather,
    synchronous copy, float() per step) -- taken automatically on the CPU, for dataset objects that only support
    dataset[ids], and when the caller brings its own get_relation_tensor / get_mask.  All feeds produce the same batches.
    stats: a dict that receives {"feed", "phase_seconds": {phase: [per epoch]} (device time between the phase's first and
    last launch; host wall time on the CPU), "phase_samples": {phase: n}, "epoch_seconds": [wall clock per epoch],
    "step_losses": {phase: [per epoch: [loss dict of every batch, in order]]}}.
    probe: callable(phase, epoch, ids, x, kwargs) called with every batch right before its step -- the sample ids of this
    rank's shard, the (augmented) batch and the model kwargs exactly as the step is about to read them (the tests hold
    them against what the reference's loop hands its model, tests/golden/g11_train_loop.npz); it must copy what it keeps.

    `dataset` is a TensorDataset-like object indexable with a list of ids (dataset[ids][0] -> host tensor)."""
    assert val_split_ratio is None or 0 < val_split_ratio < 1
    if patience is not None:
        assert val_split_ratio is not None
    custom_hooks = get_relation_tensor is not None or get_mask is not None
    if get_relation_tensor is None and relation_mat is not None:
        get_relation_tensor = globals()["get_relation_tensor"]
    if get_mask is None and mask is not None:
        get_mask = globals()["get_mask"]
    dev = torch.device(device)
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    rank, world = D.get_rank(), D.world_size()
    optimizer = _make_optimizer(model, lr, fused, global_time_matching, sync_batchnorm)
    model.zero_grad()
    # the global time-matching term: relation blocks of the global batch, and what an empty shard needs to join its collectives
    global_tm = isinstance(optimizer, FusedTrainer) and optimizer.global_tm and relation_mat is not None
    sync_bn = isinstance(optimizer, FusedTrainer) and optimizer.sync_bn

    if feed not in ("auto", "resident", "stream", "sync"):
        raise ValueError(f"train: unknown feed {feed!r}")
    feeder = None
    if feed != "sync":
        from . import feed as F
        src = F.dataset_tensor(dataset)
        usable = (dev.type == "cuda" and not custom_hooks and src is not None and src.dim() == 4 and src.shape[2] == src.shape[3]
                  and (mask is None or F.dataset_tensor(mask) is not None))
        if usable:
            feeder = F.Feed(dataset, dev, mode=feed, mask=mask, relation_mat=relation_mat, batch_size=batch_size,
                            trainer=optimizer if isinstance(optimizer, FusedTrainer) else None)
        elif feed != "auto":
            raise ValueError(f"train: feed={feed!r} needs a CUDA device, a tensor-backed dataset and the default "
                             "get_relation_tensor / get_mask")
    if stats is not None:
        stats.update(feed=feeder.mode if feeder else "sync", phase_seconds={"train": [], "val": []}, phase_samples={},
                     step_losses={"train": [], "val": []})

    # the reference's loop takes dataset[ids][0]; a bare tensor / ndarray (what upload_zscored returns) is indexed directly
    bare = None
    if torch.is_tensor(dataset) or isinstance(dataset, np.ndarray):
        bare = torch.as_tensor(dataset)
    n_samples = len(dataset)
    sample_shape = None
    if global_tm or sync_bn:
        from .feed import dataset_tensor
        src = bare if bare is not None else dataset_tensor(dataset)
        sample_shape = tuple(src.shape[1:]) if src is not None else tuple(dataset[[0]][0].shape[1:])
    # (an int array instead of the reference's list: the same draws shuffle it into the same order -- numpy's shuffle is
    # the same Fisher-Yates walk for both -- and slicing a phase into batches costs nothing)
    sample_ids = np.arange(n_samples, dtype=np.int64)
    split = int(np.floor(val_split_ratio * n_samples))
    if world == 1:
        # the reference's draws from numpy's global generator, in the reference's order (run_training.py:490-493, 536):
        # a caller's np.random.seed reproduces the reference's split and shuffles
        order = np.random
    else:
        seed = D.broadcast_object(int(np.random.randint(0, 2 ** 31 - 1)))
        order = np.random.RandomState(seed)                 # split and shuffles: the same stream on every rank
        np.random.seed((seed + 7919 * rank) % (2 ** 32))    # augmentation draws: a stream of its own per rank
    split_start = int(order.randint(0, n_samples - split))
    if shuffle_data:
        order.shuffle(sample_ids)
    phases = {"train": np.concatenate([sample_ids[:split_start], sample_ids[split_start + split:]]),
              "val": sample_ids[split_start: split_start + split].copy()}

    os.makedirs(output_dir, exist_ok=True)
    early_stopping = EarlyStopping(patience=patience, verbose=(rank == 0), path=os.path.join(output_dir, 'model.pt'))
    early_stopping.writes = rank == 0
    say = print if rank == 0 else (lambda *a, **k: None)
    import time
    timed = stats is not None and dev.type == "cuda"
    for epoch in range(n_epochs):
        say('start epoch %d' % epoch)
        t_epoch = time.perf_counter()
        epoch_means, logs, marks = {}, {}, {}
        for phase, ids in phases.items():
            t_phase = time.perf_counter()
            if timed:
                marks[phase] = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]
                marks[phase][0].record()
            training = phase == "train"
            losses = _EpochLosses(dev if dev.type == "cuda" else None, world)
            # this rank's shard of every global batch and the weight of its gradient in the data-parallel mean
            plan, batch_ids = [], []
            for start in range(0, len(ids), batch_size):
                ids_batch = ids[start:start + batch_size]
                lo, hi = D.shard_range(len(ids_batch), rank, world)
                plan.append((ids_batch[lo:hi], D.shard_weight(len(ids_batch), rank, world)))
                batch_ids.append(ids_batch)

            def no_data(k):
                rows = (len(batch_ids[k]), optimizer.latent_numel(sample_shape)) if global_tm else None
                if training:
                    _step_without_data(model, optimizer, rows, sample_shape)
                elif rows is not None or sync_bn:
                    optimizer.evaluate_without_data(rows, sample_shape)
            if feeder is not None:
                log = _LossLog(dev, len(plan), model=model)
                batches = feeder.phase([p[0] for p in plan], transform, fused=isinstance(optimizer, FusedTrainer),
                                       tm_batches=batch_ids if global_tm else None)
                for k, (ids_local, weight) in enumerate(plan):
                    if not len(ids_local):
                        no_data(k)
                        continue
                    n, x, kw = next(batches)
                    if probe is not None:
                        probe(phase, epoch, ids_local, x, kw)
                    keys, vals = _device_step(model, optimizer, x, kw, training, weight)
                    log.add(keys, vals, n)
                for _ in batches:                                   # (runs the generator to its end)
                    pass
                logs[phase] = (log, losses)                         # read back after BOTH phases are enqueued
            else:
                per_step = []
                for k, (ids_local, weight) in enumerate(plan):
                    if not len(ids_local):
                        no_data(k)
                        continue
                    ids_tm = batch_ids[k].tolist() if global_tm else ids_local.tolist()
                    ids_local = ids_local.tolist()                  # (the reference indexes with lists)
                    if bare is not None:
                        batch = bare[ids_local].to(dev)             # a bare tensor / ndarray: dataset[ids][0] would be ONE sample
                    else:
                        batch = dataset[ids_local][0].to(dev)
                    kw = {'time_matching_mat': get_relation_tensor(relation_mat, ids_tm, device=dev) if get_relation_tensor else None,
                          'batch_mask': get_mask(mask, ids_local, device=dev) if get_mask else None}
                    last = {}
                    if transform is not None:
                        batch = _augment(batch)                     # (run_one_batch's first statement, run_training.py:396)
                    if probe is not None:
                        probe(phase, epoch, ids_local, batch, kw)
                    if (global_tm or sync_bn) and not training:
                        # (the validation pass through the trainer: the global term's and the BatchNorm exchanges sit in its
                        # forward, and the ranks without data join them -- the module's own forward would leave them waiting)
                        keys, vals = _device_step(model, optimizer, batch, kw, False, weight)
                        row = dict(zip(keys, vals.tolist()))
                        row.setdefault("time_matching_loss", 0.)
                        last = {k: [v] for k, v in _in_model_order(model, row).items()}
                    else:
                        run_one_batch(model, batch, last, optimizer=optimizer, model_kwargs=kw, transform=None,
                                      training=training, grad_weight=weight)
                    losses.add(last, len(ids_local))
                    if stats is not None:
                        per_step.append({k: v[-1] for k, v in last.items()})
                epoch_means[phase] = losses.means()
                if stats is not None:
                    stats["step_losses"][phase].append(per_step)
            if stats is not None:
                if timed:
                    marks[phase][1].record()
                else:
                    stats["phase_seconds"][phase].append(time.perf_counter() - t_phase)
                stats["phase_samples"][phase] = sum(len(p[0]) for p in plan)
        # the epoch's one device synchronisation: the loss rows of both phases (the validation pass was enqueued behind the
        # training steps without waiting for them)
        for phase, (log, losses) in logs.items():
            rows = log.rows()
            for row, n in rows:
                losses.add({k: [v] for k, v in row.items()}, n)
            epoch_means[phase] = losses.means()
            if stats is not None:
                stats["step_losses"][phase].append([row for row, _ in rows])
        if timed:
            torch.cuda.synchronize(dev)
            for phase, (e0, e1) in marks.items():                   # device time between the phase's first and last launch
                stats["phase_seconds"][phase].append(e0.elapsed_time(e1) * 1e-3)
        if shuffle_data:
            order.shuffle(phases["train"])
        if writer is not None and rank == 0:
            for phase, prefix in (("train", 'Loss/'), ("val", 'Val loss/')):
                for key, value in epoch_means[phase].items():
                    writer.add_scalar(prefix + key, value, epoch)
        early_stopping(epoch_means["val"]['total_loss'], model)
        D.barrier()                                          # model.pt is complete before any rank moves on
        if stats is not None:
            stats.setdefault("epoch_seconds", []).append(time.perf_counter() - t_epoch)      # wall clock, checkpoint included
        if early_stopping.early_stop:
            say("Early stopping")
            break
        say('epoch %d' % epoch)
        for phase, label in (("train", 'train: '), ("val", 'validation: ')):
            say(label, ''.join(['{}:{:0.4f}  '.format(key, loss) for key, loss in epoch_means[phase].items()]))
    if feeder is not None:
        feeder.close()
    return model
