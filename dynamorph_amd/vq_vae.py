"""Drop-in nn.Module surface of the reference's VQ-VAE, computed by the HIP kernels.

Mirrors (constructor signatures, attribute / submodule names, state-dict keys, return values):
  VectorQuantizer  HiddenStateExtractor/vq_vae.py:25-116  (== vae.py:12-103)
  ResidualBlock    HiddenStateExtractor/vq_vae.py:180-225
  VQ_VAE           HiddenStateExtractor/vq_vae.py:228-342
  VQ_VAE_z16       HiddenStateExtractor/vae.py:216-346
so `getattr(vae, network)(**kw).to(device)`, `load_state_dict(torch.load(model.pt))`,
`model.enc(x)`, `model.vq(z)`, `model(batch, time_matching_mat=..., batch_mask=...)`,
`total_loss.backward()` and `optimizer.step()` (run_training.py:885-910, 404-408;
pipeline/patch_VAE.py:425-452) work unchanged.

The nn.Conv2d / BatchNorm2d / ConvTranspose2d / Embedding children are parameter containers only
(that is what keeps the 68 state-dict keys); their ATen forward is never called.  All compute goes
through dynamorph_amd.engine -> libdynamorph_hip.so.  Inputs must live on the GPU: there is no CPU
fallback (a CPU tensor raises).
"""
import numpy as np
import torch
import torch.nn as nn

from . import engine as E
from . import ops

CHANNEL_VAR = np.array([1., 1.])


def _require_gpu(t, who):
    if not t.is_cuda:
        raise RuntimeError(f"{who}: input is on {t.device}; the dynamorph_amd HIP path only runs on the GPU "
                           "(no CPU fallback). Move the model and the batch to cuda first.")


def _prep(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


class _GradBag:
    """G(param) -> the tensor a backward kernel writes that parameter's gradient into."""

    def __init__(self):
        self.store = {}

    def __call__(self, p):
        g = self.store.get(id(p))
        if g is None:
            g = torch.empty_like(p)
            self.store[id(p)] = g
        return g

    def grads_for(self, params, needs):
        return tuple(self.store.get(id(p)) if need else None for p, need in zip(params, needs))


# =============================================================================== autograd
def _conv_stage_fn(forward, backward):
    """The autograd Function of a conv stage with parameters, (x, layers, per_sample, *params) -> z, on an engine pair
    forward(layers, x, per_sample=) -> (z, cx) and backward(layers, cx, g_z, G, want_dx=) -> dx."""
    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, layers, per_sample, *params):
            z, cx = forward(layers, x, per_sample=per_sample)
            ctx.layers, ctx.cx, ctx.params = layers, cx, params
            return z

        @staticmethod
        def backward(ctx, g_z):
            G = _GradBag()
            dx = backward(ctx.layers, ctx.cx, g_z, G, want_dx=ctx.needs_input_grad[0])
            ctx.cx = None
            return (dx, None, None) + G.grads_for(ctx.params, ctx.needs_input_grad[3:])
    return Fn


_EncoderFn = _conv_stage_fn(E.encoder_forward, E.encoder_backward)
_Z32StemFn = _conv_stage_fn(E.z32_stem_forward, E.z32_stem_backward)     # enc[0:5] of VQ_VAE_z32: Conv(4,2,1) BN ReLU Conv BN


class _ResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, res_layers, *params):
        out, saved = E.residual_forward(res_layers, h)
        ctx.res_layers, ctx.saved, ctx.params = res_layers, saved, params
        return out

    @staticmethod
    def backward(ctx, g):
        G = _GradBag()
        pending = []
        g_in, _ = E.residual_backward(ctx.res_layers, ctx.saved, g.contiguous(), G, None, pending=pending)
        ops.reduce_slabs_multi(pending)
        ctx.saved = None
        return (g_in, None) + G.grads_for(ctx.params, ctx.needs_input_grad[2:])


class _VQFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, codebook, commitment_cost, ema=False):
        """ema (the EMA codebook mode): loss = cc * mse; the codebook is frozen and updated in place right after this
        forward (VectorQuantizer._quantize), so the backward keeps its own copy of the K x D values it quantised with."""
        out, idx, scalars = E.vq_forward(codebook, z, commitment_cost, ema=ema)
        ctx.save_for_backward(z, codebook.detach().clone() if ema else codebook, idx)
        ctx.cc = commitment_cost
        ctx.mark_non_differentiable(idx)
        ctx.set_materialize_grads(False)
        return out, scalars[0], scalars[1], idx

    @staticmethod
    def backward(ctx, g_out, g_loss, g_perp, _g_idx):
        z, codebook, idx = ctx.saved_tensors
        if g_out is not None:
            g_out = g_out.contiguous()
        if g_loss is None:
            g_loss = torch.zeros(1, device=z.device)
        dz, dw = ops.vq_backward(z, codebook.detach(), idx, g_out, g_loss.reshape(1).contiguous(), ctx.cc,
                                 want_dz=ctx.needs_input_grad[0])
        return dz, (dw if ctx.needs_input_grad[1] else None), None, None


def _recon_input_grad(cx, channel_var, gscale):
    """d(recon_loss) / d(inputs) of vq_vae.py:320-322 -- mean(((decoded - inputs) * mask)^2 / channel_var) -- for callers that
    differentiate w.r.t. the patches (saliency maps; the reference's training never does): 2 (inputs - decoded) mask^2 /
    (N channel_var), times the upstream gradient.  Plain elementwise torch on the device tensors the forward kept."""
    if gscale is None or cx.x is None or getattr(cx, "dec", None) is None:
        return None
    x, dec = cx.x, cx.dec
    g = (x - dec) * (2.0 / x.numel())
    if cx.mask is not None:
        g = g * (cx.mask * cx.mask)
    if channel_var is not None:
        g = g / channel_var.detach().reshape(1, -1, 1, 1)
    return g * gscale.reshape(())


def _decoder_stage_fn(forward, backward):
    """The autograd Function of a decoder stage, (zq, x, mask, layers, *params) -> (decoded, and when x is given the masked
    reconstruction loss of vq_vae.py:320-322, else None), on an engine pair forward(layers, zq, x, mask) -> (decoded, cx) and
    backward(layers, cx, gscale, g_dec, G, want the gradient w.r.t. zq) -> g_zq."""
    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, zq, x, mask, layers, *params):
            dec, cx = forward(layers, zq, x, mask)
            ctx.layers, ctx.cx, ctx.params = layers, cx, params
            ctx.set_materialize_grads(False)
            if x is None:
                return dec, None
            B, NIN, H, W = x.shape
            zeros = torch.zeros(2, device=x.device)
            recon = ops.loss_finalize(cx.loss_slabs, B * NIN * H * W, zeros, 1.0, 0.0)[0]
            return dec, recon

        @staticmethod
        def backward(ctx, g_dec, g_recon):
            G = _GradBag()
            gscale = g_recon.reshape(1).contiguous() if g_recon is not None else None
            if g_dec is not None:
                g_dec = g_dec.contiguous()
            if gscale is None and g_dec is None:
                return (None,) * (4 + len(ctx.params))
            g_x = _recon_input_grad(ctx.cx, ctx.layers.channel_var, gscale) if ctx.needs_input_grad[1] else None
            g_zq = backward(ctx.layers, ctx.cx, gscale, g_dec, G, ctx.needs_input_grad[0])
            ctx.cx = None
            return (g_zq, g_x, None, None) + G.grads_for(ctx.params, ctx.needs_input_grad[4:])
    return Fn


_DecoderFn = _decoder_stage_fn(E.decoder_forward, E.decoder_backward)
_Z32TailFn = _decoder_stage_fn(E.z32_tail_forward, E.z32_tail_backward)     # dec[1:5] of VQ_VAE_z32: ConvT BN ReLU ConvT


# ================================================================================ modules
class _PairMSDFn(torch.autograd.Function):
    """sim[i][j] = mean((z[i] - z[j])**2)  (vq_vae.py:327-329) on the HIP kernels dm_pair_msd(_backward)."""

    @staticmethod
    def forward(ctx, zf):
        _require_gpu(zf, "time-matching loss")
        z = zf.detach().contiguous().float()
        ctx.save_for_backward(z)
        return ops.pair_msd(z)

    @staticmethod
    def backward(ctx, g_sim):
        (z,) = ctx.saved_tensors
        return ops.pair_msd_backward(z, g_sim.contiguous().float())


class _TimeMatchingFn(torch.autograd.Function):
    """The time-matching loss as ONE op: Gram matrix on the MFMA, the loss form of the model family (mode 0:
    vq_vae.py:330-331; mode 1: vae.py:327-336) in the kernel's epilogue, the backward a second MFMA product
    (dm_time_matching_forward / _backward).  Returns the scalar loss."""

    @staticmethod
    def forward(ctx, zf, tm, mode, w_a, w_t, w_n, margin):
        _require_gpu(zf, "time-matching loss")
        z = zf.detach().contiguous().float()
        loss, S = ops.time_matching_forward(z, tm.detach().contiguous().float(), mode, w_a, w_t, w_n, margin)
        ctx.save_for_backward(z, S)
        ctx.tm_state = getattr(S, "_dm_tm_state", None)     # (saved tensors come back as new objects: attributes do not)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        z, S = ctx.saved_tensors
        if ctx.tm_state is not None:
            S._dm_tm_state = ctx.tm_state
        return (ops.time_matching_backward(z, S, g.reshape(1).contiguous().float()),) + (None,) * 6


def time_matching_loss(latents, time_matching_mat, z16_form, w_a=0.0, w_t=0.0, w_n=0.0, margin=0.0):
    """latents (B, ...) -> scalar loss of the pairwise term; the reference's expressions when the MFMA kernels do not tile
    the latent length (n % 32 != 0): distances from dm_pair_msd, weights / hinge / reduction in torch."""
    zf = latents.reshape((latents.shape[0], -1))
    assert (zf.shape[0], zf.shape[0]) == tuple(time_matching_mat.shape)
    if ops.time_matching_supported(zf.shape[0], zf.shape[1]):
        return _TimeMatchingFn.apply(zf, time_matching_mat, 1 if z16_form else 0, float(w_a), float(w_t), float(w_n), float(margin))
    sim_mat = _PairMSDFn.apply(zf)
    if not z16_form:
        return (sim_mat * time_matching_mat).sum()                          # vq_vae.py:331
    wts = time_matching_mat.clone()                                          # vae.py:327-335
    wts[time_matching_mat == 2] = w_a
    wts[time_matching_mat == 1] = w_t
    wts[time_matching_mat == 0] = w_n
    val = sim_mat * wts
    val = torch.where(time_matching_mat == 0, torch.clamp(val + margin, min=0), val)
    return val.mean()


class VectorQuantizer(nn.Module):
    """Vector quantizer of "Neural Discrete Representation Learning" (reference vq_vae.py:25-116).

    ema_decay (None: the reference's module, the codebook trained by the gradient of q_latent_loss): a decay in [0, 1) turns
    on the paper's exponential-moving-average codebook update (appendix A.1).  The codebook `w.weight` is then
    a frozen parameter under its old name, the buffers `ema_cluster_size` N (K) and `ema_w` m (K, D) start at N = 1, m = e,
    the loss is commitment_cost * mse(q.detach(), z), and in train() mode every forward with gradients enabled ends with
        n[k] = #{p: idx[p] = k};  s[k] = sum of the z assigned to k
        N <- g N + (1 - g) n;  m <- g m + (1 - g) s;  e[k] <- m[k] / ((N[k] + eps) / (sum N + K eps) * sum N)
    in place under no_grad.  Nothing is updated in eval() mode, under torch.no_grad() or by encode_inputs / decode_inputs.  The counts travel as
    fp32: exact up to 2^24 positions per code and step."""

    def __init__(self, embedding_dim=128, num_embeddings=128, commitment_cost=0.25, device='cuda:0',
                 ema_decay=None, ema_epsilon=1e-5):
        super(VectorQuantizer, self).__init__()
        self.embedding_dim = embedding_dim
        self.num_embeddings = num_embeddings
        self.commitment_cost = commitment_cost
        self.device = device
        self.w = nn.Embedding(num_embeddings, embedding_dim)
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"VectorQuantizer: ema_decay must be None or in [0, 1), got {ema_decay}")
        if float(ema_epsilon) < 0.0:
            raise ValueError(f"VectorQuantizer: ema_epsilon must be >= 0, got {ema_epsilon}")
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_epsilon = float(ema_epsilon)
        if self.ema:
            self.w.weight.requires_grad_(False)
            self.register_buffer("ema_cluster_size", torch.ones(num_embeddings))
            self.register_buffer("ema_w", self.w.weight.detach().clone())

    @property
    def ema(self):
        return getattr(self, "ema_decay", None) is not None      # (a module pickled before the mode existed has no attribute)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """A checkpoint without the two EMA buffers (the reference's format, or a gradient-trained model of this package)
        loads into an EMA module: the buffers take the initial state of the loaded codebook, N = 1 and m = e."""
        if self.ema:
            w = state_dict.get(prefix + "w.weight")
            if w is not None and tuple(w.shape) == tuple(self.w.weight.shape):
                if prefix + "ema_cluster_size" not in state_dict and prefix + "ema_w" not in state_dict:
                    state_dict[prefix + "ema_cluster_size"] = torch.ones_like(self.ema_cluster_size)
                    state_dict[prefix + "ema_w"] = w.detach().clone()
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def ema_statistics(self, z, idx):
        """(K * (D + 1),) device tensor: the K * D sums of the z assigned to each code, then the K counts (as floats), of
        this batch -- the new backward kernel without its dz, its slabs reduced in slab order."""
        _, slabs = ops.vq_backward_stats(z, self.w.weight.detach(), idx, None, None, float(self.commitment_cost), want_dz=False)
        return ops.reduce_slabs(slabs, torch.empty(slabs.shape[1], device=z.device))

    def ema_apply(self, stats):
        """The update from a batch's (global) statistics, in place, one launch."""
        ops.vq_ema_apply(stats, self.ema_cluster_size, self.ema_w, self.w.weight.data, self.ema_decay, self.ema_epsilon)

    def _quantize(self, z, commitment_cost=None):
        """(output_quantized, loss, perplexity, idx) of a prepared z.  In the EMA mode a training forward -- train() mode
        with gradients enabled; the validation pass of the training loop runs under no_grad -- ends with the update."""
        cc = float(self.commitment_cost if commitment_cost is None else commitment_cost)
        out, loss, perplexity, idx = _VQFn.apply(z, self.w.weight, cc, self.ema)
        if self.ema and self.training and torch.is_grad_enabled():
            if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
                raise ValueError("VectorQuantizer: the EMA codebook update on the autograd route forms its statistics from "
                                 "this process's batch only; with more than one rank train with FusedTrainer (fused=True), "
                                 "whose statistics ride the step's all-reduce")
            with torch.no_grad():
                self.ema_apply(self.ema_statistics(z.detach(), idx))
        return out, loss, perplexity, idx

    def forward(self, inputs):
        """inputs (B, D, H, W) -> (output_quantized, loss, perplexity)   [vq_vae.py:52-84]"""
        _require_gpu(inputs, "VectorQuantizer.forward")
        out, loss, perplexity, _ = self._quantize(_prep(inputs))
        assert out.shape == inputs.shape
        return out, loss, perplexity

    @property
    def embeddings(self):
        return self.w.weight

    def encode_inputs(self, inputs):
        """Index tensor (B, H, W) int64 of the nearest embedding vectors   [vq_vae.py:90-103]"""
        _require_gpu(inputs, "VectorQuantizer.encode_inputs")
        idx, _, _, _ = ops.vq_forward(_prep(inputs.detach()), self.w.weight.detach(), want_out=False)
        return idx

    def decode_inputs(self, encoding_indices):
        """Quantized encodings (B, D, H, W) assembled from indices   [vq_vae.py:105-116]"""
        _require_gpu(encoding_indices, "VectorQuantizer.decode_inputs")
        return ops.vq_decode(encoding_indices.contiguous(), self.w.weight.detach())


def _held(base):
    """A layer of the reference's nn.Sequential kept as a PARAMETER CONTAINER: same class hierarchy, constructor, parameter
    and buffer names (the state-dict contract), but calling it directly raises -- the arithmetic of the path runs in the HIP
    pipeline of the parent (`model.enc`, `model.dec`, `ResidualBlock`), and a child called on its own would silently be
    ATen / MIOpen, i.e. a fallback."""
    class Held(base):
        def forward(self, *args, **kwargs):
            raise RuntimeError(f"{base.__name__} inside dynamorph_amd is a parameter container of the HIP pipeline: call the "
                               "enclosing module (model.enc / model.dec / ResidualBlock); there is no ATen fallback")
    Held.__name__ = base.__name__              # what a reader of repr(model) / type(layer).__name__ sees: the reference's
    Held.__qualname__ = "_" + base.__name__     # where pickle finds the class again: the module-level names below
    return Held


_Conv2d, _ConvTranspose2d, _BatchNorm2d, _ReLU = (_held(nn.Conv2d), _held(nn.ConvTranspose2d), _held(nn.BatchNorm2d),
                                                  _held(nn.ReLU))


def _res_layer(num_hiddens, num_residual_hiddens):
    return nn.Sequential(
        _ReLU(),
        _Conv2d(num_hiddens, num_residual_hiddens, 3, padding=1),
        _BatchNorm2d(num_residual_hiddens),
        _ReLU(),
        _Conv2d(num_residual_hiddens, num_hiddens, 1),
        _BatchNorm2d(num_hiddens))


class ResidualBlock(nn.Module):
    """output = output + layers[i](output)   (reference vq_vae.py:180-225)."""

    def __init__(self, num_hiddens=128, num_residual_hiddens=512, num_residual_layers=2):
        super(ResidualBlock, self).__init__()
        self.num_hiddens = num_hiddens
        self.num_residual_layers = num_residual_layers
        self.num_residual_hiddens = num_residual_hiddens
        self.layers = nn.ModuleList([_res_layer(num_hiddens, num_residual_hiddens)
                                     for _ in range(num_residual_layers)])

    def _handles(self):
        return [(l[1], l[2], l[4], l[5]) for l in self.layers]

    def forward(self, x):
        _require_gpu(x, "ResidualBlock.forward")
        hs = self._handles()
        params = [p for ca, bna, cb, bnb in hs for p in (ca.weight, ca.bias, bna.weight, bna.bias,
                                                         cb.weight, cb.bias, bnb.weight, bnb.bias)]
        return _ResidualFn.apply(_prep(x), hs, *params)


class _HipEncoder(nn.Sequential):
    """`model.enc`: the nn.Sequential of the reference (same child indices), computed as one HIP pipeline."""

    per_sample_stats = False

    def forward(self, x):
        _require_gpu(x, "VQ_VAE.enc")
        layers = E.Layers(enc=self)
        return _EncoderFn.apply(_prep(x), layers, self.per_sample_stats, *layers.encoder_params())


class _HipDecoder(nn.Sequential):
    """`model.dec`."""

    def forward(self, z):
        _require_gpu(z, "VQ_VAE.dec")
        layers = E.Layers(dec=self)
        dec, _ = _DecoderFn.apply(_prep(z), None, None, layers, *layers.decoder_params())
        return dec


class VQ_VAE(nn.Module):
    """Vector-Quantized VAE with a 16 x 16 x num_hiddens latent (reference vq_vae.py:228-342)."""

    _z16_loss = False
    _layers_class = E.Layers         # (engine.layers_of)

    def __init__(self,
                 num_inputs=2,
                 num_hiddens=16,
                 num_residual_hiddens=32,
                 num_residual_layers=2,
                 num_embeddings=64,
                 commitment_cost=0.25,
                 channel_var=CHANNEL_VAR,
                 weight_recon=1.,
                 weight_commitment=1.,
                 weight_matching=0.005,
                 device="cuda:0",
                 w_a=1.1,
                 w_t=0.1,
                 w_n=-0.5,
                 margin=0.5,
                 ema_decay=None,
                 ema_epsilon=1e-5,
                 **kwargs):
        # callers pass gpu=True (pipeline/patch_VAE.py:431) or alpha/gpu (plot_scripts/recon_loss.py:18);
        # the reference forwards them to nn.Module.__init__ and crashes on current torch -- swallow them.
        for k in ("gpu", "alpha", "extra_loss"):
            kwargs.pop(k, None)
        super(VQ_VAE, self).__init__(**kwargs)
        self.num_inputs = num_inputs
        self.num_hiddens = num_hiddens
        self.num_residual_layers = num_residual_layers
        self.num_residual_hiddens = num_residual_hiddens
        self.num_embeddings = num_embeddings
        self.commitment_cost = commitment_cost
        self.channel_var = nn.Parameter(
            torch.from_numpy(np.asarray(channel_var, dtype=np.float64)).float().reshape((1, num_inputs, 1, 1)),
            requires_grad=False)
        self.weight_recon = weight_recon
        self.weight_commitment = weight_commitment
        self.weight_matching = weight_matching
        self.w_a, self.w_t, self.w_n, self.margin = w_a, w_t, w_n, margin
        nh = num_hiddens
        self.enc = _HipEncoder(
            _Conv2d(num_inputs, nh // 2, 1),
            _Conv2d(nh // 2, nh // 2, 4, stride=2, padding=1),
            _BatchNorm2d(nh // 2),
            _ReLU(),
            _Conv2d(nh // 2, nh, 4, stride=2, padding=1),
            _BatchNorm2d(nh),
            _ReLU(),
            _Conv2d(nh, nh, 4, stride=2, padding=1),
            _BatchNorm2d(nh),
            _ReLU(),
            _Conv2d(nh, nh, 3, padding=1),
            _BatchNorm2d(nh),
            ResidualBlock(nh, num_residual_hiddens, num_residual_layers))
        self.vq = VectorQuantizer(nh, num_embeddings, commitment_cost=commitment_cost, device=device,
                                  ema_decay=ema_decay, ema_epsilon=ema_epsilon)
        self.dec = _HipDecoder(
            _ConvTranspose2d(nh, nh // 2, 4, stride=2, padding=1),
            _ReLU(),
            _ConvTranspose2d(nh // 2, nh // 4, 4, stride=2, padding=1),
            _ReLU(),
            _ConvTranspose2d(nh // 4, nh // 4, 4, stride=2, padding=1),
            _ReLU(),
            _Conv2d(nh // 4, num_inputs, 1))

    # ---- the pairwise term (vq_vae.py:324-332; weighted / hinge form of VQ_VAE_z16, vae.py:322-336): one fused op ----
    def _time_matching(self, z_before, time_matching_mat):
        return time_matching_loss(z_before, time_matching_mat, self._z16_loss, getattr(self, "w_a", 0.0),
                                  getattr(self, "w_t", 0.0), getattr(self, "w_n", 0.0), getattr(self, "margin", 0.0))

    def forward(self, inputs, time_matching_mat=None, batch_mask=None):
        """inputs (B, C, H, W) -> (decoded, loss dict)   [vq_vae.py:300-338]"""
        _require_gpu(inputs, "VQ_VAE.forward")
        x = _prep(inputs)
        layers = E.Layers(self)
        z_before = _EncoderFn.apply(x, layers, self.enc.per_sample_stats, *layers.encoder_params())
        if self.vq.ema:        # (the update follows in train() mode)
            z_after, c_loss, perplexity, _ = self.vq._quantize(z_before, self.commitment_cost)
        else:
            z_after, c_loss, perplexity, _ = _VQFn.apply(z_before, self.vq.w.weight, float(self.commitment_cost))
        mask = _prep(batch_mask) if batch_mask is not None else None
        decoded, recon_loss = _DecoderFn.apply(z_after, x, mask, layers, *layers.decoder_params())
        total_loss = self.weight_recon * recon_loss + self.weight_commitment * c_loss
        time_matching_loss = 0.
        if time_matching_mat is not None:
            time_matching_loss = self._time_matching(z_before, time_matching_mat)
            total_loss = total_loss + self.weight_matching * time_matching_loss
        if self._z16_loss:
            return decoded, {'recon_loss': recon_loss, 'commitment_loss': c_loss,
                             'time_matching_loss': time_matching_loss, 'perplexity': perplexity,
                             'total_loss': total_loss}
        return decoded, {'recon_loss': recon_loss, 'commitment_loss': c_loss,
                         'time_matching_loss': time_matching_loss, 'total_loss': total_loss,
                         'perplexity': perplexity}

    def predict(self, inputs):
        """Prediction fn, same as forward pass."""
        return self.forward(inputs)


class VQ_VAE_z16(VQ_VAE):
    """vae.py:216-346: same network and state dict as VQ_VAE; weighted hinge time-matching loss and
    'perplexity' listed before 'total_loss'."""
    _z16_loss = True


# ================================================================================ VQ_VAE_z32
class _Z32Encoder(nn.Sequential):
    """`model.enc` of VQ_VAE_z32 (same child indices as the reference's nn.Sequential): the stem as one autograd node, then
    the ResidualBlock module."""

    def forward(self, x):
        _require_gpu(x, "VQ_VAE_z32.enc")
        L = E.Z32Layers(enc=self)
        return L.enc_block(_Z32StemFn.apply(_prep(x), L, False, *L.stem_params()))


def _z32_decode(L, z, x, mask):
    """The ResidualBlock module, then the tail as one autograd node -> (decoded, recon_loss or None)."""
    return _Z32TailFn.apply(L.dec_block(z), x, mask, L, *L.tail_params())


class _Z32Decoder(nn.Sequential):
    """`model.dec` of VQ_VAE_z32."""

    def forward(self, z):
        _require_gpu(z, "VQ_VAE_z32.dec")
        # (no loss here, so the channel variances are not needed: `model.dec` holds no reference to its parent)
        return _z32_decode(E.Z32Layers(dec=self), _prep(z), None, None)[0]


class VQ_VAE_z32(nn.Module):
    """Vector-Quantized VAE with a 32 x 32 x num_hiddens latent (reference vae.py:348-474): two stride-2 convs and a
    residual stack in the encoder, a residual stack, BatchNorm and two transposed convs in the decoder, the
    weighted-hinge time-matching loss on z_after.  The default widths (num_hiddens 16, num_residual_hiddens 32) run on the
    register-resident kernels, any other width (config_example.yml: 64 / 64 / 512 codes) on the implicit-GEMM kernels of
    csrc/conv_wide.hip."""

    _layers_class = E.Z32Layers      # (engine.layers_of)

    def __init__(self, num_inputs=2, num_hiddens=16, num_residual_hiddens=32, num_residual_layers=2, num_embeddings=64,
                 commitment_cost=0.25, channel_var=np.ones(2), weight_matching=0.005, w_a=1.1, w_t=0.1, w_n=-0.5,
                 margin=0.5, extra_loss=None, device="cuda:0", ema_decay=None, ema_epsilon=1e-5, **kwargs):
        kwargs.pop("gpu", None)
        alpha = kwargs.pop("alpha", None)
        super(VQ_VAE_z32, self).__init__(**kwargs)
        if extra_loss is not None and not (isinstance(extra_loss, dict) and all(callable(f) for f in extra_loss.values())):
            raise TypeError("extra_loss: None or {loss name: callable(labels, z_after_flat) -> (loss, frac_pos)}  [vae.py:382-383]")
        # vae.py:467 multiplies every extra loss by self.alpha, which the reference's constructor never sets (its docstring
        # lists `alpha`, its signature does not: the attribute has to be assigned by the caller).  Here `alpha=` is accepted
        # and stored; without it the attribute is missing exactly as in the reference.
        if alpha is not None:
            self.alpha = alpha
        self.num_inputs = num_inputs
        self.num_hiddens = num_hiddens
        self.num_residual_layers = num_residual_layers
        self.num_residual_hiddens = num_residual_hiddens
        self.num_embeddings = num_embeddings
        self.commitment_cost = commitment_cost
        self.channel_var = nn.Parameter(
            torch.from_numpy(np.asarray(channel_var, dtype=np.float64)).float().reshape((1, num_inputs, 1, 1)),
            requires_grad=False)
        self.weight_matching = weight_matching
        self.w_a, self.w_t, self.w_n, self.margin = w_a, w_t, w_n, margin
        nh = num_hiddens
        self.enc = _Z32Encoder(
            _Conv2d(num_inputs, nh // 2, 4, stride=2, padding=1),
            _BatchNorm2d(nh // 2),
            _ReLU(),
            _Conv2d(nh // 2, nh, 4, stride=2, padding=1),
            _BatchNorm2d(nh),
            ResidualBlock(nh, num_residual_hiddens, num_residual_layers))
        self.vq = VectorQuantizer(nh, num_embeddings, commitment_cost=commitment_cost, device=device,
                                  ema_decay=ema_decay, ema_epsilon=ema_epsilon)
        self.dec = _Z32Decoder(
            ResidualBlock(nh, num_residual_hiddens, num_residual_layers),
            _ConvTranspose2d(nh, nh // 2, 4, stride=2, padding=1),
            _BatchNorm2d(nh // 2),
            _ReLU(),
            _ConvTranspose2d(nh // 2, num_inputs, 4, stride=2, padding=1))
        self.extra_loss = extra_loss

    def forward(self, inputs, labels=None, time_matching_mat=None, batch_mask=None):
        """inputs (B, C, H, W) -> (decoded, loss dict)   [vae.py:430-470].  extra_loss (vae.py:463-469): every
        `loss_fn(labels, z_after.reshape(B, -1)) -> (loss, frac_pos)` is the caller's torch code on the device latents; its
        gradient reaches the encoder through the quantiser's straight-through backward like the time-matching term's."""
        _require_gpu(inputs, "VQ_VAE_z32.forward")
        x = _prep(inputs)
        z_before = self.enc(x)
        z_after, c_loss, perplexity = self.vq(z_before)
        mask = _prep(batch_mask) if batch_mask is not None else None
        decoded, recon_loss = _z32_decode(E.Z32Layers(self), z_after, x, mask)
        total_loss = recon_loss + c_loss
        if time_matching_mat is not None:
            tml = time_matching_loss(z_after, time_matching_mat, True, self.w_a, self.w_t, self.w_n, self.margin)   # vae.py:441-455
            total_loss = total_loss + tml * self.weight_matching
        else:
            tml = 0
        loss_dict = {'recon_loss': recon_loss, 'commitment_loss': c_loss,
                     'time_matching_loss': tml, 'perplexity': perplexity,
                     'total_loss': total_loss}
        if self.extra_loss is not None:                                   # vae.py:463-469
            z_after_ = z_after.reshape((z_after.shape[0], -1))
            for loss_name, loss_fn in self.extra_loss.items():
                extra_loss, frac_pos = loss_fn(labels, z_after_)
                total_loss = total_loss + extra_loss * self.alpha
                loss_dict['total_loss'] = total_loss
                loss_dict[loss_name] = extra_loss
        return decoded, loss_dict

    def predict(self, inputs):
        """Prediction fn, same as forward pass."""
        return self.forward(inputs)
