"""Kernel orchestration for the VQ-VAE path: which HIP kernel runs on which tensor, in what order.

Every function here only enqueues kernels from libdynamorph_hip.so on the current stream (via
dynamorph_amd.ops); there is no ATen math and no host synchronisation, so a whole training step
can be captured into a HIP graph.

Layer map (reference HiddenStateExtractor/vq_vae.py:276-298, ResidualBlock :203-224):
  enc.0 (1x1) o enc.1 (4x4/s2)  -> ONE 4x4/s2 conv on (x, 1): the composite weight is rebuilt
                                    from the stored parameters every call (dm_e1_compose); the
                                    ones channel carries enc.0's bias through the zero padding.
  enc.2/3, enc.5/6, enc.8/9      -> BatchNorm(+ReLU) folded into the NEXT conv's operand load;
                                    the producing conv's epilogue emits the (sum, sum^2) slabs.
  enc.10, enc.11, enc.12         -> 3x3 conv, BN, residual stack (3x3 -> BN -> ReLU -> 1x1 -> BN, + skip)
  dec.0/2/4 (ConvTranspose 4/2/1)-> 3x3-neighbourhood conv with N = 4 phases x Cout + pixel shuffle
  dec.6 (1x1) + recon loss       -> fused VALU head kernel

Backward mirrors it: each conv layer = one data-gradient kernel (whose epilogue applies the ReLU
mask, joins the residual branch and emits the BatchNorm-backward reductions) + one weight-gradient
kernel; BatchNorm backward itself is an AFFINE2 operand load.  Biases of convs that feed a
train-mode BatchNorm have an identically zero gradient (the batch mean removes them) and are
written as exact zeros.
"""
from types import SimpleNamespace

import torch

from . import ops
from .ops import DM_LOAD_AFFINE, DM_LOAD_AFFINE2, DM_LOAD_AFFINE_RELU, DM_LOAD_IDENT, DM_LOAD_RELU, Op, weight_view


FUSED_BACKWARD = True     # False: the two-launch pairs everywhere (two tests in test_gpu_model.py monkeypatch it)


class Layers:
    """Parameter handles resolved from a VQ_VAE-shaped nn.Module (state-dict names of the reference), or from one of its
    halves: `model.enc` / `model.dec` called on their own build Layers(enc=self) / Layers(dec=self) -- no back-reference
    to the parent, so copy.deepcopy(model) and pickling give an independent, working module."""

    latent_stride = 8            # patch pixels per latent position: three stride-2 convolutions
    latent_after_vq = False      # the latents of the pairwise term and of the inference drivers' cotangents: z_before

    def __init__(self, model=None, enc=None, dec=None):
        if model is not None:
            enc, dec = model.enc, model.dec
            self.loss_weights = (float(model.weight_recon), float(model.weight_commitment))     # of (recon, commitment) in total
        self.codebook = model.vq.w if model is not None else None
        self.channel_var = model.channel_var if model is not None else None
        if enc is not None:
            self.enc0, self.enc1, self.bn1 = enc[0], enc[1], enc[2]
            self.enc4, self.bn2 = enc[4], enc[5]
            self.enc7, self.bn3 = enc[7], enc[8]
            self.enc10, self.bn4 = enc[10], enc[11]
            self.res = enc[12]._handles()
            self.nin, self.nh = self.enc0.weight.shape[1], self.enc10.weight.shape[0]
            self.nrh = self.res[0][0].weight.shape[0] if self.res else 0
        if dec is not None:
            self.dec0, self.dec2, self.dec4, self.dec6 = dec[0], dec[2], dec[4], dec[6]
            if enc is None:
                self.nin, self.nh = self.dec6.weight.shape[0], self.dec0.weight.shape[0]

    def encoder_params(self):
        ps = [self.enc0.weight, self.enc0.bias, self.enc1.weight, self.enc1.bias, self.bn1.weight, self.bn1.bias,
              self.enc4.weight, self.enc4.bias, self.bn2.weight, self.bn2.bias,
              self.enc7.weight, self.enc7.bias, self.bn3.weight, self.bn3.bias,
              self.enc10.weight, self.enc10.bias, self.bn4.weight, self.bn4.bias]
        for ca, bna, cb, bnb in self.res:
            ps += [ca.weight, ca.bias, bna.weight, bna.bias, cb.weight, cb.bias, bnb.weight, bnb.bias]
        return ps

    def decoder_params(self):
        return [self.dec0.weight, self.dec0.bias, self.dec2.weight, self.dec2.bias,
                self.dec4.weight, self.dec4.bias, self.dec6.weight, self.dec6.bias]


class Z32Layers:
    """The twin of Layers for VQ_VAE_z32 (vae.py:348-474), again without a back-reference to the parent.  The child indices of
    its two nn.Sequentials are spelled here and nowhere else: enc = conv0 bn0 ReLU conv1 bn1 enc_block, dec = dec_block up0 bn_up
    ReLU up1.  enc_block / dec_block: the ResidualBlock modules; enc_res / dec_res: their handles (residual_forward / _backward)."""

    latent_stride = 4            # two stride-2 convolutions
    latent_after_vq = True       # the pairwise term acts on z_after (vae.py:441-455)
    loss_weights = (1.0, 1.0)    # total = recon + commitment (vae.py:457)

    def __init__(self, model=None, enc=None, dec=None):
        if model is not None:
            enc, dec = model.enc, model.dec
        self.codebook = model.vq.w if model is not None else None
        self.channel_var = model.channel_var if model is not None else None
        if enc is not None:
            self.conv0, self.bn0, self.conv1, self.bn1, self.enc_block = enc[0], enc[1], enc[3], enc[4], enc[5]
            self.enc_res = self.enc_block._handles()
            self.nin, self.nh = self.conv0.weight.shape[1], self.conv1.weight.shape[0]
        if dec is not None:
            self.dec_block, self.up0, self.bn_up, self.up1 = dec[0], dec[1], dec[2], dec[4]
            self.dec_res = self.dec_block._handles()
            if enc is None:
                self.nin, self.nh = self.up1.weight.shape[1], self.up0.weight.shape[0]

    def stem_params(self):
        return [p for m in (self.conv0, self.bn0, self.conv1, self.bn1) for p in (m.weight, m.bias)]

    def tail_params(self):
        return [p for m in (self.up0, self.bn_up, self.up1) for p in (m.weight, m.bias)]


def layers_of(model, who=None):
    """The Layers object of a model of either family (the models name their class: VQ_VAE._layers_class).  Any other module:
    TypeError in the name of the caller `who`; who=None: None (encode_patches runs such a module as it is)."""
    cls = getattr(model, "_layers_class", None)
    if cls is None and who is not None:
        raise TypeError("{}: {} is not built on the HIP path (VQ_VAE, VQ_VAE_z16, VQ_VAE_z32)".format(who, type(model).__name__))
    return None if cls is None else cls(model)


# ------------------------------------------------------------------------- BatchNorm glue
# The synchronized-BatchNorm context of the step being enqueued (a BnSync), or None: every training-mode BatchNorm with batch
# statistics then normalises with the statistics of the global batch.  Set by FusedTrainer (bn_sync); None is the default.
_bn_sync = None


class bn_sync:
    """with bn_sync(ctx): the BatchNorm glue below routes through ctx (None: unchanged)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        global _bn_sync
        self.prev, _bn_sync = _bn_sync, self.ctx
        return self.ctx

    def __exit__(self, *exc):
        global _bn_sync
        _bn_sync = self.prev


class BnSync:
    """Statistics of the global batch for data-parallel training (nn.SyncBatchNorm's arithmetic).
    weights: float64 device tensor [forward weight, gradient weight] -- 1 and grad_weight for a rank with data, 0 and 0 for a
    rank that only joins the exchanges.  exchange(payload): the caller's SUM over ranks of a float64 payload, in place (inline
    all-reduce; during a graph capture: the end of a segment).  One exchange per layer and direction, in launch order."""

    def __init__(self, weights, exchange):
        self.weights, self.exchange = weights, exchange
        self.fwd = {}                     # BatchNorm module -> its all-reduced forward payload (the global count)

    def forward(self, stats, bn, count):
        payload = ops.bn_sync_pack(stats, count, self.weights[0:1])
        self.exchange(payload)
        self.fwd[bn] = payload
        return ops.bn_finalize_payload(payload, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                                       bn.num_batches_tracked, _momentum(bn), bn.eps)

    def backward(self, stats, bn, saved, G):
        payload = ops.bn_backward_pack(stats, saved, self.weights[1:2], G(bn.weight), G(bn.bias))
        self.exchange(payload)
        return ops.bn_backward_payload(payload, self.fwd[bn], bn.weight.detach(), saved, self.weights[1:2])


def _momentum(bn):
    return 0.1 if bn.momentum is None else bn.momentum


def _bn_coef(stats, bn, count, per_sample, nbatch, defer=None):
    """Batch statistics -> (coef, saved).  eval() mode (never used by the reference path) takes the
    running statistics instead; its coefficients are three tiny device ops, no HIP kernel needed.
    defer: list collecting the running-statistics updates of the per-sample path (ops.bn_running_replay)."""
    if _bn_sync is not None and bn.training and not per_sample:
        return _bn_sync.forward(stats, bn, count)
    if not bn.training:
        invstd = torch.rsqrt(bn.running_var + bn.eps)
        scale = bn.weight.detach() * invstd
        coef = torch.stack([scale, torch.zeros_like(scale), bn.bias.detach() - bn.running_mean * scale,
                            torch.zeros_like(scale)], 1).contiguous()
        return coef, torch.stack([bn.running_mean, invstd], 1).contiguous()     # what _bn_backward takes in eval() mode
    spg = stats.shape[0] // nbatch if per_sample else 1
    return ops.bn_finalize(stats, count, bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                           bn.num_batches_tracked, _momentum(bn), bn.eps, per_sample=per_sample, slabs_per_group=spg,
                           defer=defer if per_sample else None)


def _w(p):
    return p.detach()


def view_strides(shape, swapped):
    """(sn, sc, sky, skx, off) of the dm_weight_view of a contiguous weight (A, Bc, k, k), k = 4, 3 or 1.  Stored order: the
    output index is dim 0 (a Conv2d forward, a ConvTranspose2d's data gradient).  Swapped: the output index is dim 1 (a
    Conv2d's data gradient, a ConvTranspose2d forward); the 3x3 taps are then flipped, the 4x4 ones are not -- the
    phase-decomposed kernels do that themselves."""
    _, bc, k, _ = shape
    d0, d1 = bc * k * k, k * k
    sky, skx = (k, 1) if k > 1 else (0, 0)
    if not swapped:
        return d0, d1, sky, skx, 0
    if k == 3:
        return d1, d0, -sky, -skx, 8
    return d1, d0, sky, skx, 0


def _view(w):
    return weight_view(_w(w), *view_strides(w.shape, False))


def _view_swapped(w):
    return weight_view(_w(w), *view_strides(w.shape, True))


def _no_grads(p):
    """G of a data-only backward pass (want_param_grads=False): no parameter has a gradient buffer, nothing is written."""
    return None


def _bn_backward(stats, count, bn, saved, g, a, G, gbias=None, zero=True, nbatch=0):
    """One BatchNorm-backward step: native_batch_norm_backward's reductions for `bn` from the (sum g, sum g * a) slabs ->
    da = BatchNorm backward of g as an AFFINE2 operand over the raw conv output a (its .coef: the coefficients); eval()
    mode (fixed statistics: count 0) keeps only da = gamma * invstd * g.  gbias: the gradient of the conv bias that feeds
    `bn`, written here (_fed_bias; None: the caller writes it where its launch belongs).
    nbatch = B > 0: per-sample statistics -- `stats` holds a whole number of slabs per patch, `count` is ONE patch's positions
    and `saved` (B, C, 2); patch b's da comes from patch b's own sums, the parameter gradients are the sums over the patches
    (ops.bn_backward_finalize_per_sample).  eval() mode shares its statistics and takes the batch form either way."""
    if nbatch and bn.training:
        c = ops.bn_backward_finalize_per_sample(stats, stats.shape[0] // nbatch, count, _w(bn.weight), saved,
                                                G(bn.weight), G(bn.bias))
    elif _bn_sync is not None and bn.training:
        c = _bn_sync.backward(stats, bn, saved, G)
    else:
        c = ops.bn_backward_finalize(stats, count if bn.training else 0, _w(bn.weight), saved, G(bn.weight), G(bn.bias))
    if gbias is not None:
        _fed_bias(gbias, bn, c, G, zero)
    return Op(g, DM_LOAD_AFFINE2, c, p1=a, per_sample=bool(nbatch))


# ------------------------------------------------------------------------------- encoder
_side_streams = {}


def _side_stream(device):
    """One helper stream per device for work that is off the critical path (the running-statistics replay)."""
    key = torch.device(device).index
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _side_streams[key]


def e1_operands(L):
    """(weff, bias_border) of the composite enc.0 o enc.1 convolution.  A function of the stored parameters only: the
    inference path builds them once per encode_patches call (weights do not change there), the training path every step."""
    return ops.e1_compose_border(_w(L.enc0.weight), _w(L.enc0.bias), _w(L.enc1.weight), _w(L.enc1.bias))


def encoder_forward(L, x, per_sample=False, e1=None, join=True, latents_only=False, defer_last_join=0, replay_as_latents=False):
    """x (B,NIN,H,W) -> z_before (B,nh,H/8,W/8).  per_sample=True normalises every BatchNorm with
    that sample's own statistics = pipeline/patch_VAE.py:445-452 (batch-of-one calls in train mode).
    e1: e1_operands(L) computed by the caller (inference: once per call).
    latents_only (per_sample only): the caller wants z and the running statistics, nothing to differentiate through --
    the 16 x 16 part of the encoder (enc.10 .. enc.12) then is ONE launch that keeps a patch on its CU
    (ops.latent_tail_forward) where that kernel is built.
    defer_last_join = K (training step only): when the quantiser can do it (ops.vq_forward_join_supported for K codes), the
    LAST residual join is left to the VectorQuantizer kernel's load path: the return value is then (None, cx) and
    cx.pending_join = (rb, h_in, coef) goes to vq_forward_joined, which also produces z.
    replay_as_latents (per_sample only, a context to differentiate through): where latents_only would take the one-launch
    latent tail, that kernel ALSO runs, for its per-patch sums alone: they, not the layer-by-layer slabs (equal up to the order
    of the additions), feed the running-statistics replay of enc.11 / enc.12, so the running statistics advance to the same
    bits as under encode_patches / score_patches.  The forward values and everything kept for backward are the chain's.
    join=False (per_sample only): the running-statistics replay -- a side effect no kernel of the path reads -- is left
    running on a helper stream beside whatever the caller launches next (the VectorQuantizer); the caller MUST call
    cx.join() before it hands the stream back (a HIP-graph capture cannot end with unjoined work)."""
    B, NIN, H, W = x.shape
    nh, nrh, c1 = L.nh, L.nrh, L.nh // 2
    ps = per_sample
    cx = SimpleNamespace(x=x, per_sample=ps, B=B, H=H, W=W, res=[], join=lambda: None)
    defer = [] if ps else None       # per-sample path: running statistics of all eight layers in one launch at the end

    # forward: K = 16*NIN; the ones channel of the composite is folded into a per-position bias table (bias_border)
    weff, border = e1 if e1 is not None else e1_operands(L)
    H1, W1 = H // 2, W // 2
    a1, st = ops.conv4x4s2(Op(x), _view(weff), B, NIN, c1, H, W, want_stats=True, bias_border=border, per_tile=ps)
    coef1, saved1 = _bn_coef(st, L.bn1, H1 * W1 * (1 if ps else B), ps, B, defer)

    H2, W2 = H1 // 2, W1 // 2
    a2, st = ops.conv4x4s2(Op(a1, DM_LOAD_AFFINE_RELU, coef1, per_sample=ps), _view(L.enc4.weight), B, c1, nh, H1, W1,
                           want_stats=True, bias=_w(L.enc4.bias), per_tile=ps)
    coef2, saved2 = _bn_coef(st, L.bn2, H2 * W2 * (1 if ps else B), ps, B, defer)

    H3, W3 = H2 // 2, W2 // 2
    n3 = H3 * W3 * (1 if ps else B)
    tail_built = (ps and (latents_only or replay_as_latents) and L.bn3.training and L.bn4.training
                  and all(bna.training and bnb.training for _, bna, _, bnb in L.res)
                  and ops.latent_tail_supported(nh, nrh, H3, W3, len(L.res)))
    fuse_tail = tail_built and latents_only
    a3, st = ops.conv4x4s2(Op(a2, DM_LOAD_AFFINE_RELU, coef2, per_sample=ps), _view(L.enc7.weight), B, nh, nh, H2, W2,
                           want_stats=True, bias=_w(L.enc7.bias), per_tile=ps)
    coef3, saved3 = _bn_coef(st, L.bn3, n3, ps, B, defer)
    cx.__dict__.update(a1=a1, a2=a2, a3=a3, coef1=coef1, coef2=coef2, coef3=coef3, saved1=None, dims=(H1, W1, H2, W2, H3, W3))

    if tail_built:
        z, st4, sts = ops.latent_tail_forward(
            a3, coef3, _w(L.enc10.weight), _w(L.enc10.bias), _w(L.bn4.weight), _w(L.bn4.bias), L.bn4.eps,
            [(_w(ca.weight), _w(ca.bias), _w(bna.weight), _w(bna.bias), bna.eps, _w(cb.weight), _w(cb.bias),
              _w(bnb.weight), _w(bnb.bias), bnb.eps) for ca, bna, cb, bnb in L.res])
        bns = [L.bn4] + [bn for _, bna, _, bnb in L.res for bn in (bna, bnb)]
        for slabs, bn in zip([st4] + [s for pair in sts for s in pair], bns):
            defer.append((slabs, 1, n3, bn.running_mean, bn.running_var, bn.num_batches_tracked, _momentum(bn)))
    if fuse_tail:
        _replay(cx, x, defer, join)
        return z, cx
    tail_defer = [] if tail_built else defer         # replay_as_latents: the chain's own updates of these layers are dropped
    a4, st = ops.conv3x3(Op(a3, DM_LOAD_AFFINE_RELU, coef3, per_sample=ps), _view(L.enc10.weight), B, nh, nh, H3, W3,
                         taps=9, want_stats=True, bias=_w(L.enc10.bias), per_tile=ps)
    coef4, saved4 = _bn_coef(st, L.bn4, n3, ps, B, tail_defer)
    h = ops.apply(Op(a4, DM_LOAD_AFFINE, coef4, per_sample=ps), B, nh, H3, W3)

    cx.__dict__.update(a4=a4, coef4=coef4, saved1=saved1, saved2=saved2, saved3=saved3, saved4=saved4)
    fuse = bool(defer_last_join) and not ps and len(L.res) > 0 and L.res[-1][3].training and \
        ops.vq_forward_join_supported(nh, int(defer_last_join), H3, W3)
    z, cx.res = residual_forward(L.res, h, ps, tail_defer, defer_last_join=fuse)
    cx.pending_join = (cx.res[-1].rb, cx.res[-1].h_in, cx.res[-1].coefb) if fuse else None
    _replay(cx, x, defer, join)
    return z, cx


def _replay(cx, x, defer, join):
    """The deferred running-statistics updates of the per-sample path, one launch on the helper stream."""
    if defer:
        cur = torch.cuda.current_stream(x.device)
        side = _side_stream(x.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for seg in defer:
                seg[0].record_stream(side)                 # the statistics slabs are read on the helper stream
            ops.bn_running_replay(defer)
        cx.join = lambda: cur.wait_stream(side)
        if join:
            cx.join()


def _need_per_sample_slabs(stats, B, route):
    """Per-sample BatchNorm statistics need the producing kernel's slabs grouped by sample (a whole number per sample); a
    route that hands back anything else cannot serve them -- an error that names the route, never batch statistics."""
    if stats is None or stats.shape[0] % B != 0:
        raise NotImplementedError("%s: this kernel route has no per-sample statistics (%s slabs for %d samples)"
                                  % (route, "no" if stats is None else stats.shape[0], B))


def residual_forward(res_layers, h, per_sample=False, defer=None, defer_last_join=False):
    """ResidualBlock.forward (vq_vae.py:212-225) on a materialised h (B,nh,H,W).
    defer: the caller's list of postponed running-statistics updates (per-sample path); None: flushed here.
    defer_last_join: the last layer's `h + BN(rb)` is NOT launched (the caller fuses it into its consumer); returns None
    for the output then."""
    B, nh, H, W = h.shape
    n = H * W * (1 if per_sample else B)
    saved = []
    own = defer is None and per_sample
    if own:
        defer = []
    for ca, bna, cb, bnb in res_layers:
        nrh = ca.weight.shape[0]
        ra, st = ops.conv3x3(Op(h, DM_LOAD_RELU), _view(ca.weight), B, nh, nrh, H, W, taps=9, want_stats=True, bias=_w(ca.bias),
                             per_tile=per_sample)
        if per_sample:
            _need_per_sample_slabs(st, B, "residual_forward: 3x3 convolution %d -> %d at %d x %d" % (nh, nrh, H, W))
        coefa, saveda = _bn_coef(st, bna, n, per_sample, B, defer)
        rb, st = ops.conv3x3(Op(ra, DM_LOAD_AFFINE_RELU, coefa, per_sample=per_sample), _view(cb.weight), B, nrh, nh, H, W,
                             taps=1, want_stats=True, bias=_w(cb.bias), per_tile=per_sample)
        if per_sample:
            _need_per_sample_slabs(st, B, "residual_forward: 1x1 convolution %d -> %d at %d x %d" % (nrh, nh, H, W))
        coefb, savedb = _bn_coef(st, bnb, n, per_sample, B, defer)
        last = defer_last_join and ca is res_layers[-1][0]
        hn = None if last else ops.apply(Op(rb, DM_LOAD_AFFINE, coefb, per_sample=per_sample), B, nh, H, W, resid=h)
        saved.append(SimpleNamespace(h_in=h, ra=ra, rb=rb, coefa=coefa, saveda=saveda, coefb=coefb, savedb=savedb,
                                     per_sample=per_sample))
        h = hn
    if own and defer:
        ops.bn_running_replay(defer)
    return h, saved


def _fed_bias(gbias, bn, coef_bwd, G, zero=True):
    """Gradient of a convolution bias that feeds the BatchNorm `bn`: identically zero in train mode (the batch mean removes a
    constant; zero=False: the caller's buffer holds the zero already); in eval() mode the sum of the BatchNorm's input
    gradient over the positions, gamma / sqrt(running_var + eps) * dbeta."""
    if gbias is None:                                # a data-only pass
        return
    if bn.training:
        if zero:
            gbias.zero_()
    else:
        torch.mul(coef_bwd[:, 0], G(bn.bias), out=gbias)


def _conv_backward_pair(dy, x, xcoef, w, gw, B, CD, CX, H, W, k, pending, like, stat_q, resid=None, want_stats=True,
                        between=lambda: None, per_sample=False):
    """The two-launch backward of a Conv2d CX -> CD (k = 3, 1: same size; k = 4: stride 2), for the shapes its fused kernel is
    not built for: the weight gradient of dy (B,CD,H,W) against the conv's input relu(BN(x)) (xcoef None: relu(x)), then the
    data gradient with that ReLU's mask, the residual branch `resid` and the (sum, sum * stat_q) slabs for the BatchNorm
    below.  between: a bias gradient whose launch sits between the two.  Returns (dx, stats).
    per_sample: xcoef is per patch and the slabs come back grouped by patch; gw None (a data-only pass): no weight gradient."""
    ps = per_sample
    xin, mask = (Op(x, DM_LOAD_RELU), Op(x)) if xcoef is None else (Op(x, DM_LOAD_AFFINE_RELU, xcoef, per_sample=ps),
                                                                   Op(x, DM_LOAD_AFFINE, xcoef, per_sample=ps))
    if gw is not None:
        ops.wgrad(dy, xin, gw, B, CD, CX, H, W, k, pending=pending)
    between()
    # (stride 2 backwards is the phase-decomposed transposed convolution: 4 phases x CX outputs, pixel-shuffled)
    per_tile = ps and want_stats
    dx, stats = ops.conv3x3(dy, _view_swapped(w), B, CD, 4 * CX if k == 4 else CX, H, W, taps=9 if k == 4 else k * k,
                            pixel_shuffle=k == 4, want_stats=want_stats, like=like, mask=mask, resid=resid, stat_q=stat_q,
                            **({"per_tile": True} if per_tile else {}))
    if per_tile:
        _need_per_sample_slabs(stats, B, "backward of the %d x %d convolution %d -> %d at %d x %d" % (k, k, CX, CD, H, W))
    return dx, stats


def residual_backward(res_layers, saved, g_h, G, q_below, pending=None, zero_fed_biases=True, want_param_grads=True,
                      per_sample=None):
    """Gradient of the residual stack.  g_h: gradient w.r.t. its output.  q_below: the raw conv output
    whose BatchNorm produced the stack's input (None if there is none); when given, the returned stats
    are the (sum g, sum g*q_below) slabs that BatchNorm's backward needs.  Returns (g_in, stats).
    A stack that ran with per_sample=True (its saved contexts say so; per_sample: for a stack without layers) goes backward
    per patch: every BatchNorm's backward takes that patch's own sums and count, the slabs are grouped by patch, and the
    fused kernels -- one coefficient set and one slab per persistent workgroup -- are not reached.
    want_param_grads=False: the data gradient alone; G is not called, no weight gradient is launched."""
    ps = bool(saved[0].per_sample if saved else per_sample)
    chan_stats = ops.channel_stats_per_sample if ps else ops.channel_stats
    if not want_param_grads:
        G = _no_grads
    if not saved:
        return g_h, (chan_stats(g_h, q_below) if q_below is not None else None)
    B, nh, H, W = g_h.shape
    cnt = H * W * (1 if ps else B)
    nb = B if ps else 0
    fused = FUSED_BACKWARD and not ps and want_param_grads
    stats = chan_stats(g_h, saved[-1].rb)
    for i in range(len(saved) - 1, -1, -1):
        ca, bna, cb, bnb = res_layers[i]
        s = saved[i]
        nrh = ca.weight.shape[0]
        da_rb = _bn_backward(stats, cnt, bnb, s.savedb, g_h, s.rb, G, G(cb.bias), zero_fed_biases, nbatch=nb)
        if fused and s.coefa.dim() == 2 and ops.conv1x1_bwd_fused_supported(nh, nrh, H, W):
            # the 1x1 convolution's data and weight gradient from ONE staging of (g_h, rb, ra) -- csrc/conv1x1_bwd.hip
            dy_ra, st = ops.conv1x1_bwd_fused(da_rb, s.ra, s.coefa, _w(cb.weight), G(cb.weight), B, nh, nrh, H, W, pending=pending)
        else:
            dy_ra, st = _conv_backward_pair(da_rb, s.ra, s.coefa, cb.weight, G(cb.weight), B, nh, nrh, H, W, 1, pending, like=g_h,
                                            stat_q=s.ra, per_sample=ps)
        da_ra = _bn_backward(st, cnt, bna, s.saveda, dy_ra, s.ra, G, G(ca.bias), zero_fed_biases, nbatch=nb)
        q = saved[i - 1].rb if i > 0 else q_below
        if fused and ops.conv3x3_bwd_fused_supported(nrh, nh, H, W):
            # the 3x3 convolution's data and weight gradient from ONE staging of the patch -- csrc/conv3x3_bwd.hip
            g_h, stats = ops.conv3x3_bwd_fused(da_ra, s.h_in, None, _w(ca.weight), G(ca.weight), B, nrh, resid=g_h, q=q,
                                               want_stats=q is not None, pending=pending)
        else:
            g_h, stats = _conv_backward_pair(da_ra, s.h_in, None, ca.weight, G(ca.weight), B, nrh, nh, H, W, 3, pending, like=g_h,
                                             stat_q=q, resid=g_h, want_stats=q is not None, per_sample=ps)
    return g_h, stats


def latent_stage_backward(L, cx, g_z, G, pending=None, zero_fed_biases=True, want_param_grads=True, fused=True):
    """The 16 x 16 stage of encoder_backward (on a 128 px patch), enc.12 .. enc.10: g_z (B,nh,H3,W3), the gradient at the
    encoder's output -> (dy3, stats): the gradient at enc.7's raw output a3, masked by relu(BN3(a3)), and its
    (sum dy3, sum dy3 * a3) slabs for enc.8's backward (grouped by patch on a per_sample context).  encoder_backward's own
    first step; also what the stage's tests and tools/gradbench.py call.
    A data-only pass on a per_sample context in train mode is ONE launch that keeps a patch on its CU
    (ops.latent_tail_backward) where that kernel is built; fused=False: the layer-by-layer launches there too."""
    if not hasattr(cx, "a4"):
        raise NotImplementedError("encoder_backward: this context was made with latents_only=True (nothing was kept to "
                                  "differentiate through)")
    if not want_param_grads:
        G = _no_grads
    B, nh = cx.B, L.nh
    H3, W3 = cx.dims[4:]
    ps = bool(cx.per_sample)
    if (fused and ps and not want_param_grads and L.bn3.training and L.bn4.training
            and all(bna.training and bnb.training for _, bna, _, bnb in L.res)
            and ops.latent_tail_supported(nh, L.nrh, H3, W3, len(L.res))):
        return ops.latent_tail_backward(
            g_z.contiguous(), cx.a3, cx.coef3, cx.a4, cx.saved4, _w(L.bn4.weight), _w(L.enc10.weight),
            [(s.ra, s.rb, s.h_in, s.coefa, s.saveda, s.savedb, _w(bna.weight), _w(bnb.weight), _w(ca.weight), _w(cb.weight))
             for s, (ca, bna, cb, bnb) in zip(cx.res, L.res)])
    g_h, stats = residual_backward(L.res, cx.res, g_z.contiguous(), G, cx.a4, pending=pending, zero_fed_biases=zero_fed_biases,
                                   want_param_grads=want_param_grads, per_sample=ps)
    da4 = _bn_backward(stats, H3 * W3 * (1 if ps else B), L.bn4, cx.saved4, g_h, cx.a4, G, G(L.enc10.bias), zero_fed_biases,
                       nbatch=B if ps else 0)
    if FUSED_BACKWARD and not ps and want_param_grads and cx.coef3.dim() == 2 and ops.conv3x3_bwd_fused_supported(nh, nh, H3, W3):
        # enc.10: data and weight gradient from ONE staging of the patch -- csrc/conv3x3_bwd.hip
        return ops.conv3x3_bwd_fused(da4, cx.a3, cx.coef3, _w(L.enc10.weight), G(L.enc10.weight), B, nh, q=cx.a3, pending=pending)
    return _conv_backward_pair(da4, cx.a3, cx.coef3, L.enc10.weight, G(L.enc10.weight), B, nh, nh, H3, W3, 3, pending,
                               like=g_h, stat_q=cx.a3, per_sample=ps)


def encoder_backward(L, cx, g_z, G, zero_fed_biases=True, pending_extra=(), want_dx=False, want_param_grads=True):
    """Accumulates nothing: every parameter gradient G(p) is overwritten.  want_dx: also returns the gradient w.r.t. the input
    patches (the reference's training never asks for it; autograd there would answer) -- the data gradient of the composite
    enc.0 o enc.1 convolution, a transposed convolution with the composite weights' image channels.
    zero_fed_biases=False skips writing the (identically zero) gradients of the conv biases that feed a
    BatchNorm -- for callers whose gradient buffer is zero there already (FusedTrainer).
    A context made with per_sample=True goes backward per patch at any B (the reference's batch-of-one calls, batched): patch
    b's BatchNorm backward takes patch b's own (sum dy, sum dy * a), mean, invstd and count H * W, so g_z[b] -> dx[b] is what a
    batch of that one patch gives; the parameter gradients are the sums over the patches.  Every operand then carries
    per-sample coefficients and every data-gradient launch writes its slabs per patch; the fused backward kernels (one
    coefficient set in registers, one slab per persistent workgroup) are not reached.
    want_param_grads=False: the data gradient only -- G is not called; no weight-gradient launch, no e1_chain, no slab
    reduction, no dgamma / dbeta."""
    pending = list(pending_extra)                    # (slabs, dst) pairs that ride along in the one slab reduction
    if not want_param_grads:
        G = _no_grads
    B, x = cx.B, cx.x
    ps = bool(cx.per_sample)
    nb = B if ps else 0
    fused = FUSED_BACKWARD and not ps and want_param_grads
    NIN, nh, c1 = L.nin, L.nh, L.nh // 2
    H1, W1, H2, W2, H3, W3 = cx.dims
    dy3, st = latent_stage_backward(L, cx, g_z, G, pending, zero_fed_biases, want_param_grads)

    da3 = _bn_backward(st, H3 * W3 * (1 if ps else B), L.bn3, cx.saved3, dy3, cx.a3, G, G(L.enc7.bias), zero_fed_biases, nbatch=nb)
    if fused and cx.coef2.dim() == 2 and ops.conv4x4s2_bwd_fused_supported(nh, nh, H3, W3):
        # enc.7: data and weight gradient from ONE staging of the patch -- csrc/conv4x4s2_patch.hip
        dy2, st = ops.conv4x4s2_bwd_fused(da3, cx.a2, cx.coef2, _w(L.enc7.weight), G(L.enc7.weight), B, pending=pending)
    else:
        dy2, st = _conv_backward_pair(da3, cx.a2, cx.coef2, L.enc7.weight, G(L.enc7.weight), B, nh, nh, H3, W3, 4, pending,
                                      like=dy3, stat_q=cx.a2, per_sample=ps)

    da2 = _bn_backward(st, H2 * W2 * (1 if ps else B), L.bn2, cx.saved2, dy2, cx.a2, G, G(L.enc4.bias), zero_fed_biases, nbatch=nb)
    if fused and cx.coef1.dim() == 2 and ops.conv_bwd_s2_fused_supported(nh, c1, H2, W2):
        # enc.4: data gradient + weight gradient from ONE staging of (dy2, a2, a1) -- csrc/conv_mfma.hip, kernel D
        dy1, st = ops.conv_bwd_s2_fused(da2, Op(cx.a1, DM_LOAD_AFFINE_RELU, cx.coef1), _view_swapped(L.enc4.weight),
                                        G(L.enc4.weight), B, nh, c1, H2, W2, mask=Op(cx.a1, DM_LOAD_AFFINE, cx.coef1),
                                        stat_q=cx.a1, pending=pending)
    else:
        dy1, st = _conv_backward_pair(da2, cx.a1, cx.coef1, L.enc4.weight, G(L.enc4.weight), B, nh, c1, H2, W2, 4, pending,
                                      like=dy3, stat_q=cx.a1, per_sample=ps)

    da1 = _bn_backward(st, H1 * W1 * (1 if ps else B), L.bn1, cx.saved1, dy1, cx.a1, G, nbatch=nb)
    if want_param_grads:
        dweff = torch.empty((c1, NIN + 1, 4, 4), device=x.device, dtype=torch.float32)
        ops.wgrad(da1, Op(x, ones=True), dweff, B, c1, NIN + 1, H1, W1, 4, pending=pending)
        ops.reduce_slabs_multi(pending)                  # all encoder weight gradients in one launch
        ops.e1_chain(dweff, _w(L.enc0.weight), _w(L.enc0.bias), _w(L.enc1.weight), G(L.enc0.weight), G(L.enc0.bias), G(L.enc1.weight))
        _fed_bias(G(L.enc1.bias), L.bn1, da1.coef, G, zero_fed_biases)
    if want_dx:
        # a1 = conv(x, Weff[:, :NIN]) + border bias: dx = ConvTranspose(da1, Weff[:, :NIN]) (phase-decomposed kernel family;
        # the ones channel of the composite carries no gradient to x)
        weff, _ = e1_operands(L)
        dx, _ = ops.conv3x3(da1, _view_swapped(weff), B, c1, 4 * NIN, H1, W1, taps=9, pixel_shuffle=True)
        return dx
    return None


# ------------------------------------------------------------------------------------ VQ
def _vq_state(codebook, shape, slabs, ws, commitment_cost):
    """What ops.vq_loss_finalize needs to produce the quantiser's scalars at the end of the step."""
    B, D, H, W = shape
    return SimpleNamespace(slabs=slabs, ws=ws, K=codebook.shape[0], D=D, positions=B * H * W, cc=commitment_cost)


def vq_forward(codebook, z, commitment_cost, want_out=True, defer_scalars=False, want_scalars=True, ema=False):
    """ema: the scalar launch reports the loss of the EMA codebook mode, cc * mse (the quantisation itself is the same).
    defer_scalars (training pass): no scalar launches here; the third return value is the state
    ops.vq_loss_finalize needs to produce them together with the reconstruction loss at the end of the step.
    want_scalars=False (inference latents, patch_VAE.py:445-452 discards loss and perplexity): no counter reduction and no
    scalar launch at all; the third return value is None."""
    B, D, H, W = z.shape
    if not want_scalars:
        idx, out, _, _ = ops.vq_forward(z, _w(codebook), want_out=want_out, want_hist=False)
        return out, idx, None
    if defer_scalars:
        idx, out, slabs, ws = ops.vq_forward(z, _w(codebook), want_out=want_out, want_hist=False)
        return out, idx, _vq_state(codebook, z.shape, slabs, ws, commitment_cost)
    idx, out, slabs, hist = ops.vq_forward(z, _w(codebook), want_out=want_out)
    scalars = ops.vq_finalize(slabs, hist, B * H * W, D, commitment_cost, ema=ema)     # (loss, perplexity, mse)
    return out, idx, scalars


def vq_forward_joined(codebook, pending_join, commitment_cost):
    """encoder_forward(..., defer_last_join=K) left the last residual join to the quantiser: one launch forms z, quantises
    it and writes both.  Returns (z, out, idx, state for ops.vq_loss_finalize) -- vq_forward(defer_scalars=True)'s contract
    plus the latents."""
    rb, h_in, coef = pending_join
    idx, out, slabs, ws, z = ops.vq_forward_join(rb, h_in, coef, _w(codebook))
    return z, out, idx, _vq_state(codebook, rb.shape, slabs, ws, commitment_cost)


# -------------------------------------------------------------------------------- decoder
def decoder_forward(L, zq, x=None, mask=None, defer_tail=False):
    """defer_tail (training pass only): when the fused tail is available, leave dec.4/dec.6 and the reconstruction
    loss to decoder_backward, which then runs them together with their backward in one kernel
    (ops.dec_tail_train); `decoded` is not produced and cx.loss_slabs is filled by decoder_backward."""
    B, nh, H3, W3 = zq.shape
    c1, c2 = nh // 2, nh // 4
    d0, d2 = _dec_upsample(L, zq)
    var = _dec_var(L, zq)
    fused = ops.dec_tail_supported(c2, L.dec6.weight.shape[0], 4 * H3, 4 * W3)
    if fused and defer_tail and x is not None:
        cx = SimpleNamespace(zq=zq, d0=d0, d2=d2, d4=None, dec=None, x=x, mask=mask, loss_slabs=None, deferred=True)
        return None, cx
    if fused:
        # dec.4 + ReLU + dec.6 (+ loss) in one kernel; the 4 x 128 x 128 tensor d4 is never stored
        d4 = None
        dec, slabs = ops.dec_tail_forward(d2, _w(L.dec4.weight), _w(L.dec4.bias), _w(L.dec6.weight), _w(L.dec6.bias), x, mask, var)
    else:
        d4 = _dec4_forward(L, d2)
        if ops.head_supported(c2, L.dec6.weight.shape[0]):
            dec, slabs = ops.head_forward(d4, _w(L.dec6.weight), _w(L.dec6.bias), x, mask, var)
        else:
            # widths without a fused head: dec.6 as a plain 1x1 convolution, the loss as its own pass
            nin = L.dec6.weight.shape[0]
            dec, _ = ops.conv3x3(Op(d4), _view(L.dec6.weight), B, c2, nin, 8 * H3, 8 * W3, taps=1, bias=_w(L.dec6.bias))
            slabs = ops.recon_loss(dec, x, mask, var) if x is not None else None
    cx = SimpleNamespace(zq=zq, d0=d0, d2=d2, d4=d4, dec=dec, x=x, mask=mask, loss_slabs=slabs, deferred=False)
    return dec, cx


def _dec_upsample(L, zq):
    """dec.0 + ReLU and dec.2 + ReLU: zq (B,nh,H3,W3) -> d0 (B,nh/2,2H3,2W3), d2 (B,nh/4,4H3,4W3)."""
    B, nh, H3, W3 = zq.shape
    c1, c2 = nh // 2, nh // 4
    d0, _ = ops.conv3x3(Op(zq), _view_swapped(L.dec0.weight), B, nh, 4 * c1, H3, W3, taps=9, pixel_shuffle=True,
                        bias=_w(L.dec0.bias), relu=True)
    d2, _ = ops.conv3x3(Op(d0), _view_swapped(L.dec2.weight), B, c1, 4 * c2, 2 * H3, 2 * W3, taps=9, pixel_shuffle=True,
                        bias=_w(L.dec2.bias), relu=True)
    return d0, d2


def _var(channel_var, nin, device):
    # (model.dec called on its own has no loss and hence no channel variances)
    return _w(channel_var).reshape(-1) if channel_var is not None else torch.ones(nin, device=device)


def _dec_var(L, zq):
    return _var(L.channel_var, L.dec6.weight.shape[0], zq.device)


def decoder_score(L, zq, x, mask=None, want_decoded=False):
    """The decoder for per-patch scores: -> (decoded or None, patch_sums (B, NIN) float64 of (dec*m - x*m)^2 / var per patch
    and channel).  The decoder has no BatchNorm, so every patch is the reference's batch-of-one call as it stands; what
    differs from decoder_forward is the reduction.  Where the fused tail is built (ops.dec_tail_supported) its scoring form
    runs and `decoded` is only written when asked for; other widths run the existing forward kernels and sum the stored
    `decoded` per patch."""
    B, nh, H3, W3 = zq.shape
    nin = L.dec6.weight.shape[0]
    if not ops.dec_tail_supported(nh // 4, nin, 4 * H3, 4 * W3):
        dec, _ = decoder_forward(L, zq)
        return dec, ops.recon_loss_per_sample(dec, x, mask, _dec_var(L, zq))
    _, d2 = _dec_upsample(L, zq)
    return ops.dec_tail_score(d2, _w(L.dec4.weight), _w(L.dec4.bias), _w(L.dec6.weight), _w(L.dec6.bias), x, mask,
                              _dec_var(L, zq), want_decoded=want_decoded)


def _dec4_forward(L, d2):
    B, c2, H, W = d2.shape
    d4, _ = ops.conv3x3(Op(d2), _view_swapped(L.dec4.weight), B, c2, 4 * c2, H, W, taps=9, pixel_shuffle=True, bias=_w(L.dec4.bias),
                        relu=True)
    return d4


def _pending(pending):
    """-> (the caller's list of (slabs, dst) pairs for the ONE slab reduction of its whole backward pass, a no-op), or for None
    (a list of our own, its reduction launch): what to append to and what to call after the last append."""
    if pending is not None:
        return pending, lambda: None
    own = []
    return own, lambda: ops.reduce_slabs_multi(own)


def _loss_gradient(dec, x, mask, var, gscale, gdec_ext, want_sums=True):
    """The gradient w.r.t. decoded -- of the reconstruction loss (gscale; None: no loss term) plus the upstream one (gdec_ext;
    None: none) -- and the slabs of its channel sums (the last layer's bias gradient; want_sums=False: not reduced)."""
    if gscale is None:
        g, part = gdec_ext.contiguous(), None
    else:
        g, part = ops.recon_loss_backward(dec, x, mask, var, gscale)
        if gdec_ext is not None:
            g, part = g + gdec_ext, None
    return g, part if (part is not None or not want_sums) else ops.channel_stats(g)


def _head_backward_unfused(L, cx, d4, var, gscale, gdec_ext, G, pending):
    """dec.6 backward for widths the fused head is not built for: loss gradient, bias sums, the 1x1 weight gradient
    and the input gradient (masked by dec.4's ReLU, its channel sums = dec.4's bias gradient) as separate launches."""
    B, c2, H, W = d4.shape
    NIN = L.dec6.weight.shape[0]
    g, sums = _loss_gradient(cx.dec, cx.x, cx.mask, var, gscale, gdec_ext)
    ops.sum_slabs(sums, G(L.dec6.bias))
    ops.wgrad(Op(g), Op(d4), G(L.dec6.weight), B, NIN, c2, H, W, 1, pending=pending)
    g4, st = ops.conv3x3(Op(g), _view_swapped(L.dec6.weight), B, NIN, c2, H, W, taps=1, want_stats=True, mask=Op(d4))
    ops.sum_slabs(st, G(L.dec4.bias))
    return g4


def decoder_backward(L, cx, gscale, gdec_ext, G, want_gz=True, pending=None):
    """gscale: 1-element device tensor = d(total)/d(recon_loss) (None: no loss term);
    gdec_ext: upstream gradient w.r.t. decoded (None: none).
    pending: the caller's list of (slabs, dst) pairs for ONE slab reduction of the whole backward pass -- the decoder's pairs
    are appended and NOT reduced here (FusedTrainer: they ride in the encoder's launch); None: reduced here."""
    zq = cx.zq
    B, nh, H3, W3 = zq.shape
    c1, c2 = nh // 2, nh // 4
    NIN = L.dec6.weight.shape[0]
    var = _dec_var(L, zq)
    pending, reduce = _pending(pending)
    if cx.deferred:
        if gdec_ext is not None or gscale is None:
            raise ValueError("decoder_backward: a deferred tail takes the reconstruction-loss gradient only")
        g2, part, wsl, cx.loss_slabs = ops.dec_tail_train(cx.d2, _w(L.dec4.weight), _w(L.dec4.bias), _w(L.dec6.weight),
                                                          _w(L.dec6.bias), cx.x, cx.mask, var, gscale)
        ops.pend_stats(pending, part, [G(L.dec6.weight), G(L.dec6.bias), G(L.dec4.bias), G(L.dec2.bias)])
        pending.append((wsl, G(L.dec4.weight)))
    elif cx.d4 is None and gdec_ext is None and gscale is not None:
        # fused tail: recompute d4 from d2, g4 lives only in LDS
        g2, part, wsl = ops.dec_tail_backward(cx.d2, _w(L.dec4.weight), _w(L.dec4.bias), _w(L.dec6.weight), cx.dec, cx.x,
                                              cx.mask, var, gscale)
        ops.pend_stats(pending, part, [G(L.dec6.weight), G(L.dec6.bias), G(L.dec4.bias), G(L.dec2.bias)])
        pending.append((wsl, G(L.dec4.weight)))
    else:
        d4 = cx.d4 if cx.d4 is not None else _dec4_forward(L, cx.d2)
        if ops.head_supported(c2, NIN):
            g4, part = ops.head_backward(cx.dec, cx.x, cx.mask, var, d4, _w(L.dec6.weight), gscale, gdec_ext)
            ops.pend_stats(pending, part, [G(L.dec6.weight), G(L.dec6.bias), G(L.dec4.bias)])
        else:
            g4 = _head_backward_unfused(L, cx, d4, var, gscale, gdec_ext, G, pending)
        ops.wgrad(Op(cx.d2), Op(g4), G(L.dec4.weight), B, c2, c2, 4 * H3, 4 * W3, 4, pending=pending)
        g2, st = ops.conv4x4s2(Op(g4), _view(L.dec4.weight), B, c2, c2, 8 * H3, 8 * W3, want_stats=True, mask=Op(cx.d2))
        ops.pend_stats(pending, st, [G(L.dec2.bias)])
    g2 = g2.contiguous()
    if FUSED_BACKWARD and ops.convT_bwd_fused_supported(c1, c2, 2 * H3, 2 * W3):
        # dec.2: input and weight gradient from ONE staging of (d0, g2) -- csrc/convT_bwd.hip
        g0, st = ops.convT_bwd_fused(cx.d0, g2, _w(L.dec2.weight), G(L.dec2.weight), mask_relu=True, want_stats=True,
                                     pending=pending)
    else:
        ops.wgrad(Op(cx.d0), Op(g2), G(L.dec2.weight), B, c1, c2, 2 * H3, 2 * W3, 4, pending=pending)
        g0, st = ops.conv4x4s2(Op(g2), _view(L.dec2.weight), B, c2, c1, 4 * H3, 4 * W3, want_stats=True, mask=Op(cx.d0))
    ops.pend_stats(pending, st, [G(L.dec0.bias)])         # bias gradients ride in the one slab reduction below
    g_zq = None
    if want_gz and FUSED_BACKWARD and ops.convT_bwd_fused_supported(nh, c1, H3, W3):
        g_zq, _ = ops.convT_bwd_fused(zq.contiguous(), g0, _w(L.dec0.weight), G(L.dec0.weight), pending=pending)     # dec.0 likewise
    else:
        ops.wgrad(Op(zq), Op(g0), G(L.dec0.weight), B, nh, c1, H3, W3, 4, pending=pending)
    reduce()                                         # all decoder weight gradients in one launch
    if not want_gz:
        return None
    if g_zq is None:
        g_zq, _ = ops.conv4x4s2(Op(g0), _view(L.dec0.weight), B, c1, nh, 2 * H3, 2 * W3)
    return g_zq


# ======================================================================== VQ_VAE_z32 (vae.py:348-474)
# 32x32 latent: enc = Conv(4,2,1) BN ReLU Conv(4,2,1) BN ResidualBlock; dec = ResidualBlock ConvT BN ReLU ConvT.
# L: a Z32Layers.  The residual stacks are the ResidualBlock module itself (residual_forward/backward); the four z32_stem_* /
# z32_tail_* functions are the two conv "stems" around them (the autograd path runs them as nodes of their own, beside the
# ResidualBlock's), the four z32_encoder_* / z32_decoder_* functions the whole stages, with the calling conventions of
# encoder_forward .. decoder_backward.  Same conventions as above: raw conv outputs + statistics slabs, BatchNorm applied by
# the consumer's operand load, BatchNorm backward as an AFFINE2 operand.
def z32_stem_forward(L, x, per_sample=False):
    """x (B,NIN,H,W) -> h = BN(conv1(relu(BN(conv0(x))))) (B,nh,H/4,W/4), materialised for the residual stack.
    per_sample=True: every BatchNorm uses that sample's own statistics (process_VAE's batch-of-one calls, batched)."""
    conv0, bn0, conv1, bn1 = L.conv0, L.bn0, L.conv1, L.bn1
    B, NIN, H, W = x.shape
    ps = per_sample
    c1, nh = conv0.weight.shape[0], conv1.weight.shape[0]
    H1, W1, H2, W2 = H // 2, W // 2, H // 4, W // 4
    a1, st = ops.conv4x4s2(Op(x), _view(conv0.weight), B, NIN, c1, H, W, want_stats=True, bias=_w(conv0.bias), per_tile=ps)
    coef1, saved1 = _bn_coef(st, bn0, H1 * W1 * (1 if ps else B), ps, B)
    a2, st = ops.conv4x4s2(Op(a1, DM_LOAD_AFFINE_RELU, coef1, per_sample=ps), _view(conv1.weight), B, c1, nh, H1, W1,
                           want_stats=True, bias=_w(conv1.bias), per_tile=ps)
    coef2, saved2 = _bn_coef(st, bn1, H2 * W2 * (1 if ps else B), ps, B)
    h = ops.apply(Op(a2, DM_LOAD_AFFINE, coef2, per_sample=ps), B, nh, H2, W2)
    cx = SimpleNamespace(x=x, a1=a1, a2=a2, coef1=coef1, coef2=coef2, saved1=saved1, saved2=saved2, per_sample=ps,
                         dims=(B, NIN, c1, nh, H1, W1, H2, W2))
    return h, cx


def z32_stem_backward(L, cx, g_h, G, stats=None, pending=None, zero_fed_biases=True, want_dx=False,
                      want_param_grads=True):
    """stats: the (sum g, sum g*a2) slabs when the caller's last kernel already produced them (residual_backward with
    q_below = cx.a2); pending: the caller's list for ONE slab reduction of the whole backward pass (None: reduced here);
    zero_fed_biases=False: the gradient buffer is zero already (FusedTrainer) -- the identically zero gradients of the
    conv biases that feed a BatchNorm are not written.
    A context made with per_sample=True goes backward per patch and want_param_grads=False returns the data gradient only,
    both as in encoder_backward (`stats` then is grouped by patch: residual_backward's per-sample slabs)."""
    conv0, bn0, conv1, bn1 = L.conv0, L.bn0, L.conv1, L.bn1
    B, NIN, c1, nh, H1, W1, H2, W2 = cx.dims
    ps = bool(getattr(cx, "per_sample", False))
    nb = B if ps else 0
    if not want_param_grads:
        G = _no_grads
    g_h = g_h.contiguous()
    pending, reduce = _pending(pending)
    if stats is None:
        stats = (ops.channel_stats_per_sample if ps else ops.channel_stats)(g_h, cx.a2)
    da2 = _bn_backward(stats, H2 * W2 * (1 if ps else B), bn1, cx.saved2, g_h, cx.a2, G, nbatch=nb)
    dy1, st = _conv_backward_pair(da2, cx.a1, cx.coef1, conv1.weight, G(conv1.weight), B, nh, c1, H2, W2, 4, pending, like=g_h,
                                  stat_q=cx.a1, between=lambda: _fed_bias(G(conv1.bias), bn1, da2.coef, G, zero_fed_biases),
                                  per_sample=ps)
    da1 = _bn_backward(st, H1 * W1 * (1 if ps else B), bn0, cx.saved1, dy1, cx.a1, G, nbatch=nb)
    if want_param_grads:
        ops.wgrad(da1, Op(cx.x), G(conv0.weight), B, c1, NIN, H1, W1, 4, pending=pending)
        _fed_bias(G(conv0.bias), bn0, da1.coef, G, zero_fed_biases)
        reduce()
    if want_dx:          # the gradient w.r.t. the input patches: conv0's data gradient (see encoder_backward)
        dx, _ = ops.conv3x3(da1, _view_swapped(conv0.weight), B, c1, 4 * NIN, H1, W1, taps=9, pixel_shuffle=True)
        return dx
    return None


def z32_tail_forward(L, r, x, mask, per_sample=False, defer=None):
    """r (B,nh,H2,W2) -> decoded (B,NIN,4*H2,4*W2) (+ loss slabs when x is given).
    per_sample=True: the BatchNorm uses every sample's own statistics (the reference's batch-of-one call, batched), exactly
    as z32_stem_forward does; defer: the caller's list of postponed running-statistics updates (ops.bn_running_replay)."""
    up0, bn, up1 = L.up0, L.bn_up, L.up1
    B, nh, H2, W2 = r.shape
    ps = per_sample
    c1, NIN = up0.weight.shape[1], up1.weight.shape[1]
    d1, st = ops.conv3x3(Op(r), _view_swapped(up0.weight), B, nh, 4 * c1, H2, W2, taps=9, pixel_shuffle=True,
                         want_stats=True, bias=_w(up0.bias), per_tile=ps)
    if ps:
        _need_per_sample_slabs(st, B, "z32_tail_forward: dec.1 (ConvTranspose2d %d -> %d at %d x %d)" % (nh, c1, H2, W2))
    coefd, savedd = _bn_coef(st, bn, 4 * H2 * W2 * (1 if ps else B), ps, B, defer)
    dec, _ = ops.conv3x3(Op(d1, DM_LOAD_AFFINE_RELU, coefd, per_sample=ps), _view_swapped(up1.weight), B, c1, 4 * NIN,
                         2 * H2, 2 * W2, taps=9, pixel_shuffle=True, bias=_w(up1.bias))
    var = _var(L.channel_var, NIN, r.device)
    slabs = ops.recon_loss(dec, x, mask, var) if x is not None else None
    cx = SimpleNamespace(r=r, d1=d1, coefd=coefd, savedd=savedd, dec=dec, x=x, mask=mask, var=var, loss_slabs=slabs,
                         per_sample=ps, dims=(B, nh, c1, NIN, H2, W2))
    return dec, cx


def z32_tail_backward(L, cx, gscale, gdec_ext, G, want_gr=True, pending=None, zero_fed_biases=True,
                      want_param_grads=True):
    """gscale: 1-element device tensor d(total)/d(recon_loss) or None; gdec_ext: upstream gradient w.r.t. decoded or None.
    pending / zero_fed_biases / a per_sample context / want_param_grads: as in z32_stem_backward."""
    up0, bn, up1 = L.up0, L.bn_up, L.up1
    B, nh, c1, NIN, H2, W2 = cx.dims
    ps = bool(getattr(cx, "per_sample", False))
    nb = B if ps else 0
    if not want_param_grads:
        G = _no_grads
    pending, reduce = _pending(pending)
    g, sums = _loss_gradient(cx.dec, cx.x, cx.mask, cx.var, gscale, gdec_ext, want_sums=want_param_grads)
    d1_in, d1_mask = (Op(cx.d1, DM_LOAD_AFFINE_RELU, cx.coefd, per_sample=ps), Op(cx.d1, DM_LOAD_AFFINE, cx.coefd, per_sample=ps))
    if want_param_grads:
        ops.pend_stats(pending, sums, [G(up1.bias)])         # the last layer's bias gradient rides in the slab reduction
        ops.wgrad(d1_in, Op(g), G(up1.weight), B, c1, NIN, 2 * H2, 2 * W2, 4, pending=pending)
    dy, st = ops.conv4x4s2(Op(g), _view(up1.weight), B, NIN, c1, 4 * H2, 4 * W2, want_stats=True, mask=d1_mask, stat_q=cx.d1,
                           **({"per_tile": True} if ps else {}))
    if ps:
        _need_per_sample_slabs(st, B, "z32_tail_backward: dec.4 (ConvTranspose2d %d -> %d at %d x %d)" % (c1, NIN, 2 * H2, 2 * W2))
    # da = BatchNorm backward of dy.  The weight-gradient kernels take that transform on their S operand; as the T operand only
    # where the one-pass kernel prefetches both tensors (the example widths) -- elsewhere da is materialised here
    da = _bn_backward(st, 4 * H2 * W2 * (1 if ps else B), bn, cx.savedd, dy, cx.d1, G, nbatch=nb)
    cdb = da.coef
    if want_param_grads:
        if not ops.wgrad_t_affine2_supported(nh, c1, H2, W2, 4):
            da = Op(ops.apply(da, B, c1, 2 * H2, 2 * W2))
        ops.wgrad(Op(cx.r), da, G(up0.weight), B, nh, c1, H2, W2, 4, pending=pending)
        _fed_bias(G(up0.bias), bn, cdb, G, zero_fed_biases)
    g_r = None
    if want_gr:
        g_r, _ = ops.conv4x4s2(da, _view(up0.weight), B, c1, nh, 2 * H2, 2 * W2)
    if want_param_grads:
        reduce()
    return g_r


def z32_encoder_forward(L, x, per_sample=False):
    """x (B,NIN,H,W) -> (z_before (B,nh,H/4,W/4), cx): the stem, then the residual stack (cx.res: its saved contexts)."""
    h, cx = z32_stem_forward(L, x, per_sample=per_sample)
    z, cx.res = residual_forward(L.enc_res, h, per_sample)
    return z, cx


def z32_encoder_backward(L, cx, g_z, G, zero_fed_biases=True, pending_extra=(), want_dx=False, want_param_grads=True):
    """encoder_backward's contract: every parameter gradient G(p) is overwritten, pending_extra rides along in the ONE slab
    reduction, want_dx returns the gradient w.r.t. the patches, want_param_grads=False is the data gradient alone."""
    pending = list(pending_extra)
    g_h, stats = residual_backward(L.enc_res, cx.res, g_z, G, cx.a2, pending=pending, zero_fed_biases=zero_fed_biases,
                                   want_param_grads=want_param_grads, per_sample=cx.per_sample)
    dx = z32_stem_backward(L, cx, g_h, G, stats=stats, pending=pending, zero_fed_biases=zero_fed_biases, want_dx=want_dx,
                           want_param_grads=want_param_grads)
    if want_param_grads:
        ops.reduce_slabs_multi(pending)
    return dx


def z32_decoder_forward(L, zq, x=None, mask=None, per_sample=False):
    """zq (B,nh,H2,W2) -> (decoded, cx): the residual stack (cx.res: its saved contexts), then the tail (+ loss slabs when x is
    given).  per_sample: the running statistics of all five BatchNorms advance in one launch right behind the tail."""
    defer = [] if per_sample else None
    r, saved = residual_forward(L.dec_res, zq, per_sample, defer)
    dec, cx = z32_tail_forward(L, r, x, mask, per_sample=per_sample, defer=defer)
    cx.res = saved
    if per_sample:
        ops.bn_running_replay(defer)
    return dec, cx


def z32_decoder_backward(L, cx, gscale, gdec_ext, G, want_gz=True, pending=None, zero_fed_biases=True, want_param_grads=True):
    """decoder_backward's contract (gscale / gdec_ext / pending); zero_fed_biases, a per_sample context and want_param_grads as
    in z32_stem_backward.  Returns the gradient w.r.t. zq (the stack's backward forms it either way; want_gz=False: None)."""
    pending, reduce = _pending(pending)
    g_r = z32_tail_backward(L, cx, gscale, gdec_ext, G, pending=pending, zero_fed_biases=zero_fed_biases,
                            want_param_grads=want_param_grads)
    g_zq, _ = residual_backward(L.dec_res, cx.res, g_r, G, None, pending=pending, zero_fed_biases=zero_fed_biases,
                                want_param_grads=want_param_grads, per_sample=cx.per_sample)
    if want_param_grads:
        reduce()
    return g_zq if want_gz else None
