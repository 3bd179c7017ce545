"""Tensor-level wrappers over the C ABI: they take CUDA (ROCm) torch tensors, pass raw
device pointers and the current HIP stream, and allocate outputs with PyTorch.

Nothing here computes on the host and nothing falls back to ATen: a tensor that is not a
contiguous fp32 device tensor is an error.
"""
import collections
import ctypes as C
import functools

import torch

from . import _lib as L
from ._lib import DM_LOAD_AFFINE, DM_LOAD_AFFINE2, DM_LOAD_AFFINE_RELU, DM_LOAD_IDENT, DM_LOAD_RELU  # noqa: F401


def _stream():
    """The stream of the device the call's tensors live on (recorded by _ptr), not of whatever device is current; the
    launch itself runs under a device guard (_lib._guarded)."""
    dev = L.call_device.index
    return torch.cuda.current_stream(dev).cuda_stream


def _op(fn):
    """Every tensor-level wrapper below is one "call": the device recorded by _ptr is cleared when it starts and when it
    ends (also on an exception), so a half-assembled launch can never leak its device into the next call, and every pointer
    marshalled for the launch -- before or after host-only queries -- is checked against the same device."""
    @functools.wraps(fn)
    def call(*args, **kw):
        L.call_device.index = None
        try:
            return fn(*args, **kw)
        finally:
            L.call_device.index = None
    return call


def _ptr(t, dtype=torch.float32):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("dynamorph_amd: tensor is not on the GPU (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise ValueError(f"dynamorph_amd: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("dynamorph_amd: tensor must be contiguous")
    _note_device(t.device.index)
    return t.data_ptr()


def _note_device(dev):
    """First operand of a call: its device becomes the call's; every later one must live there too."""
    if L.call_device.index is None:
        L.call_device.index = dev
    elif L.call_device.index != dev:
        raise ValueError(f"dynamorph_amd: operands of one call live on different devices "
                         f"(cuda:{L.call_device.index} and cuda:{dev})")


class Op:
    """A tensor together with its on-load transform (dm_operand)."""
    __slots__ = ("p0", "p1", "coef", "mode", "ones", "bstride", "_keep")

    def __init__(self, p0, mode=DM_LOAD_IDENT, coef=None, p1=None, ones=False, per_sample=False):
        self.p0, self.p1, self.coef, self.mode, self.ones = p0, p1, coef, mode, ones
        # per-sample coefficients are (B, C, 4); eval-mode BatchNorm hands the shared (C, 4) table to the per-sample path too
        self.bstride = coef.shape[-2] * 4 if (per_sample and coef is not None and coef.dim() == 3) else 0

    def struct(self):
        return L.Operand(_ptr(self.p0), _ptr(self.p1), _ptr(self.coef), self.bstride, self.mode, 1 if self.ones else 0)


def _null_operand():
    return L.Operand(None, None, None, 0, DM_LOAD_IDENT, 0)


class WView:
    """dm_weight_view plus a reference to the tensor it points into (a bare struct would dangle as soon
    as a temporary such as `w.to(device)` is collected and the caching allocator reuses its block)."""
    __slots__ = ("struct", "_keep", "_scratch")

    def __init__(self, w, sn, sc, sky, skx, off=0):
        if not (w.is_cuda and w.dtype == torch.float32):
            raise ValueError("dynamorph_amd: weights must be fp32 device tensors (the HIP path has no CPU fallback)")
        if not w.is_contiguous():
            # the strides below address a contiguous (n, c, ky, kx) tensor: a channels_last / transposed / sliced parameter
            # would be read with the wrong layout
            raise ValueError("dynamorph_amd: weights must be contiguous")
        self._keep = w
        self._scratch = None
        self.struct = L.WeightView(w.data_ptr(), off, sn, sc, sky, skx, None, 0)

    def ref(self):
        """The struct for a launch; records / checks the weights' device like every other operand of the call."""
        _note_device(self._keep.device.index)
        return C.byref(self.struct)

    def with_scratch(self, nfloats):
        """Attach `nfloats` of device scratch (dm_weight_view.scratch; what dm_conv*_scratch_floats asked for)."""
        if nfloats > 0 and (self._scratch is None or self._scratch.numel() < nfloats):
            self._scratch = torch.empty(nfloats, device=self._keep.device, dtype=torch.float32)
            self.struct.scratch = self._scratch.data_ptr()
            self.struct.scratch_floats = nfloats
        return self


def weight_view(w, sn, sc, sky, skx, off=0):
    return WView(w, sn, sc, sky, skx, off)


def epilogue(bias=None, relu=False, mask=None, resid=None, stat_q=None, stats=None, per_tile=False, bias_border=None):
    m = mask.struct() if mask is not None else _null_operand()
    return L.Epilogue(_ptr(bias), _ptr(bias_border), 1 if relu else 0, 1 if per_tile else 0, m, _ptr(resid),
                      _ptr(stat_q), _ptr(stats, torch.float64))


def _new(shape, like, dtype=torch.float32):
    return torch.empty(shape, device=like.device, dtype=dtype)


# ----------------------------------------------------------------------------- VQ
@_op
def vq_forward(z, codebook, want_idx=True, want_out=True, variant=L.DM_VQ_AUTO, want_rechecked=False, want_hist=True):
    """Returns (idx int64 (B,H,W), out (B,D,H,W), sse_slabs, hist).
    want_hist=False: no counter reduction is launched; the fourth return value is then the WORKSPACE holding the counter
    replicas, for vq_loss_finalize.
    variant: L.DM_VQ_AUTO (default) / DM_VQ_EXACT / DM_VQ_MFMA -- same results, different kernels (include/dynamorph_hip.h).
    want_rechecked: a fifth return value, the 1-element int32 device tensor counting the positions the MFMA kernel
    re-evaluated exactly (0 after the exact kernel)."""
    lib = L.load()
    if want_rechecked and not want_hist:
        raise ValueError("vq_forward: the re-check count is summed by the counter reduction (want_hist=True)")
    B, D, H, W = z.shape
    K = codebook.shape[0]
    nb = lib.dm_vq_num_blocks(B * H * W)
    idx = _new((B, H, W), z, torch.int64) if want_idx else None
    out = torch.empty_like(z) if want_out else None
    slabs = _new((nb,), z, torch.float64)
    hist = _new((K,), z, torch.int32) if want_hist else None         # cleared by dm_vq_forward itself
    wsb = lib.dm_vq_workspace_bytes(K, D)
    ws = _new((wsb // 4,), z)
    L.check(lib.dm_vq_forward_variant(_ptr(z), _ptr(codebook), _ptr(idx, torch.int64), _ptr(out),
                                      _ptr(slabs, torch.float64), _ptr(hist, torch.int32), B, D, K, H, W, _ptr(ws), wsb,
                                      variant, _stream()), "dm_vq_forward")
    if want_rechecked:
        return idx, out, slabs, hist, ws[:1].view(torch.int32)
    return idx, out, slabs, (hist if want_hist else ws)


def vq_forward_join_supported(D, K, H, W):
    return bool(L.load().dm_vq_forward_join_supported(D, K, H, W))


@_op
def vq_forward_join(rb, h_in, coef, codebook, want_idx=True, want_out=True):
    """The last residual join and the VectorQuantizer in one launch (include/dynamorph_hip.h, dm_vq_forward_join):
    z = fma(coef[:, 0], rb, coef[:, 2]) + h_in, quantised like vq_forward(z, ..., want_hist=False).
    Returns (idx, out, sse_slabs, workspace, z)."""
    lib = L.load()
    B, D, H, W = rb.shape
    K = codebook.shape[0]
    if tuple(h_in.shape) != tuple(rb.shape) or tuple(coef.shape) != (D, 4):
        raise ValueError("dm_vq_forward_join: rb / h_in (B, D, H, W) and a shared (D, 4) coefficient table")
    nb = lib.dm_vq_num_blocks(B * H * W)
    z = torch.empty_like(rb)
    idx = _new((B, H, W), rb, torch.int64) if want_idx else None
    out = torch.empty_like(rb) if want_out else None
    slabs = _new((nb,), rb, torch.float64)
    wsb = lib.dm_vq_workspace_bytes(K, D)
    ws = _new((wsb // 4,), rb)
    L.check(lib.dm_vq_forward_join(_ptr(rb), _ptr(h_in), _ptr(coef), _ptr(z), _ptr(codebook), _ptr(idx, torch.int64), _ptr(out),
                                   _ptr(slabs, torch.float64), None, B, D, K, H, W, _ptr(ws), wsb, _stream()),
            "dm_vq_forward_join")
    return idx, out, slabs, ws, z


@_op
def vq_forward_repeat(z, codebook, repeats, variant=L.DM_VQ_AUTO, bufs=None, want_hist=True):
    """Measurement helper (include/dynamorph_hip.h, dm_vq_forward_repeat): one preparation, `repeats` launches of the
    distance / argmin kernel, one counter reduction, on preallocated buffers `bufs` (from a first call) so that nothing is
    allocated inside a timed region.  want_hist=False: hist = NULL, i.e. no counter reduction -- how the training step and
    the inference path call dm_vq_forward (their counters are read from the workspace by the step's one scalar launch, or
    not at all).  Returns bufs."""
    lib = L.load()
    B, D, H, W = z.shape
    K = codebook.shape[0]
    if bufs is None:
        wsb = lib.dm_vq_workspace_bytes(K, D)
        bufs = (_new((B, H, W), z, torch.int64), torch.empty_like(z), _new((lib.dm_vq_num_blocks(B * H * W),), z, torch.float64),
                _new((K,), z, torch.int32), _new((wsb // 4,), z), wsb)
    idx, out, slabs, hist, ws, wsb = bufs
    L.check(lib.dm_vq_forward_repeat(_ptr(z), _ptr(codebook), _ptr(idx, torch.int64), _ptr(out), _ptr(slabs, torch.float64),
                                     _ptr(hist if want_hist else None, torch.int32), B, D, K, H, W, _ptr(ws), wsb, variant,
                                     repeats, _stream()),
            "dm_vq_forward_repeat")
    return bufs


@_op
def vq_finalize(slabs, hist, positions, D, commitment_cost, ema=False):
    """(loss, perplexity, mse); ema: the loss of the EMA codebook mode, cc * mse (dm_vq_finalize_ema)."""
    lib = L.load()
    scalars = _new((3,), slabs)
    fn, who = (lib.dm_vq_finalize_ema, "dm_vq_finalize_ema") if ema else (lib.dm_vq_finalize, "dm_vq_finalize")
    L.check(fn(_ptr(slabs, torch.float64), slabs.numel(), _ptr(hist, torch.int32), hist.numel(),
               positions, D, commitment_cost, _ptr(scalars), _stream()), who)
    return scalars


@_op
def vq_loss_finalize(sse_slabs, ws, K, D, positions, commitment_cost, loss_slabs, count, weight_recon, weight_commitment,
                     ema=False):
    """(recon, commitment, total, perplexity) in one launch: vq_finalize + loss_finalize on the counter replicas that
    vq_forward(..., want_hist=False) left in its workspace `ws`.  ema: commitment = cc * mse (dm_vq_loss_finalize_ema)."""
    lib = L.load()
    out = _new((4,), sse_slabs)
    if ema:
        L.check(lib.dm_vq_loss_finalize_ema(_ptr(sse_slabs, torch.float64), sse_slabs.numel(), _ptr(ws), K, D, positions,
                                            commitment_cost, _ptr(loss_slabs, torch.float64), loss_slabs.numel(), count,
                                            weight_recon, weight_commitment, None, 0, 0.0, _ptr(out), _stream()),
                "dm_vq_loss_finalize_ema")
        return out
    L.check(lib.dm_vq_loss_finalize(_ptr(sse_slabs, torch.float64), sse_slabs.numel(), _ptr(ws), K, D, positions,
                                    commitment_cost, _ptr(loss_slabs, torch.float64), loss_slabs.numel(), count,
                                    weight_recon, weight_commitment, _ptr(out), _stream()), "dm_vq_loss_finalize")
    return out


@_op
def vq_loss_finalize_tm(sse_slabs, ws, K, D, positions, commitment_cost, loss_slabs, count, weight_recon, weight_commitment,
                        tm_slabs, weight_matching, ema=False):
    """vq_loss_finalize with the pairwise term: (recon, commitment, total + weight_matching * tm, perplexity, tm) in one
    launch from the partial losses time_matching_forward(..., want_slabs=True) left."""
    lib = L.load()
    out = _new((5,), sse_slabs)
    fn = lib.dm_vq_loss_finalize_ema if ema else lib.dm_vq_loss_finalize_tm
    L.check(fn(_ptr(sse_slabs, torch.float64), sse_slabs.numel(), _ptr(ws), K, D, positions,
               commitment_cost, _ptr(loss_slabs, torch.float64), loss_slabs.numel(), count,
               weight_recon, weight_commitment, _ptr(tm_slabs, torch.float64), tm_slabs.shape[0],
               weight_matching, _ptr(out), _stream()), "dm_vq_loss_finalize_ema" if ema else "dm_vq_loss_finalize_tm")
    return out


@_op
def vq_decode(idx, codebook):
    lib = L.load()
    B, H, W = idx.shape
    K, D = codebook.shape
    q = _new((B, D, H, W), codebook)
    L.check(lib.dm_vq_decode(_ptr(idx, torch.int64), _ptr(codebook), _ptr(q), B, D, K, H, W, _stream()), "dm_vq_decode")
    return q


@_op
def vq_backward(z, codebook, idx, g_out, g_loss, commitment_cost, dw=None, want_dz=True):
    """g_loss: 1-element device tensor (or None = 1).  dw given: accumulated into with float atomics (zero it first);
    dw None: a fresh tensor from the slab form (see vq_backward_slabs for when that form is ordered)."""
    lib = L.load()
    B, D, H, W = z.shape
    K = codebook.shape[0]
    if dw is None:
        dz, slabs = vq_backward_slabs(z, codebook, idx, g_out, g_loss, commitment_cost, want_dz=want_dz)
        return dz, reduce_slabs(slabs, torch.empty_like(codebook))
    dz = torch.empty_like(z) if want_dz else None
    L.check(lib.dm_vq_backward(_ptr(z), _ptr(codebook), _ptr(idx, torch.int64), _ptr(g_out), _ptr(g_loss),
                               commitment_cost, _ptr(dz), _ptr(dw), B, D, K, H, W, _stream()), "dm_vq_backward")
    return dz, dw


@_op
def vq_backward_slabs(z, codebook, idx, g_out, g_loss, commitment_cost, want_dz=True):
    """Like vq_backward, but the codebook gradient comes back as per-workgroup slabs (nslabs, K*D) for
    reduce_slabs / reduce_slabs_multi: no global float atomics, nothing to zero.  Codebooks of at most 64 codes with
    embedding_dim 16/32/64 and H*W % 64 == 0 (every reference configuration) accumulate as a one-hot product on the
    matrix cores in a fixed order: bit-reproducible.  Larger codebooks add inside a workgroup with LDS float atomics in
    arrival order, so the low bits of THEIR gradient may differ from run to run."""
    lib = L.load()
    B, D, H, W = z.shape
    K = codebook.shape[0]
    dz = torch.empty_like(z) if want_dz else None
    slabs = _new((lib.dm_vq_backward_num_slabs(B * H * W, K, D), K * D), z)
    L.check(lib.dm_vq_backward_slabs(_ptr(z), _ptr(codebook), _ptr(idx, torch.int64), _ptr(g_out), _ptr(g_loss),
                                     commitment_cost, _ptr(dz), _ptr(slabs), B, D, K, H, W, _stream()),
            "dm_vq_backward_slabs")
    return dz, slabs


@_op
def vq_backward_stats(z, codebook, idx, g_out, g_loss, commitment_cost, want_dz=True):
    """The quantiser's backward in the EMA codebook mode (include/dynamorph_hip.h, dm_vq_backward_stats): dz as
    vq_backward_slabs writes it, and per-workgroup slabs (nslabs, K * (D + 1)) of the update's statistics -- K * D sums of the
    assigned z, then K counts as floats -- for reduce_slabs / reduce_slabs_multi.  The order of the additions is fixed on
    every route.  want_dz=False (and g_out, g_loss None): the statistics alone."""
    lib = L.load()
    B, D, H, W = z.shape
    K = codebook.shape[0]
    if tuple(idx.shape) != (B, H, W) or tuple(codebook.shape) != (K, D):
        raise ValueError("dm_vq_backward_stats: z (B, D, H, W), idx (B, H, W), codebook (K, D)")
    dz = torch.empty_like(z) if want_dz else None
    slabs = _new((lib.dm_vq_backward_num_slabs(B * H * W, K, D), K * (D + 1)), z)
    L.check(lib.dm_vq_backward_stats(_ptr(z), _ptr(codebook), _ptr(idx, torch.int64), _ptr(g_out), _ptr(g_loss),
                                     commitment_cost, _ptr(dz), _ptr(slabs), B, D, K, H, W, _stream()),
            "dm_vq_backward_stats")
    return dz, slabs


@_op
def vq_ema_apply(stats, cluster_size, ema_w, codebook, decay, epsilon):
    """The EMA codebook update in place, one launch (dm_vq_ema_apply): stats = (K * (D + 1),) sums then counts."""
    lib = L.load()
    K, D = codebook.shape
    if stats.numel() != K * (D + 1) or cluster_size.numel() != K or tuple(ema_w.shape) != (K, D):
        raise ValueError("dm_vq_ema_apply: stats (K * (D + 1),), cluster_size (K,), ema_w and codebook (K, D)")
    L.check(lib.dm_vq_ema_apply(_ptr(stats), _ptr(cluster_size), _ptr(ema_w), _ptr(codebook), K, D, float(decay),
                                float(epsilon), _stream()), "dm_vq_ema_apply")


# ---------------------------------------------------------------------- convolutions
@_op
def conv4x4s2(inp, wv, B, CIN, NOUT, H, W, ep=None, out=None, want_stats=False, like=None, **epkw):
    lib = L.load()
    like = like if like is not None else inp.p0
    if out is None:
        out = _new((B, NOUT, H // 2, W // 2), like)
    stats = None
    if want_stats:
        nb = lib.dm_conv4x4s2_num_blocks(B, CIN, NOUT, H, W, 1 if epkw.get("per_tile") else 0)
        if nb <= 0:
            raise ValueError(f"dm_conv4x4s2: shape {(B, CIN, NOUT, H, W)} not tileable")
        stats = _new((nb, NOUT, 2), like, torch.float64)
    e = epilogue(stats=stats, **epkw)
    o = inp.struct()
    fallback = _conv4_fallback(inp.mode, epkw)
    wv.with_scratch(lib.dm_conv4x4s2_scratch_floats(CIN, NOUT, H, W, 1 if fallback else 0))
    L.check(lib.dm_conv4x4s2(C.byref(o), wv.ref(), _ptr(out), C.byref(e), B, CIN, NOUT, H, W, _stream()),
            "dm_conv4x4s2")
    return out, stats


@_op
def conv3x3(inp, wv, B, CIN, NOUT, H, W, taps=9, pixel_shuffle=False, out=None, want_stats=False, like=None, **epkw):
    lib = L.load()
    like = like if like is not None else inp.p0
    co = NOUT // 4 if pixel_shuffle else NOUT
    if out is None:
        out = _new((B, co, 2 * H, 2 * W) if pixel_shuffle else (B, co, H, W), like)
    stats = None
    if want_stats:
        nb = lib.dm_conv3x3_num_blocks(B, CIN, NOUT, H, W, taps, 1 if pixel_shuffle else 0, 1 if epkw.get("per_tile") else 0)
        if nb <= 0:
            raise ValueError(f"dm_conv3x3: shape {(B, CIN, NOUT, H, W)} not tileable")
        stats = _new((nb, co, 2), like, torch.float64)
    e = epilogue(stats=stats, **epkw)
    o = inp.struct()
    wv.with_scratch(lib.dm_conv3x3_scratch_floats(CIN, NOUT, H, W, taps, 1 if pixel_shuffle else 0,
                                                  1 if epkw.get("per_tile") else 0))
    L.check(lib.dm_conv3x3(C.byref(o), wv.ref(), _ptr(out), C.byref(e), B, CIN, NOUT, H, W, taps,
                           1 if pixel_shuffle else 0, _stream()), "dm_conv3x3")
    return out, stats


@_op
def wgrad(S, T, dst, B, CS, CT, Hs, Ws, k, pending=None):
    """dst (CS*CT*k*k floats, any shape) <- sum over batch/positions; deterministic slab reduction.
    pending: a list -> the slabs are left unreduced and (slabs, dst) is appended for reduce_slabs_multi."""
    lib = L.load()
    nb = lib.dm_wgrad_num_blocks(B, CS, CT, Hs, Ws, k)
    if nb <= 0:
        raise ValueError(f"dm_wgrad: shape {(B, CS, CT, Hs, Ws, k)} not tileable")
    slabs = _new((nb, CS * CT * k * k), S.p0)
    s, t = S.struct(), T.struct()
    L.check(lib.dm_wgrad(C.byref(s), C.byref(t), _ptr(slabs), None if pending is not None else _ptr(dst), B, CS, CT, Hs,
                         Ws, k, _stream()), "dm_wgrad")
    if pending is not None:
        pending.append((slabs, dst))
    return dst


def wgrad_t_affine2_supported(CS, CT, Hs, Ws, k):
    """True where dm_wgrad takes T as an AFFINE2 operand (a BatchNorm backward folded into the load of the output gradient)."""
    return bool(L.load().dm_wgrad_t_affine2_supported(CS, CT, Hs, Ws, k))


# ------------------------------------------------------------------ launch plans (host only)
Plan = collections.namedtuple("Plan", "kernel workgroups waves walkers dealing ring units")
_SOME = 64          # stands for a non-NULL device pointer in a plan query: the library reads which pointers are set, never what they point to


def _given(v):
    return v is not None and v is not False


def _plan_op(x, per_sample=False, ones=False):
    """dm_operand of a plan query from an Op (its tensors are not touched) or from a bare DM_LOAD_* mode; None: no operand."""
    if x is None:
        return _null_operand()
    if isinstance(x, Op):
        return L.Operand(_SOME, _SOME if x.p1 is not None else None, _SOME if x.coef is not None else None, x.bstride,
                         x.mode, 1 if x.ones else 0)
    mode = int(x)
    return L.Operand(_SOME, _SOME if mode == L.DM_LOAD_AFFINE2 else None, _SOME if mode >= L.DM_LOAD_AFFINE else None,
                     4 if per_sample else 0, mode, 1 if ones else 0)


def _plan_ep(mask=None, resid=None, stat_q=None, stats=None, per_tile=False, bias=None, bias_border=None, relu=False):
    """dm_epilogue of a plan query: every argument but `mask` (an Op or a mode) counts as present when it is not None / False;
    stat_q "gate" (or the mask Op's own tensor) = the gate tensor doubles as the statistics' second factor."""
    some = lambda v: _SOME if _given(v) else None
    gate = mask is not None and (stat_q == "gate" if isinstance(stat_q, str) else (isinstance(mask, Op) and stat_q is mask.p0))
    m = _plan_op(mask)
    return L.Epilogue(some(bias), some(bias_border), 1 if relu else 0, 1 if per_tile else 0, m, some(resid),
                      m.p0 if gate else (_SOME + 64 if _given(stat_q) else None), some(stats))


def _plan_wv(nfloats, scratch):
    return L.WeightView(_SOME, 0, 1, 1, 1, 1, _SOME if (scratch and nfloats > 0) else None, nfloats if scratch else 0)


def _plan_result(rc, plan, who):
    L.check(rc, who)
    return Plan(*(getattr(plan, k) for k in Plan._fields))


def _conv4_fallback(mode, epkw):
    """The operand / epilogue forms dm_conv4x4s2 keeps off its register-resident kernels (conv_mfma.hip, conv4_resident_takes)."""
    return mode == L.DM_LOAD_AFFINE2 or (_given(epkw.get("bias_border")) and
                                         any(_given(epkw.get(k)) for k in ("mask", "resid", "stat_q")))


def conv4x4s2_plan(inp, B, CIN, NOUT, H, W, per_sample=False, ones=False, scratch=True, **epkw):
    """Which kernel conv4x4s2 launches for this call and how it deals its units (include/dynamorph_hip.h, dm_launch_plan).
    inp: the Op of the call or a bare DM_LOAD_* mode (then per_sample / ones describe it); epkw as conv4x4s2 takes them, with
    True standing for any tensor and stat_q="gate" for the mask's own tensor; scratch: the weight view carries the scratch
    conv4x4s2 attaches.  Touches no device."""
    lib = L.load()
    o, e = _plan_op(inp, per_sample, ones), _plan_ep(**epkw)
    w = _plan_wv(lib.dm_conv4x4s2_scratch_floats(CIN, NOUT, H, W, 1 if _conv4_fallback(o.mode, epkw) else 0), scratch)
    plan = L.LaunchPlan()
    return _plan_result(lib.dm_conv4x4s2_plan(C.byref(o), C.byref(w), C.byref(e), B, CIN, NOUT, H, W, C.byref(plan)), plan,
                        "dm_conv4x4s2_plan")


def conv3x3_plan(inp, B, CIN, NOUT, H, W, taps=9, pixel_shuffle=False, per_sample=False, scratch=True, **epkw):
    """conv4x4s2_plan for a conv3x3 call (taps 9 or 1, or the transposed form)."""
    lib = L.load()
    o, e = _plan_op(inp, per_sample), _plan_ep(**epkw)
    w = _plan_wv(lib.dm_conv3x3_scratch_floats(CIN, NOUT, H, W, taps, 1 if pixel_shuffle else 0, 1 if epkw.get("per_tile") else 0),
                 scratch)
    plan = L.LaunchPlan()
    return _plan_result(lib.dm_conv3x3_plan(C.byref(o), C.byref(w), C.byref(e), B, CIN, NOUT, H, W, taps,
                                            1 if pixel_shuffle else 0, C.byref(plan)), plan, "dm_conv3x3_plan")


def wgrad_plan(S, T, B, CS, CT, Hs, Ws, k, per_sample=False, t_ones=False):
    """Which kernel wgrad launches (S, T: Ops or bare modes; per_sample: both carry per-sample coefficients; t_ones: T has the
    ones channel) and how it deals its units."""
    s, t = _plan_op(S, per_sample), _plan_op(T, per_sample, t_ones)
    plan = L.LaunchPlan()
    return _plan_result(L.load().dm_wgrad_plan(C.byref(s), C.byref(t), B, CS, CT, Hs, Ws, k, C.byref(plan)), plan, "dm_wgrad_plan")


def conv1x1_bwd_fused_plan(dy, B, CD, CX, H, W):
    """Which kernel conv1x1_bwd_fused launches (dy: Op or bare mode) and how it deals its units."""
    d = _plan_op(dy)
    plan = L.LaunchPlan()
    return _plan_result(L.load().dm_conv1x1_bwd_fused_plan(C.byref(d), B, CD, CX, H, W, C.byref(plan)), plan,
                        "dm_conv1x1_bwd_fused_plan")


def backward_precision(mode=None):
    """Arithmetic of the backward matrix products: "f32", the exact fp32 chain -- the only one built (the split-bf16 opt-in
    of earlier rounds is retired: include/dynamorph_hip.h, dm_backward_precision; asking for it raises).  mode None: query."""
    names = ("f32", "split-bf16")
    if mode is not None and mode not in names:
        raise ValueError(f"backward_precision: {mode!r} (one of {names})")
    prev = L.load().dm_backward_precision(-1 if mode is None else names.index(mode))
    L.check(min(prev, 0), "dm_backward_precision")
    return names[prev]


def _queue_or_reduce(slabs, dst, pending):
    """Weight-gradient slabs of a fused backward: queued as (slabs, dst) for reduce_slabs_multi, or (pending None) reduced
    into dst at once."""
    if pending is not None:
        pending.append((slabs, dst))
    else:
        reduce_slabs(slabs, dst)


def conv_bwd_s2_fused_supported(CD, CX, H, W):
    return bool(L.load().dm_conv_bwd_s2_fused_supported(CD, CX, H, W))


@_op
def conv_bwd_s2_fused(dy, tin, wv, dst, B, CD, CX, H, W, mask, stat_q=None, pending=None, want_stats=True):
    """Backward of a Conv2d(CX -> CD, 4, 2, 1) in one kernel (include/dynamorph_hip.h, dm_conv_bwd_s2_fused): data
    gradient (B, CX, 2H, 2W), masked by `mask` (the layer input, AFFINE) with its (sum, sum * input) statistics slabs, and
    the weight-gradient slabs, queued for reduce_slabs_multi into `dst` (pending) or reduced at once (pending None).
    dy: the output gradient as an AFFINE2 operand (BatchNorm backward folded in) on the (H, W) grid; tin: the layer input as
    the forward read it (AFFINE_RELU).  Returns (dx, stats)."""
    lib = L.load()
    nb = lib.dm_conv_bwd_s2_fused_num_blocks(B, CD, CX, H, W)
    if nb <= 0:
        raise ValueError(f"dm_conv_bwd_s2_fused: shape {(B, CD, CX, H, W)} not built")
    dx = _new((B, CX, 2 * H, 2 * W), dy.p0)
    stats = _new((nb, CX, 2), dy.p0, torch.float64) if want_stats else None
    slabs = _new((nb, CD * CX * 16), dy.p0)
    e = epilogue(mask=mask, stat_q=stat_q, stats=stats)
    d, t = dy.struct(), tin.struct()
    L.check(lib.dm_conv_bwd_s2_fused(C.byref(d), C.byref(t), wv.ref(), _ptr(dx), C.byref(e), _ptr(slabs), B, CD, CX, H, W,
                                     _stream()), "dm_conv_bwd_s2_fused")
    _queue_or_reduce(slabs, dst, pending)
    return dx, stats


def conv1x1_bwd_fused_supported(CD, CX, H, W):
    return bool(L.load().dm_conv1x1_bwd_fused_supported(CD, CX, H, W))


@_op
def conv1x1_bwd_fused(dy, x, xcoef, w, dst, B, CD, CX, H, W, pending=None):
    """Data AND weight gradient of a 1x1 convolution (CX -> CD channels) that feeds a train-mode BatchNorm, one launch
    (include/dynamorph_hip.h, dm_conv1x1_bwd_fused).  dy: Op of the output gradient (AFFINE2 = BatchNorm backward folded in);
    x: the layer input raw, xcoef (CX, 4) its BatchNorm + ReLU coefficients; w (CD, CX, 1, 1); dst: the weight gradient.
    Returns (dx, stats (nslabs, CX, 2)); the weight slabs are reduced into dst here, or queued on `pending`."""
    lib = L.load()
    nb = lib.dm_conv1x1_bwd_fused_num_blocks(B, CD, CX, H, W)
    if nb <= 0:
        raise ValueError(f"dm_conv1x1_bwd_fused: shape {CX} -> {CD} channels on {H}x{W} not built")
    dx = _new((B, CX, H, W), x)
    stats = _new((nb, CX, 2), x, torch.float64)
    slabs = _new((nb, CD * CX), x)
    d = dy.struct()
    L.check(lib.dm_conv1x1_bwd_fused(C.byref(d), _ptr(x), _ptr(xcoef), _ptr(w), _ptr(dx), _ptr(stats, torch.float64),
                                     _ptr(slabs), B, CD, CX, H, W, _stream()), "dm_conv1x1_bwd_fused")
    _queue_or_reduce(slabs, dst, pending)
    return dx, stats


def conv3x3_bwd_fused_supported(CD, CX, H, W):
    return bool(L.load().dm_conv3x3_bwd_fused_supported(CD, CX, H, W))


@_op
def conv3x3_bwd_fused(dy, x, xcoef, w, dst, B, CD, resid=None, q=None, want_stats=True, pending=None):
    """Data AND weight gradient of a 3x3 convolution (16 -> CD channels, 16 x 16 latents) that feeds a train-mode BatchNorm,
    one launch (include/dynamorph_hip.h, dm_conv3x3_bwd_fused).  dy: Op of the output gradient; x: the layer input raw,
    xcoef (16, 4) its BatchNorm + ReLU coefficients (None: plain ReLU); resid: added to dx; q: second factor of the statistics.
    Returns (dx, stats (nslabs, 16, 2) or None); the weight slabs are reduced into dst here, or queued on `pending`."""
    lib = L.load()
    CX, H, W = x.shape[1], x.shape[2], x.shape[3]
    nb = lib.dm_conv3x3_bwd_fused_num_blocks(B, CD, CX, H, W)
    if nb <= 0:
        raise ValueError(f"dm_conv3x3_bwd_fused: shape {CX} -> {CD} channels on {H}x{W} not built")
    dx = torch.empty_like(x)
    stats = _new((nb, CX, 2), x, torch.float64) if want_stats else None
    slabs = _new((nb, CD * CX * 9), x)
    d = dy.struct()
    L.check(lib.dm_conv3x3_bwd_fused(C.byref(d), _ptr(x), _ptr(xcoef), _ptr(w), _ptr(resid), _ptr(q), _ptr(dx),
                                     _ptr(stats, torch.float64), _ptr(slabs), B, CD, CX, H, W, _stream()),
            "dm_conv3x3_bwd_fused")
    _queue_or_reduce(slabs, dst, pending)
    return dx, stats


def conv4x4s2_bwd_fused_supported(CD, CX, H, W):
    return bool(L.load().dm_conv4x4s2_bwd_fused_supported(CD, CX, H, W))


@_op
def conv4x4s2_bwd_fused(dy, x, xcoef, w, dst, B, pending=None):
    """Data AND weight gradient of Conv2d(16 -> 16, 4, 2, 1) (enc.7) that feeds a train-mode BatchNorm, one launch
    (include/dynamorph_hip.h, dm_conv4x4s2_bwd_fused).  dy: Op of the output gradient (B, 16, 16, 16); x (B, 16, 32, 32): the
    layer input raw, xcoef (16, 4) its BatchNorm + ReLU coefficients.  Returns (dx, stats (nslabs, 16, 2))."""
    lib = L.load()
    CX, CD = x.shape[1], w.shape[0]
    H, W = x.shape[2] // 2, x.shape[3] // 2
    nb = lib.dm_conv4x4s2_bwd_fused_num_blocks(B, CD, CX, H, W)
    if nb <= 0:
        raise ValueError(f"dm_conv4x4s2_bwd_fused: shape {CX} -> {CD} channels, {H}x{W} output grid not built")
    dx = torch.empty_like(x)
    stats = _new((nb, CX, 2), x, torch.float64)
    slabs = _new((nb, CD * CX * 16), x)
    d = dy.struct()
    L.check(lib.dm_conv4x4s2_bwd_fused(C.byref(d), _ptr(x), _ptr(xcoef), _ptr(w), _ptr(dx), _ptr(stats, torch.float64),
                                       _ptr(slabs), B, CD, CX, H, W, _stream()), "dm_conv4x4s2_bwd_fused")
    _queue_or_reduce(slabs, dst, pending)
    return dx, stats


def convT_bwd_fused_supported(CI, CO, H, W):
    return bool(L.load().dm_convt_bwd_fused_supported(CI, CO, H, W))


@_op
def convT_bwd_fused(S, G, w, dst, mask_relu=False, want_stats=False, pending=None):
    """Input AND weight gradient of a thin ConvTranspose2d(CI -> CO, 4, 2, 1), one launch (include/dynamorph_hip.h,
    dm_convt_bwd_fused).  S (B, CI, H, W): the layer input; G (B, CO, 2H, 2W): the output gradient; w (CI, CO, 4, 4);
    dst: the weight gradient.  Returns (gin, stats (nslabs, CI, 2) or None); the weight slabs are reduced into dst here, or
    queued on `pending`."""
    lib = L.load()
    B, CI, H, W = S.shape
    CO = w.shape[1]
    if tuple(G.shape) != (B, CO, 2 * H, 2 * W) or tuple(w.shape) != (CI, CO, 4, 4):
        raise ValueError("dm_convt_bwd_fused: shapes do not match")
    nb = lib.dm_convt_bwd_fused_num_blocks(B, CI, CO, H, W)
    if nb <= 0:
        raise ValueError(f"dm_convt_bwd_fused: ConvTranspose2d({CI} -> {CO}) on {H}x{W} not built")
    gin = torch.empty_like(S)
    stats = _new((nb, CI, 2), S, torch.float64) if want_stats else None
    slabs = _new((nb, CI * CO * 16), S)
    L.check(lib.dm_convt_bwd_fused(_ptr(S), _ptr(G), _ptr(w), _ptr(gin), _ptr(stats, torch.float64), _ptr(slabs),
                                   1 if mask_relu else 0, B, CI, CO, H, W, _stream()), "dm_convt_bwd_fused")
    _queue_or_reduce(slabs, dst, pending)
    return gin, stats


def pend_stats(pending, stats, dsts):
    """Queue the column sums of a statistics slab tensor (nslabs, N, 2) for reduce_slabs_multi: consecutive runs of
    columns go to the tensors `dsts` (what sum_slabs / sum_slabs_scatter would do in a launch of their own)."""
    col = 0
    for d in dsts:
        pending.append((stats, d, col))
        col += d.numel()
    if col != stats.shape[1]:
        raise ValueError("pend_stats: destinations must cover the slab's columns")


@_op
def reduce_slabs_multi(pending):
    """One launch for every (slabs, dst) pair collected by wgrad(..., pending=...) and every (stats, dst, column) run
    queued by pend_stats."""
    lib = L.load()
    while pending:
        chunk, pending[:] = pending[:32], pending[32:]
        segs = (L.ReduceSeg * len(chunk))()
        for i, item in enumerate(chunk):
            if len(item) == 3:      # (stats (nslabs, N, 2) float64, dst, first column): a run of columns of a statistics slab
                stats, dst, col = item
                if stats.dtype != torch.float64 or stats.dim() != 3 or col + dst.numel() > stats.shape[1]:
                    raise ValueError("reduce_slabs_multi: bad statistics segment")
                _ptr(stats, torch.float64)
                segs[i] = L.ReduceSeg(stats.data_ptr() + 16 * col, _ptr(dst), stats.shape[0], dst.numel(), stats.shape[1], 1)
            else:
                slabs, dst = item
                segs[i] = L.ReduceSeg(_ptr(slabs), _ptr(dst), slabs.shape[0], slabs.shape[1], 0, 0)
        L.check(lib.dm_reduce_slabs_multi(segs, len(chunk), _stream()), "dm_reduce_slabs_multi")


@_op
def sum_slabs_scatter(stats, dsts, scale=1.0):
    """stats (nslabs, N, 2) float64 -> consecutive runs of the N sums written straight into the tensors `dsts`."""
    lib = L.load()
    N = stats.shape[1]
    sc = L.Scatter()
    sc.nseg = len(dsts)
    end = 0
    for k, d in enumerate(dsts):
        end += d.numel()
        sc.end[k] = end
        sc.dst[k] = _ptr(d)
    if end != N:
        raise ValueError(f"dm_sum_slabs_scatter: destinations cover {end} of {N} entries")
    L.check(lib.dm_sum_slabs_scatter(_ptr(stats, torch.float64), stats.shape[0], N, scale, C.byref(sc), _stream()),
            "dm_sum_slabs_scatter")


# ------------------------------------------------------------------------ BatchNorm
@_op
def bn_finalize(stats, count_per_group, gamma, beta, running_mean, running_var, nbt, momentum, eps,
                per_sample=False, slabs_per_group=1, defer=None):
    """defer (per_sample only): a list -> the running statistics are NOT touched by this launch; their update is appended
    to the list for bn_running_replay, which brings every deferred layer up to date in one launch."""
    lib = L.load()
    nslabs, Cn = stats.shape[0], stats.shape[1]
    if per_sample and defer is not None:
        defer.append((stats, slabs_per_group, count_per_group, running_mean, running_var, nbt, momentum))
        running_mean = running_var = nbt = None
    if per_sample:
        Bn = nslabs // slabs_per_group
        coef = _new((Bn, Cn, 4), gamma)
        saved = _new((Bn, Cn, 2), gamma)
    else:
        coef = _new((Cn, 4), gamma)
        saved = _new((Cn, 2), gamma)
    L.check(lib.dm_bn_finalize(_ptr(stats, torch.float64), nslabs, slabs_per_group, Cn, count_per_group, _ptr(gamma),
                               _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(nbt, torch.int64), momentum,
                               eps, _ptr(coef), _ptr(saved), 1 if per_sample else 0, _stream()), "dm_bn_finalize")
    return coef, saved


@_op
def bn_running_replay(deferred):
    """One launch for the running statistics of every layer bn_finalize(..., defer=deferred) skipped."""
    lib = L.load()
    while deferred:
        chunk, deferred[:] = deferred[:16], deferred[16:]
        segs = (L.ReplaySeg * len(chunk))()
        for i, (stats, spg, cnt, rm, rv, nbt, mom) in enumerate(chunk):
            segs[i] = L.ReplaySeg(_ptr(stats, torch.float64), stats.shape[0], spg, stats.shape[1], cnt, _ptr(rm), _ptr(rv),
                                  _ptr(nbt, torch.int64), mom)
        L.check(lib.dm_bn_running_replay(segs, len(chunk), _stream()), "dm_bn_running_replay")


def latent_tail_supported(c, cr, h, w, nres):
    return bool(L.load().dm_latent_tail_supported(c, cr, h, w, nres))


@_op
def latent_tail_forward(a3, coef3, w10, b10, gamma4, beta4, eps4, res):
    """enc.10 .. enc.12 of every patch with that patch's own BatchNorm statistics, one launch (csrc/latent_tail.hip).
    res: per residual layer (wa, ba, gamma_a, beta_a, eps_a, wb, bb, gamma_b, beta_b, eps_b).
    Returns (z, stats4, [(stats_a, stats_b), ...]): the per-patch sums (B, C, 2) float64 for bn_running_replay."""
    lib = L.load()
    B, Cn, H, W = a3.shape
    z = _new((B, Cn, H, W), a3)
    st4 = _new((B, Cn, 2), a3, torch.float64)
    args = L.LatentTailArgs()
    args.a3, args.coef3 = _ptr(a3), _ptr(coef3)
    args.w10, args.b10 = _ptr(w10), _ptr(b10)
    args.gamma4, args.beta4, args.stats4, args.z = _ptr(gamma4), _ptr(beta4), _ptr(st4, torch.float64), _ptr(z)
    args.eps4, args.B, args.C, args.H, args.W, args.nres = eps4, B, Cn, H, W, len(res)
    args.CR = res[0][0].shape[0] if res else 32
    sts = []
    for i, (wa, ba, ga, bea, epsa, wb, bb, gb, beb, epsb) in enumerate(res):
        sa = _new((B, wa.shape[0], 2), a3, torch.float64)
        sb = _new((B, wb.shape[0], 2), a3, torch.float64)
        r = args.res[i]
        r.wa, r.ba, r.gamma_a, r.beta_a, r.stats_a, r.eps_a = _ptr(wa), _ptr(ba), _ptr(ga), _ptr(bea), _ptr(sa, torch.float64), epsa
        r.wb, r.bb, r.gamma_b, r.beta_b, r.stats_b, r.eps_b = _ptr(wb), _ptr(bb), _ptr(gb), _ptr(beb), _ptr(sb, torch.float64), epsb
        sts.append((sa, sb))
    L.check(lib.dm_latent_tail_forward(C.byref(args), _stream()), "dm_latent_tail_forward")
    return z, st4, sts


@_op
def latent_tail_backward(g_z, a3, coef3, a4, saved4, gamma4, w10, res):
    """The data-only backward of enc.12 .. enc.10 of every patch with that patch's own BatchNorm sums, one launch
    (csrc/latent_tail_bwd.hip; latent_tail_supported is its gate).  res: per residual layer (ra, rb, h_in, coefa, saveda, savedb,
    gamma_a, gamma_b, wa, wb) as the per-sample forward saved them.  Returns (dy3 (B, C, H, W), already masked by
    relu(BN3(a3)), stats3 (B, C, 2) float64 = (sum dy3, sum dy3 * a3) per patch)."""
    lib = L.load()
    B, Cn, H, W = g_z.shape
    if coef3.dim() != 3 or saved4.dim() != 3:
        raise ValueError("dm_latent_tail_backward: per-sample coefficients (B, C, 4) and saved statistics (B, C, 2)")
    dy3 = torch.empty_like(g_z)
    st3 = _new((B, Cn, 2), g_z, torch.float64)
    args = L.LatentTailBwdArgs()
    args.g_z, args.a3, args.coef3, args.a4, args.saved4 = _ptr(g_z), _ptr(a3), _ptr(coef3), _ptr(a4), _ptr(saved4)
    args.gamma4, args.w10, args.dy3, args.stats3 = _ptr(gamma4), _ptr(w10), _ptr(dy3), _ptr(st3, torch.float64)
    args.B, args.C, args.H, args.W, args.nres = B, Cn, H, W, len(res)
    args.CR = res[0][0].shape[1] if res else 32
    for i, layer in enumerate(res):
        ra, rb, h_in, coefa, saveda, savedb = layer[:6]
        if coefa.dim() != 3 or saveda.dim() != 3 or savedb.dim() != 3 or tuple(rb.shape) != tuple(g_z.shape) or \
                tuple(h_in.shape) != tuple(g_z.shape) or ra.shape[0] != B:
            raise ValueError("dm_latent_tail_backward: residual layer %d: per-sample tensors of the batch's shape" % i)
        for k, t in zip(("ra", "rb", "h_in", "coefa", "saveda", "savedb", "gamma_a", "gamma_b", "wa", "wb"), layer):
            setattr(args.res[i], k, _ptr(t))
    L.check(lib.dm_latent_tail_backward(C.byref(args), _stream()), "dm_latent_tail_backward")
    return dy3, st3


@_op
def bn_backward_finalize(stats, count, gamma, saved, dgamma, dbeta):
    lib = L.load()
    nslabs, Cn = stats.shape[0], stats.shape[1]
    coef_bwd = _new((Cn, 4), gamma)
    L.check(lib.dm_bn_backward_finalize(_ptr(stats, torch.float64), nslabs, Cn, count, _ptr(gamma), _ptr(saved),
                                        _ptr(dgamma), _ptr(dbeta), _ptr(coef_bwd), _stream()), "dm_bn_backward_finalize")
    return coef_bwd


@_op
def bn_backward_finalize_per_sample(stats, slabs_per_group, count_per_group, gamma, saved, dgamma=None, dbeta=None):
    """bn_backward_finalize with every patch its own batch: stats (B * slabs_per_group, C, 2) grouped by patch, saved
    (B, C, 2) from bn_finalize(per_sample=True), count_per_group the positions of one patch.  Returns the (B, C, 4) AFFINE2
    coefficients; dgamma / dbeta (or None: not computed) get the sums over the patches, in index order."""
    lib = L.load()
    nslabs, Cn = stats.shape[0], stats.shape[1]
    if slabs_per_group <= 0 or nslabs % slabs_per_group or tuple(saved.shape) != (nslabs // slabs_per_group, Cn, 2):
        raise ValueError(f"dm_bn_backward_finalize_per_sample: {nslabs} slabs in groups of {slabs_per_group} against saved "
                         f"statistics {tuple(saved.shape)}")
    coef_bwd = _new((nslabs // slabs_per_group, Cn, 4), gamma)
    L.check(lib.dm_bn_backward_finalize_per_sample(_ptr(stats, torch.float64), nslabs, slabs_per_group, Cn, count_per_group,
                                                   _ptr(gamma), _ptr(saved), _ptr(dgamma), _ptr(dbeta), _ptr(coef_bwd),
                                                   _stream()), "dm_bn_backward_finalize_per_sample")
    return coef_bwd


# synchronized BatchNorm (data parallel): a layer's statistics as one float64 payload the ranks all-reduce between two launches;
# weight is a 1-element float64 device tensor (read at run time: a captured graph replays for any global batch)
@_op
def bn_sync_pack(stats, count, weight):
    """(nslabs, C, 2) slabs -> payload (2C+1,) = weight * [sum x, sum x^2, count]."""
    lib = L.load()
    nslabs, Cn = stats.shape[0], stats.shape[1]
    payload = _new((2 * Cn + 1,), stats, torch.float64)
    L.check(lib.dm_bn_sync_pack(_ptr(stats, torch.float64), nslabs, Cn, count, _ptr(weight, torch.float64),
                                _ptr(payload, torch.float64), _stream()), "dm_bn_sync_pack")
    return payload


@_op
def bn_finalize_payload(payload, gamma, beta, running_mean, running_var, nbt, momentum, eps):
    """bn_finalize on the all-reduced payload (global count at payload[2C]) -> (coef, saved)."""
    lib = L.load()
    Cn = (payload.numel() - 1) // 2
    coef = _new((Cn, 4), gamma)
    saved = _new((Cn, 2), gamma)
    L.check(lib.dm_bn_finalize_payload(_ptr(payload, torch.float64), Cn, _ptr(gamma), _ptr(beta), _ptr(running_mean),
                                       _ptr(running_var), _ptr(nbt, torch.int64), momentum, eps, _ptr(coef), _ptr(saved),
                                       _stream()), "dm_bn_finalize_payload")
    return coef, saved


@_op
def bn_backward_pack(stats, saved, weight, dgamma, dbeta):
    """dgamma / dbeta from the local (sum dy, sum dy*a) slabs; returns the payload (2C,) = weight * [sum dy, sum dy*a]."""
    lib = L.load()
    nslabs, Cn = stats.shape[0], stats.shape[1]
    payload = _new((2 * Cn,), stats, torch.float64)
    L.check(lib.dm_bn_backward_pack(_ptr(stats, torch.float64), nslabs, Cn, _ptr(saved), _ptr(weight, torch.float64),
                                    _ptr(dgamma), _ptr(dbeta), _ptr(payload, torch.float64), _stream()), "dm_bn_backward_pack")
    return payload


@_op
def bn_backward_payload(payload, fwd_payload, gamma, saved, weight):
    """The AFFINE2 coefficients of da from the all-reduced backward payload; fwd_payload: the layer's all-reduced forward
    payload (its global count), weight: this rank's gradient weight."""
    lib = L.load()
    Cn = payload.numel() // 2
    coef_bwd = _new((Cn, 4), gamma)
    L.check(lib.dm_bn_backward_payload(_ptr(payload, torch.float64), _ptr(fwd_payload, torch.float64), Cn, _ptr(gamma),
                                       _ptr(saved), _ptr(weight, torch.float64), _ptr(coef_bwd), _stream()),
            "dm_bn_backward_payload")
    return coef_bwd


@_op
def apply(inp, B, Cn, H, W, resid=None, out=None):
    lib = L.load()
    if out is None:
        out = _new((B, Cn, H, W), inp.p0)
    o = inp.struct()
    L.check(lib.dm_apply(C.byref(o), _ptr(resid), _ptr(out), B, Cn, H, W, _stream()), "dm_apply")
    return out


@_op
def channel_stats(p, q=None):
    lib = L.load()
    B, Cn, H, W = p.shape
    nb = lib.dm_channel_stats_num_blocks(B, Cn, H, W)
    stats = _new((nb, Cn, 2), p, torch.float64)
    L.check(lib.dm_channel_stats(_ptr(p), _ptr(q), _ptr(stats, torch.float64), B, Cn, H, W, _stream()), "dm_channel_stats")
    return stats


@_op
def channel_stats_per_sample(p, q=None):
    """(B, C, 2) float64: (sum p, sum p*q) of every patch on its own -- the slabs bn_backward_finalize_per_sample takes."""
    lib = L.load()
    B, Cn, H, W = p.shape
    stats = _new((B, Cn, 2), p, torch.float64)
    L.check(lib.dm_channel_stats_per_sample(_ptr(p), _ptr(q), _ptr(stats, torch.float64), B, Cn, H, W, _stream()),
            "dm_channel_stats_per_sample")
    return stats


@_op
def sum_slabs(stats, dst, scale=1.0, n=None):
    """dst[i] = scale * sum_slabs stats[slab][i][0] for all N = stats.shape[1] entries of the slab rows.  The kernel
    writes N values: a shorter dst (or an n other than N) is refused here instead of being written past its end."""
    lib = L.load()
    N = stats.shape[1]
    if dst.numel() < N or (n is not None and n != N):
        raise ValueError(f"dm_sum_slabs: the slab rows have {N} entries, dst {dst.numel()}, n {n}")
    L.check(lib.dm_sum_slabs(_ptr(stats, torch.float64), stats.shape[0], N, scale, _ptr(dst), _stream()), "dm_sum_slabs")
    return dst


# ------------------------------------------------------------------------------ head
@_op
def head_forward(d4, w6, b6, x, mask, channel_var):
    lib = L.load()
    B, C4, H, W = d4.shape
    NIN = w6.shape[0]
    dec = _new((B, NIN, H, W), d4)
    slabs = None
    if x is not None:
        slabs = _new((lib.dm_head_num_blocks(B, H, W),), d4, torch.float64)
    mc = mask.shape[1] if mask is not None else 0
    L.check(lib.dm_head_forward(_ptr(d4), _ptr(w6), _ptr(b6), _ptr(x), _ptr(mask), mc, _ptr(channel_var), _ptr(dec),
                                _ptr(slabs, torch.float64), B, C4, NIN, H, W, _stream()), "dm_head_forward")
    return dec, slabs


@_op
def head_backward(dec, x, mask, channel_var, d4, w6, gscale, gdec_ext=None):
    """Returns (g4, part) with part: (nblocks, NIN*C4 + NIN + C4, 2) float64 slabs."""
    lib = L.load()
    B, C4, H, W = d4.shape
    NIN = w6.shape[0]
    g4 = torch.empty_like(d4)
    part = _new((lib.dm_head_num_blocks(B, H, W), NIN * C4 + NIN + C4, 2), d4, torch.float64)
    mc = mask.shape[1] if mask is not None else 0
    L.check(lib.dm_head_backward(_ptr(dec), _ptr(x), _ptr(mask), mc, _ptr(channel_var), _ptr(d4), _ptr(w6),
                                 _ptr(gscale), _ptr(gdec_ext), _ptr(g4), _ptr(part, torch.float64), B, C4, NIN, H, W,
                                 _stream()), "dm_head_backward")
    return g4, part


def head_supported(c4, nin):
    return bool(L.load().dm_head_supported(c4, nin))


def dec_tail_supported(c2, nin, h2, w2):
    return bool(L.load().dm_dec_tail_supported(c2, nin, h2, w2))


@_op
def dec_tail_forward(d2, w4, b4, w6, b6, x, mask, channel_var):
    """Fused dec.4 + ReLU + dec.6 (+ masked reconstruction loss partials when x is given)."""
    lib = L.load()
    B, C2, H2, W2 = d2.shape
    NIN = w6.shape[0]
    dec = _new((B, NIN, 2 * H2, 2 * W2), d2)
    slabs = _new((lib.dm_dec_tail_num_blocks(B, H2, W2),), d2, torch.float64) if x is not None else None
    mc = mask.shape[1] if mask is not None else 0
    L.check(lib.dm_dec_tail_forward(_ptr(d2), _ptr(w4), _ptr(b4), _ptr(w6), _ptr(b6), _ptr(x), _ptr(mask), mc,
                                    _ptr(channel_var), _ptr(dec), _ptr(slabs, torch.float64), B, C2, NIN, H2, W2,
                                    _stream()), "dm_dec_tail_forward")
    return dec, slabs


@_op
def dec_tail_backward(d2, w4, b4, w6, dec, x, mask, channel_var, gscale):
    """Returns (g2, part (nb, NIN*4+NIN+8, 2) float64, w_slabs (nb, 256) float32)."""
    lib = L.load()
    B, C2, H2, W2 = d2.shape
    NIN = w6.shape[0]
    nb = lib.dm_dec_tail_num_blocks(B, H2, W2)
    g2 = torch.empty_like(d2)
    part = _new((nb, NIN * C2 + NIN + 2 * C2, 2), d2, torch.float64)
    wsl = _new((nb, C2 * C2 * 16), d2)
    mc = mask.shape[1] if mask is not None else 0
    L.check(lib.dm_dec_tail_backward(_ptr(d2), _ptr(w4), _ptr(b4), _ptr(w6), _ptr(dec), _ptr(x), _ptr(mask), mc,
                                     _ptr(channel_var), _ptr(gscale), _ptr(g2), _ptr(part, torch.float64), _ptr(wsl),
                                     B, C2, NIN, H2, W2, _stream()), "dm_dec_tail_backward")
    return g2, part, wsl


@_op
def dec_tail_train(d2, w4, b4, w6, b6, x, mask, channel_var, gscale):
    """Forward loss + backward of the decoder tail in one kernel (no `decoded`).
    Returns (g2, part, w_slabs, loss_slabs)."""
    lib = L.load()
    B, C2, H2, W2 = d2.shape
    NIN = w6.shape[0]
    nb = lib.dm_dec_tail_num_blocks(B, H2, W2)
    g2 = torch.empty_like(d2)
    part = _new((nb, NIN * C2 + NIN + 2 * C2, 2), d2, torch.float64)
    wsl = _new((nb, C2 * C2 * 16), d2)
    loss = _new((nb,), d2, torch.float64)
    mc = mask.shape[1] if mask is not None else 0
    L.check(lib.dm_dec_tail_train(_ptr(d2), _ptr(w4), _ptr(b4), _ptr(w6), _ptr(b6), _ptr(x), _ptr(mask), mc,
                                  _ptr(channel_var), _ptr(gscale), _ptr(g2), _ptr(part, torch.float64), _ptr(wsl),
                                  _ptr(loss, torch.float64), B, C2, NIN, H2, W2, _stream()), "dm_dec_tail_train")
    return g2, part, wsl, loss


@_op
def reduce_slabs(slabs, dst):
    lib = L.load()
    L.check(lib.dm_reduce_slabs(_ptr(slabs), slabs.shape[0], slabs.shape[1], _ptr(dst), _stream()), "dm_reduce_slabs")
    return dst


@_op
def loss_finalize(loss_slabs, count, vq_scalars, weight_recon, weight_commitment):
    lib = L.load()
    out = _new((4,), vq_scalars)
    L.check(lib.dm_loss_finalize(_ptr(loss_slabs, torch.float64), loss_slabs.numel(), count, _ptr(vq_scalars),
                                 weight_recon, weight_commitment, _ptr(out), _stream()), "dm_loss_finalize")
    return out


# ------------------------------------------------------------------ plain reconstruction loss
@_op
def recon_loss(dec, x, mask, channel_var):
    """Partial sums (nblocks,) float64 of (dec*m - x*m)^2 / var for loss_finalize."""
    lib = L.load()
    B, NIN, H, W = dec.shape
    slabs = _new((lib.dm_recon_loss_num_blocks(B, NIN, H, W),), dec, torch.float64)
    mc = mask.shape[1] if mask is not None else 0
    L.check(lib.dm_recon_loss(_ptr(dec), _ptr(x), _ptr(mask), mc, _ptr(channel_var), _ptr(slabs, torch.float64),
                              B, NIN, H, W, _stream()), "dm_recon_loss")
    return slabs


@_op
def recon_loss_backward(dec, x, mask, channel_var, gscale):
    """(g_decoded, bias_slabs (nblocks, NIN, 2) float64)."""
    lib = L.load()
    B, NIN, H, W = dec.shape
    g = torch.empty_like(dec)
    part = _new((lib.dm_recon_loss_num_blocks(B, NIN, H, W), NIN, 2), dec, torch.float64)
    mc = mask.shape[1] if mask is not None else 0
    L.check(lib.dm_recon_loss_backward(_ptr(dec), _ptr(x), _ptr(mask), mc, _ptr(channel_var), _ptr(gscale), _ptr(g),
                                       _ptr(part, torch.float64), B, NIN, H, W, _stream()), "dm_recon_loss_backward")
    return g, part


# ------------------------------------------------------------------ per-patch scores
@_op
def dec_tail_score(d2, w4, b4, w6, b6, x, mask, channel_var, want_decoded=False):
    """dec_tail_forward with the loss sums kept per patch and channel (include/dynamorph_hip.h, dm_dec_tail_score).
    Returns (decoded or None, patch_sums (B, NIN) float64); `decoded` is not written unless asked for."""
    lib = L.load()
    B, C2, H2, W2 = d2.shape
    NIN = w6.shape[0]
    dec = _new((B, NIN, 2 * H2, 2 * W2), d2) if want_decoded else None
    sums = _new((B, NIN), d2, torch.float64)
    wsb = lib.dm_dec_tail_score_workspace_bytes(B, NIN, H2, W2)
    ws = _new((max(wsb // 8, 1),), d2, torch.float64)
    mc = mask.shape[1] if mask is not None else 0
    L.check(lib.dm_dec_tail_score(_ptr(d2), _ptr(w4), _ptr(b4), _ptr(w6), _ptr(b6), _ptr(x), _ptr(mask), mc,
                                  _ptr(channel_var), _ptr(dec), _ptr(sums, torch.float64), _ptr(ws, torch.float64), wsb,
                                  B, C2, NIN, H2, W2, _stream()), "dm_dec_tail_score")
    return dec, sums


@_op
def recon_loss_per_sample(dec, x, mask, channel_var):
    """patch_sums (B, NIN) float64 of (dec*m - x*m)^2 / var from a stored `dec`; any H and W."""
    lib = L.load()
    B, NIN, H, W = dec.shape
    sums = _new((B, NIN), dec, torch.float64)
    mc = mask.shape[1] if mask is not None else 0
    L.check(lib.dm_recon_loss_per_sample(_ptr(dec), _ptr(x), _ptr(mask), mc, _ptr(channel_var), _ptr(sums, torch.float64),
                                         B, NIN, H, W, _stream()), "dm_recon_loss_per_sample")
    return sums


@_op
def vq_patch_scalars(z, idx, codebook, commitment_cost, want_counts=False, ema=False):
    """Per patch (loss, perplexity, mse) as a (B, 3) tensor, and the (B, K) int32 code histogram on request (else None).
    ema: the loss of the EMA codebook mode, cc * mse (dm_vq_patch_scalars_ema)."""
    lib = L.load()
    B, D, H, W = z.shape
    K = codebook.shape[0]
    if tuple(idx.shape) != (B, H, W) or codebook.shape[1] != D:
        raise ValueError("dm_vq_patch_scalars: z (B, D, H, W), idx (B, H, W), codebook (K, D)")
    scalars = _new((B, 3), z)
    counts = _new((B, K), z, torch.int32) if want_counts else None
    fn = lib.dm_vq_patch_scalars_ema if ema else lib.dm_vq_patch_scalars
    L.check(fn(_ptr(z), _ptr(idx, torch.int64), _ptr(codebook), commitment_cost, _ptr(scalars),
               _ptr(counts, torch.int32), B, D, K, H, W, _stream()), "dm_vq_patch_scalars_ema" if ema else "dm_vq_patch_scalars")
    return scalars, counts


@_op
def score_finalize(patch_sums, vq_scalars, weight_recon, weight_commitment, chw):
    """(B, 4 + NIN): recon, commitment, total, perplexity, recon per channel."""
    lib = L.load()
    B, NIN = patch_sums.shape
    out = _new((B, 4 + NIN), vq_scalars)
    L.check(lib.dm_score_finalize(_ptr(patch_sums, torch.float64), _ptr(vq_scalars), weight_recon, weight_commitment, chw,
                                  _ptr(out), B, NIN, _stream()), "dm_score_finalize")
    return out


# ------------------------------------------------------------------ time-matching loss
@_op
def pair_msd(z):
    """z (B, n) contiguous -> sim (B, B), sim[i][j] = mean((z[i] - z[j])**2)."""
    lib = L.load()
    B, n = z.shape
    sim = _new((B, B), z)
    L.check(lib.dm_pair_msd(_ptr(z), _ptr(sim), B, n, _stream()), "dm_pair_msd")
    return sim


@_op
def pair_msd_backward(z, g_sim):
    lib = L.load()
    B, n = z.shape
    dz = torch.empty_like(z)
    L.check(lib.dm_pair_msd_backward(_ptr(z), _ptr(g_sim), _ptr(dz), B, n, _stream()), "dm_pair_msd_backward")
    return dz


def time_matching_supported(B, n):
    return bool(L.load().dm_time_matching_supported(B, n))


def _tm_forward(z, tm, mode, weights, rows=None, stateless=False):
    """Both forward wrappers: the size queries, the allocations, the launch, and the state block attached to S.  rows:
    (r0, R) for the row-range form, None for the square one.  Returns (slabs, S)."""
    lib = L.load()
    B, n = z.shape
    if rows is None:
        r0, R = 0, B
        wsf, nsl, ints = (lib.dm_time_matching_workspace_floats(B, n), lib.dm_time_matching_num_slabs(B),
                          lib.dm_time_matching_state_ints(B))
    else:
        r0, R = rows
        wsf, nsl, ints = (lib.dm_time_matching_rows_workspace_floats(B, R, n), lib.dm_time_matching_rows_num_slabs(B, R),
                          lib.dm_time_matching_rows_state_ints(B, R))
    ws = _new((max(wsf, 1),), z)
    S = _new((2, R, B), z)
    slabs = _new((nsl, 1, 2), z, torch.float64)
    # the state block the backward call reads (the pair count of mode 0's sparse form and the map of S's nonzero blocks:
    # include/dynamorph_hip.h) travels with S as an attribute; an S that lost it (a copy, a slice) takes the dense product,
    # which gives the same gradient
    state = None if stateless else torch.empty(ints, dtype=torch.int32, device=z.device)
    if R > 0:
        name = "dm_time_matching_forward" + ("_rows" if rows is not None else "" if stateless else "_state")
        shape = (B, n) if rows is None else (B, r0, R, n)
        L.check(getattr(lib, name)(_ptr(z), _ptr(tm), *shape, mode, *weights, _ptr(ws), wsf, _ptr(S), _ptr(slabs, torch.float64),
                                   *(() if stateless else (_ptr(state, torch.int32),)), _stream()), name)
    if not stateless:
        S._dm_tm_state = state
    if rows is not None:
        S._dm_tm_rows = (r0, R)
    return slabs, S


def _tm_backward(z, S, g_loss, scale, add, rows=None):
    """Both backward wrappers: dz for the rows S was formed for, by the entry point that takes what the call has."""
    lib = L.load()
    B, n = z.shape
    r0, R = rows if rows is not None else (0, B)
    dz = _new((R, n), z)
    state = getattr(S, "_dm_tm_state", None)
    if R > 0:
        head = (_ptr(z), _ptr(S), _ptr(g_loss), scale)
        if rows is not None:
            name, args = "dm_time_matching_backward_rows", (_ptr(add), _ptr(dz), B, r0, R, n, _ptr(state, torch.int32))
        elif state is not None:
            name, args = "dm_time_matching_backward_state", (_ptr(add), _ptr(dz), B, n, _ptr(state, torch.int32))
        elif add is not None:
            name, args = "dm_time_matching_backward_add", (_ptr(add), _ptr(dz), B, n)
        else:
            name, args = "dm_time_matching_backward", (_ptr(dz), B, n)
        L.check(getattr(lib, name)(*head, *args, _stream()), name)
    return dz


@_op
def time_matching_forward(z, tm, mode, w_a=0.0, w_t=0.0, w_n=0.0, margin=0.0, want_slabs=False, allow_sparse=True):
    """The whole pairwise term on the MFMA (include/dynamorph_hip.h, dm_time_matching_forward).  z (B, n), tm (B, B) float32.
    Returns (loss: 1-element device tensor, S (2, B, B) = dloss/dsim + its transpose, far pairs / near pairs, for
    time_matching_backward).  want_slabs: the partial losses (nslabs, 1, 2) float64 instead of their sum (the training
    step's scalar launch adds them: vq_loss_finalize_tm)."""
    # (allow_sparse=False -- tests / measurements --: the stateless, dense form whatever tm holds)
    slabs, S = _tm_forward(z, tm, mode, (w_a, w_t, w_n, margin), stateless=not allow_sparse)
    return (slabs, S) if want_slabs else (sum_slabs(slabs, _new((1,), z)), S)


@_op
def time_matching_backward(z, S, g_loss=None, scale=1.0, add=None):
    """dz = [add +] scale * g_loss[0] * d loss / d z  (g_loss: 1-element device tensor or None = 1; add: a gradient of the
    same latents, (B, n) or any shape with as many elements, summed in the kernel's store instead of an elementwise pass)."""
    if add is not None and add.numel() != z.numel():
        raise ValueError("dm_time_matching_backward_add: `add` must have the latents' size")
    return _tm_backward(z, S, g_loss, scale, add)


@_op
def time_matching_forward_rows(z, tm, r0, R, mode, w_a=0.0, w_t=0.0, w_n=0.0, margin=0.0, want_slabs=False):
    """The pairwise term for the rows [r0, r0 + R) of a batch against all of it (include/dynamorph_hip.h,
    dm_time_matching_forward_rows): z (B, n) the latents of the WHOLE batch, tm (B, B) its whole relation block.  Returns
    (the rows' share of the loss: 1-element float64 tensor -- the shares of a partition of the rows add up to
    time_matching_forward's loss --, S (2, R, B) for time_matching_backward_rows).  want_slabs: the partial losses
    (nslabs, 1, 2) float64 instead of their sum.  R = 0 is allowed (an empty shard: a zero share, nothing launched)."""
    B = z.shape[0]
    if tm.shape != (B, B):
        raise ValueError(f"time_matching_forward_rows: relation block {tuple(tm.shape)} for a batch of {B}")
    slabs, S = _tm_forward(z, tm, mode, (w_a, w_t, w_n, margin), rows=(r0, R))
    return (slabs, S) if want_slabs else (slabs[:, 0, 0].sum().reshape(1), S)


@_op
def time_matching_backward_rows(z, S, g_loss=None, scale=1.0, add=None):
    """dz (R, n) = [add +] scale * g_loss[0] * d loss / d z for the rows S was formed for (time_matching_forward_rows on the
    same z): rows r0 .. r0 + R - 1 of time_matching_backward's dz.  add: (R, n) or as many elements, summed in the store."""
    if add is not None and add.numel() != S._dm_tm_rows[1] * z.shape[1]:
        raise ValueError("dm_time_matching_backward_rows: `add` must have the rows' size")
    return _tm_backward(z, S, g_loss, scale, add, rows=S._dm_tm_rows)


# ------------------------------------------------------------- composition / optimizer
@_op
def e1_compose(w0, b0, w1):
    lib = L.load()
    C0, NIN = w0.shape[0], w0.shape[1]
    C1 = w1.shape[0]
    weff = _new((C1, NIN + 1, 4, 4), w1)
    L.check(lib.dm_e1_compose(_ptr(w0), _ptr(b0), _ptr(w1), _ptr(weff), NIN, C0, C1, _stream()), "dm_e1_compose")
    return weff


@_op
def e1_compose_border(w0, b0, w1, b1):
    """(weff, bias_border): bias_border (3, 3, C1) replaces the ones channel in the forward conv."""
    lib = L.load()
    C0, NIN = w0.shape[0], w0.shape[1]
    C1 = w1.shape[0]
    weff = _new((C1, NIN + 1, 4, 4), w1)
    table = _new((3, 3, C1), w1)
    L.check(lib.dm_e1_compose_border(_ptr(w0), _ptr(b0), _ptr(w1), _ptr(b1), _ptr(weff), _ptr(table), NIN, C0, C1,
                                     _stream()), "dm_e1_compose_border")
    return weff, table


@_op
def e1_chain(dweff, w0, b0, w1, dw0, db0, dw1):
    lib = L.load()
    C0, NIN = w0.shape[0], w0.shape[1]
    C1 = w1.shape[0]
    L.check(lib.dm_e1_chain(_ptr(dweff), _ptr(w0), _ptr(b0), _ptr(w1), _ptr(dw0), _ptr(db0), _ptr(dw1), NIN, C0, C1,
                            _stream()), "dm_e1_chain")


@_op
def adam(param, grad, m, v, lr, beta1, beta2, eps, step_dev):
    lib = L.load()
    L.check(lib.dm_adam(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), param.numel(), lr, beta1, beta2, eps,
                        _ptr(step_dev), _stream()), "dm_adam")


@_op
def adam_counted(param, grad, m, v, lr, beta1, beta2, eps, steps_done, steps_done_next, grad_scale=1.0):
    """grad_scale != 1: the step reads grad * grad_scale (data parallel: the all-reduced SUM x 1 / world, in the load)."""
    lib = L.load()
    if grad_scale == 1.0:
        L.check(lib.dm_adam_counted(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), param.numel(), lr, beta1, beta2, eps,
                                    _ptr(steps_done), _ptr(steps_done_next), _stream()), "dm_adam_counted")
    else:
        L.check(lib.dm_adam_counted_scaled(_ptr(param), _ptr(grad), _ptr(m), _ptr(v), param.numel(), lr, beta1, beta2, eps,
                                           float(grad_scale), _ptr(steps_done), _ptr(steps_done_next), _stream()),
                "dm_adam_counted_scaled")


@_op
def zscore_channels(x, channel_mean, channel_std, out=None):
    """float32(zscore(x, channel_mean, channel_std)) of pipeline/train_utils.py:228-250 for an (N, C, H, W) float64 or
    float32 DEVICE tensor and GIVEN per-channel statistics (lists of Python floats, as the reference's config supplies them,
    or numpy scalars / arrays): bit-equal to the numpy expression followed by .astype(np.float32) -- the type numpy would
    compute in and the value of std + eps are worked out on the host with numpy itself."""
    import numpy as np
    lib = L.load()
    if x.dtype not in (torch.float64, torch.float32):
        raise ValueError("dm_zscore_channels: float64 or float32 input")
    x = x.contiguous()
    N, Cn, H, W = x.shape
    if len(channel_mean) != Cn or len(channel_std) != Cn:
        raise ValueError("dm_zscore_channels: one mean and one std per channel")
    np_dt = np.float64 if x.dtype == torch.float64 else np.float32
    mean, denom = np.empty(Cn), np.empty(Cn)
    dts, qts = set(), set()
    for c in range(Cn):
        diff = np.zeros(1, np_dt) - channel_mean[c]              # numpy's own promotion rules decide the types
        den = channel_std[c] + np.finfo(float).eps                # (the reference's expression: a float64 scalar)
        quot = diff / den
        dts.add(diff.dtype); qts.add(quot.dtype)
        mean[c] = float(np.asarray(channel_mean[c]).astype(diff.dtype))      # the scalars as the array operations see them
        denom[c] = float(np.asarray(den).astype(quot.dtype))
    if len(dts) != 1 or len(qts) != 1 or not dts <= {np.dtype(np.float32), np.dtype(np.float64)}:
        raise ValueError("dm_zscore_channels: statistics of mixed / unsupported types")
    diff_f64, quot_f64 = dts.pop() == np.float64, qts.pop() == np.float64
    md = torch.from_numpy(np.stack([mean, denom])).to(x.device)
    if out is None:
        out = torch.empty((N, Cn, H, W), dtype=torch.float32, device=x.device)
    L.check(lib.dm_zscore_channels(C.c_void_p(x.data_ptr()), 1 if x.dtype == torch.float64 else 0, 1 if diff_f64 else 0,
                                   1 if quot_f64 else 0, _ptr(out), C.c_void_p(md[0].data_ptr()), C.c_void_p(md[1].data_ptr()),
                                   N, Cn, H * W, _stream()), "dm_zscore_channels")
    return out


@_op
def zscore_patch(x):
    """x (N, C, H, W) float64 or float32 device tensor -> float32 z-scored patches (per patch and channel)."""
    lib = L.load()
    if x.dtype not in (torch.float64, torch.float32):
        raise ValueError("dm_zscore_patch: float64 or float32 input")
    x = x.contiguous()
    N, Cn, H, W = x.shape
    out = torch.empty((N, Cn, H, W), device=x.device, dtype=torch.float32)
    L.call_device.index = x.device.index
    L.check(lib.dm_zscore_patch(C.c_void_p(x.data_ptr()), 1 if x.dtype == torch.float64 else 0, _ptr(out), N * Cn, H * W,
                                _stream()), "dm_zscore_patch")
    return out


@_op
def augment(x, flip_code, rot_code):
    lib = L.load()
    B, Cn, H, W = x.shape
    if H != W:
        raise ValueError("dm_augment: square patches only")
    out = torch.empty_like(x)
    L.check(lib.dm_augment(_ptr(x), _ptr(out), _ptr(flip_code, torch.int32), _ptr(rot_code, torch.int32), B, Cn, H,
                           _stream()), "dm_augment")
    return out


# ----------------------------------------------------------------------------- feeding the step (csrc/feed.hip)
@_op
def gather_augment(src, ids, flip_code, rot_code, out, n=None):
    """out[:n] = rot90(flip(src[ids], flip), rot) (run_training.py:512 + :396-403) in one launch.  src (N, C, H, H) fp32
    in HBM, ids / codes int32 device vectors (None: the first n samples in order / no augmentation); `out` is written in
    place (the captured step's input buffer) and returned."""
    lib = L.load()
    N, Cn, H, W = src.shape
    if H != W:
        raise ValueError("dm_gather_augment: square patches only")
    n = int(n if n is not None else (ids.numel() if ids is not None else out.shape[0]))
    if out.shape[0] < n or tuple(out.shape[1:]) != (Cn, H, W):
        raise ValueError(f"dm_gather_augment: out {tuple(out.shape)} does not hold {n} x {(Cn, H, W)}")
    for t in (ids, flip_code, rot_code):
        if t is not None and t.numel() < n:
            raise ValueError("dm_gather_augment: fewer ids / codes than samples")
    L.check(lib.dm_gather_augment(_ptr(src), N, _ptr(ids, torch.int32), _ptr(flip_code, torch.int32),
                                  _ptr(rot_code, torch.int32), _ptr(out), n, Cn, H, _stream()), "dm_gather_augment")
    return out


@_op
def gather_rows(src, ids, out, n=None):
    """out[:n] = src[ids] for (N, ...) fp32 rows (the mask planes of a batch, run_training.py:371)."""
    lib = L.load()
    row = src[0].numel()
    n = int(n if n is not None else (ids.numel() if ids is not None else out.shape[0]))
    if out.shape[0] < n or out[0].numel() != row:
        raise ValueError("dm_gather_rows: out does not hold n rows of the source's size")
    if ids is not None and ids.numel() < n:
        raise ValueError("dm_gather_rows: fewer ids than rows")
    L.check(lib.dm_gather_rows(_ptr(src), src.shape[0], _ptr(ids, torch.int32), _ptr(out), n, row, _stream()),
            "dm_gather_rows")
    return out


@_op
def csr_block(indptr, indices, data, n, ids, pos, stamp, out):
    """out (B, B) = relation_mat[ids, :][:, ids].todense() (run_training.py:348-351) from CSR arrays in HBM."""
    lib = L.load()
    B = ids.numel()
    if tuple(out.shape) != (B, B) or pos.numel() < n or indptr.numel() != n + 1:
        raise ValueError("dm_csr_block: shapes do not match")
    if indices.numel() == 0:                      # an empty matrix: scipy hands over zero-length arrays (no pointer)
        out.zero_()
        return out
    L.check(lib.dm_csr_block(_ptr(indptr, torch.int64), _ptr(indices, torch.int32), _ptr(data), n, _ptr(ids, torch.int32),
                             B, _ptr(pos, torch.int64), int(stamp), _ptr(out), _stream()), "dm_csr_block")
    return out


def augment_codes(n):
    """(flip, rot) int32 numpy arrays for n samples, drawn from numpy's GLOBAL legacy generator exactly as the
    reference's per-sample loop draws them (run_training.py:399-402: choice([0,1,2]) then choice([0,1,2,3]), interleaved)
    -- a caller's np.random.seed reproduces the reference's augmentation -- without 2n Python-level draws: the
    generator's 32-bit words are drawn in one block, parsed by dm_augment_codes (host C), and the generator is left
    where the n interleaved calls would have left it."""
    import numpy as np
    lib = L.load()
    flip = np.empty(n, np.int32)
    rot = np.empty(n, np.int32)
    if n == 0:
        return flip, rot
    state = np.random.get_state()
    m = 3 * n + 64                                 # expected 2.33 words per sample; retried (doubling) if short
    while True:
        raw = np.random.randint(0, 2 ** 32, size=m, dtype=np.uint32)
        used = lib.dm_augment_codes(raw.ctypes.data, m, n, flip.ctypes.data, rot.ctypes.data)
        np.random.set_state(state)
        if used >= 0:
            break
        m *= 2
    np.random.randint(0, 2 ** 32, size=int(used), dtype=np.uint32)      # advance by exactly the words consumed
    return flip, rot


# ----------------------------------------------------------------------------- latent PCA (run_dim_reduction.py)
def _rows(X):
    """A 2-D fp32 device matrix with unit column stride: (pointer, N, F, leading dimension)."""
    if not X.is_cuda:
        raise ValueError("dynamorph_amd: tensor is not on the GPU (the HIP path has no CPU fallback)")
    if X.dtype != torch.float32 or X.dim() != 2:
        raise ValueError(f"dynamorph_amd: expected a 2-D float32 matrix, got {X.dtype} of shape {tuple(X.shape)}")
    if X.shape[1] > 1 and X.stride(1) != 1:
        raise ValueError("dynamorph_amd: the matrix needs unit column stride")
    _note_device(X.device.index)
    return X.data_ptr(), X.shape[0], X.shape[1], max(X.stride(0), X.shape[1])


def _pca_workspace(nbytes, like):
    return torch.empty(max(int(nbytes), 8) // 8, device=like.device, dtype=torch.float64)


@_op
def pca_colsum(X, sums=None, workspace=None):
    """sums (F,) float64 = X.sum(0) in a fixed order (dm_pca_colsum)."""
    lib = L.load()
    p, N, F, ld = _rows(X)
    nbytes = lib.dm_pca_colsum_workspace_bytes(N, F)
    if nbytes < 0:
        raise ValueError(f"dm_pca_colsum: bad shape ({N}, {F})")
    if sums is None:
        sums = _new((F,), X, torch.float64)
    if workspace is None or workspace.numel() * 8 < nbytes:
        workspace = _pca_workspace(nbytes, X)
    L.check(lib.dm_pca_colsum(p, N, F, ld, _ptr(sums, torch.float64), _ptr(workspace, torch.float64), workspace.numel() * 8,
                              _stream()), "dm_pca_colsum")
    return sums


@_op
def pca_gram(X, shift=None, G=None, accumulate=False, workspace=None):
    """G (F, F) float64 (+)= (X - shift)^T (X - shift) (dm_pca_gram); shift (F,) fp32 or None."""
    lib = L.load()
    p, N, F, ld = _rows(X)
    nbytes = lib.dm_pca_gram_workspace_bytes(N, F)
    if nbytes < 0:
        raise ValueError(f"dm_pca_gram: bad shape ({N}, {F})")
    if shift is not None and shift.numel() != F:
        raise ValueError(f"dm_pca_gram: shift has {shift.numel()} entries, F = {F}")
    if G is None:
        if accumulate:
            raise ValueError("dm_pca_gram: accumulate needs G")
        G = _new((F, F), X, torch.float64)
    elif tuple(G.shape) != (F, F):
        raise ValueError(f"dm_pca_gram: G has shape {tuple(G.shape)}, need ({F}, {F})")
    if workspace is None or workspace.numel() * 8 < nbytes:
        workspace = _pca_workspace(nbytes, X)
    L.check(lib.dm_pca_gram(p, N, F, ld, _ptr(shift), _ptr(G, torch.float64), 1 if accumulate else 0,
                            _ptr(workspace, torch.float64), workspace.numel() * 8, _stream()), "dm_pca_gram")
    return G


@_op
def pca_transform(X, V, shift=None, out=None):
    """Y (N, k) fp32 = (X - shift) V^T (dm_pca_transform); V (k, F) fp32."""
    lib = L.load()
    p, N, F, ld = _rows(X)
    if V.dim() != 2 or V.shape[1] != F:
        raise ValueError(f"dm_pca_transform: V has shape {tuple(V.shape)}, need (k, {F})")
    if shift is not None and shift.numel() != F:
        raise ValueError(f"dm_pca_transform: shift has {shift.numel()} entries, F = {F}")
    k = V.shape[0]
    if out is None:
        out = _new((N, k), X)
    elif tuple(out.shape) != (N, k):
        raise ValueError(f"dm_pca_transform: out has shape {tuple(out.shape)}, need ({N}, {k})")
    L.check(lib.dm_pca_transform(p, N, F, ld, _ptr(shift), _ptr(V), k, _ptr(out), _stream()), "dm_pca_transform")
    return out


@_op
def pca_rowgram(X, shift=None, K=None, accumulate=False, workspace=None):
    """K (N, N) float64 (+)= (X - shift)(X - shift)^T (dm_pca_rowgram); shift (F,) fp32 or None."""
    lib = L.load()
    p, N, F, ld = _rows(X)
    nbytes = lib.dm_pca_rowgram_workspace_bytes(N, F)
    if nbytes < 0:
        raise ValueError(f"dm_pca_rowgram: bad shape ({N}, {F})")
    if shift is not None and shift.numel() != F:
        raise ValueError(f"dm_pca_rowgram: shift has {shift.numel()} entries, F = {F}")
    if K is None:
        if accumulate:
            raise ValueError("dm_pca_rowgram: accumulate needs K")
        K = _new((N, N), X, torch.float64)
    elif tuple(K.shape) != (N, N) or not K.is_contiguous():
        raise ValueError(f"dm_pca_rowgram: K has shape {tuple(K.shape)}, need a contiguous ({N}, {N})")
    if workspace is None or workspace.numel() * 8 < nbytes:
        workspace = _pca_workspace(nbytes, X)
    L.check(lib.dm_pca_rowgram(p, N, F, ld, _ptr(shift), _ptr(K, torch.float64), 1 if accumulate else 0,
                               _ptr(workspace, torch.float64), workspace.numel() * 8, _stream()), "dm_pca_rowgram")
    return K


@_op
def pca_components(X, W, shift=None, out=None):
    """V (k, F) float64 = W (X - shift) (dm_pca_components); W (k, N) fp32."""
    lib = L.load()
    p, N, F, ld = _rows(X)
    if W.dim() != 2 or W.shape[1] != N:
        raise ValueError(f"dm_pca_components: W has shape {tuple(W.shape)}, need (k, {N})")
    if shift is not None and shift.numel() != F:
        raise ValueError(f"dm_pca_components: shift has {shift.numel()} entries, F = {F}")
    k = W.shape[0]
    if out is None:
        out = _new((k, F), X, torch.float64)
    elif tuple(out.shape) != (k, F) or not out.is_contiguous():
        raise ValueError(f"dm_pca_components: out has shape {tuple(out.shape)}, need a contiguous ({k}, {F})")
    L.check(lib.dm_pca_components(p, N, F, ld, _ptr(shift), _ptr(W), k, _ptr(out, torch.float64), _stream()),
            "dm_pca_components")
    return out


# ----------------------------------------------------------------------------- exact k-NN graph of the latents
KNN_MAX_K = 256                # DM_KNN_MAX_K
KNN_MAX_SLACK = 256            # DM_KNN_MAX_SLACK
KNN_DEFAULT_SLACK = 64


def knn_workspace(R, M, F, k, slack, like):
    """A workspace dm_knn accepts for panels of up to R queries (uint8, 256-byte aligned by the allocator)."""
    nbytes = L.load().dm_knn_workspace_bytes(R, M, F, k, slack)
    if nbytes < 0:
        raise ValueError(f"dm_knn: bad shape R = {R}, M = {M}, F = {F}, k = {k}, slack = {slack}")
    return torch.empty(int(nbytes), device=like.device, dtype=torch.uint8)


@_op
def knn(X, Q=None, k=15, rows=None, shift=None, slack=None, include_self=False, out=None, workspace=None):
    """The k nearest rows of X (M, F) for every query, exact with respect to the fp32-difference / float64-sum distance
    (dm_knn): (indices (R, k) int32, distances (R, k) fp32 sorted by (distance, index), n_fallback_rows (1,) int32 on the
    device).  Queries: Q (R, F), or Q=None -- the rows of X itself, all of them or rows=(r0, R), each row excluded from its
    own list by index (include_self=True: column 0 is the row itself at distance 0.0, umap-learn's layout).  shift (F,) fp32:
    subtracted in the filter's operand load (the results do not depend on it); slack: extra candidates the filter keeps
    (0 .. 256, the results do not depend on it either; 0 sends nearly every row of uncentred data through the fallback)."""
    lib = L.load()
    px, M, F, ldx = _rows(X)
    if Q is not None:
        if rows is not None or include_self:
            raise ValueError("dm_knn: rows= and include_self belong to the self form (Q=None)")
        pq, R, Fq, ldq = _rows(Q)
        if Fq != F:
            raise ValueError(f"dm_knn: Q has {Fq} features, X has {F}")
        r0 = -1
    else:
        r0, R = (0, M) if rows is None else (int(rows[0]), int(rows[1]))
        if r0 < 0 or R < 1 or r0 + R > M:
            raise ValueError(f"dm_knn: rows=({r0}, {R}) lie outside X with {M} rows")
        pq, ldq = None, 0
    k = int(k)
    if k < 1 or k > KNN_MAX_K:
        raise ValueError(f"dm_knn: k outside 1 .. {KNN_MAX_K}, got {k}")
    slack = KNN_DEFAULT_SLACK if slack is None else int(slack)
    if shift is not None and shift.numel() != F:
        raise ValueError(f"dm_knn: shift has {shift.numel()} entries, F = {F}")
    if out is None:
        idx, dist = _new((R, k), X, torch.int32), _new((R, k), X)
    else:
        idx, dist = out
        if tuple(idx.shape) != (R, k) or tuple(dist.shape) != (R, k):
            raise ValueError(f"dm_knn: out has shapes {tuple(idx.shape)}, {tuple(dist.shape)}, need ({R}, {k}) twice")
    nfb = _new((1,), X, torch.int32)
    nbytes = lib.dm_knn_workspace_bytes(R, M, F, k, slack)
    if nbytes >= 0 and (workspace is None or workspace.numel() * workspace.element_size() < nbytes):
        workspace = torch.empty(int(nbytes), device=X.device, dtype=torch.uint8)
    if workspace is None:       # a bad shape: dm_knn names it (nothing is launched)
        workspace = torch.empty(256, device=X.device, dtype=torch.uint8)
    L.check(lib.dm_knn(px, M, F, ldx, pq, R, ldq, r0, k, slack, 1 if include_self else 0, _ptr(shift), _ptr(idx, torch.int32),
                       _ptr(dist), _ptr(nfb, torch.int32), _ptr(workspace, workspace.dtype),
                       workspace.numel() * workspace.element_size(), _stream()), "dm_knn")
    return idx, dist, nfb


KNN_WIDE_MAX_FEATURES = 1 << 20    # DM_KNN_WIDE_MAX_FEATURES
KNN_WIDE_MAX_ROWS = 24576          # DM_PCA_WIDE_MAX_SAMPLES


def _knn_out(out, R, k, X, who):
    if out is None:
        return _new((R, k), X, torch.int32), _new((R, k), X)
    idx, dist = out
    if tuple(idx.shape) != (R, k) or tuple(dist.shape) != (R, k):
        raise ValueError(f"{who}: out has shapes {tuple(idx.shape)}, {tuple(dist.shape)}, need ({R}, {k}) twice")
    return idx, dist


def _knn_ws(nbytes, workspace, X):
    if nbytes >= 0 and (workspace is None or workspace.numel() * workspace.element_size() < nbytes):
        workspace = torch.empty(int(nbytes), device=X.device, dtype=torch.uint8)
    if workspace is None:       # a bad shape: the entry names it (nothing is launched)
        workspace = torch.empty(256, device=X.device, dtype=torch.uint8)
    return workspace


@_op
def knn_wide(X, Q, k=15, shift=None, slack=None, out=None, workspace=None):
    """knn(X, Q) for 1 .. 2^20 features and at most 24576 rows of X (dm_knn_wide): the same launches, the wide feature cap."""
    lib = L.load()
    px, M, F, ldx = _rows(X)
    pq, R, Fq, ldq = _rows(Q)
    if Fq != F:
        raise ValueError(f"dm_knn_wide: Q has {Fq} features, X has {F}")
    k = int(k)
    slack = KNN_DEFAULT_SLACK if slack is None else int(slack)
    if shift is not None and shift.numel() != F:
        raise ValueError(f"dm_knn_wide: shift has {shift.numel()} entries, F = {F}")
    idx, dist = _knn_out(out, R, k, X, "dm_knn_wide")
    nfb = _new((1,), X, torch.int32)
    workspace = _knn_ws(lib.dm_knn_wide_workspace_bytes(R, M, F, k, slack), workspace, X)
    L.check(lib.dm_knn_wide(px, M, F, ldx, pq, R, ldq, k, slack, _ptr(shift), _ptr(idx, torch.int32), _ptr(dist),
                            _ptr(nfb, torch.int32), _ptr(workspace, workspace.dtype),
                            workspace.numel() * workspace.element_size(), _stream()), "dm_knn_wide")
    return idx, dist, nfb


@_op
def knn_wide_self(X, K, k=15, shift=None, slack=None, include_self=False, pair_once=True, out=None, workspace=None):
    """The whole k-NN graph of X (N <= 24576 rows, 1 .. 2^20 features) from its row Gram matrix K = pca_rowgram(X, shift)
    (dm_knn_wide_self; the SAME shift, or None for both): (indices (N, k) int32, distances (N, k) fp32, n_fallback_rows (1,)
    int32, n_pairs (1,) int32 -- the exact pair evaluations of the pair-once refine -- on the device)."""
    lib = L.load()
    px, N, F, ldx = _rows(X)
    if K.dtype != torch.float64 or tuple(K.shape) != (N, N) or not K.is_contiguous():
        raise ValueError(f"dm_knn_wide_self: K has shape {tuple(K.shape)} and dtype {K.dtype}, need a contiguous float64 "
                         f"({N}, {N})")
    k = int(k)
    slack = KNN_DEFAULT_SLACK if slack is None else int(slack)
    if shift is not None and shift.numel() != F:
        raise ValueError(f"dm_knn_wide_self: shift has {shift.numel()} entries, F = {F}")
    idx, dist = _knn_out(out, N, k, X, "dm_knn_wide_self")
    nfb, npairs = _new((1,), X, torch.int32), _new((1,), X, torch.int32)
    workspace = _knn_ws(lib.dm_knn_wide_self_workspace_bytes(N, F, k, slack), workspace, X)
    L.check(lib.dm_knn_wide_self(px, N, F, ldx, _ptr(shift), _ptr(K, torch.float64), k, slack, 1 if include_self else 0,
                                 1 if pair_once else 0, _ptr(idx, torch.int32), _ptr(dist), _ptr(nfb, torch.int32),
                                 _ptr(npairs, torch.int32), _ptr(workspace, workspace.dtype),
                                 workspace.numel() * workspace.element_size(), _stream()), "dm_knn_wide_self")
    return idx, dist, nfb, npairs


def knn_ranks_default_cap(c, M):
    """Entries of a row's list of undecided columns.  Unstructured Gaussian rows at M = 100 000, F = 4096 put
    about 110 columns per target inside the filter's window, and the number grows with the density of rows, that is with M:
    c M / 480 holds twice that.  Structured data need less than one column per target beside the target itself: 4 c + 64
    at least.  At most 32768 (4 bytes each, per row of a panel); dm_knn_ranks clips it to M.  A row that needs more is
    redone exactly, so the choice moves time, never a result."""
    c, M = int(c), int(M)
    return min(32768, max(4 * c + 64, c * M // 480))


@_op
def knn_ranks(X, targets, rows=None, shift=None, cap=None, out=None, workspace=None):
    """Ranks of the given target rows among each row's neighbours in X (M, F) (dm_knn_ranks): targets (R, c) int32 on the
    device for the rows rows=(r0, R) (default all) -> (ranks (R, c) int32, n_ambiguous (1,) int32, n_redone (1,) int32 on the
    device).  rank = 1 + the number of other rows that are nearer by (exact-form fp32 distance, index); 0 for the row itself.
    The targets must lie in 0 .. M - 1 (the caller checks: nothing is read back here)."""
    lib = L.load()
    px, M, F, ldx = _rows(X)
    r0, R = (0, M) if rows is None else (int(rows[0]), int(rows[1]))
    if r0 < 0 or R < 1 or r0 + R > M:
        raise ValueError(f"dm_knn_ranks: rows=({r0}, {R}) lie outside X with {M} rows")
    if targets.dim() != 2 or targets.shape[0] != R or targets.dtype != torch.int32 or not targets.is_contiguous():
        raise ValueError(f"dm_knn_ranks: targets has shape {tuple(targets.shape)} and dtype {targets.dtype}, need a contiguous "
                         f"int32 ({R}, c)")
    c = int(targets.shape[1])
    if c < 1 or c > KNN_MAX_K:
        raise ValueError(f"dm_knn_ranks: c outside 1 .. {KNN_MAX_K}, got {c}")
    if shift is not None and shift.numel() != F:
        raise ValueError(f"dm_knn_ranks: shift has {shift.numel()} entries, F = {F}")
    cap = knn_ranks_default_cap(c, M) if cap is None else int(cap)
    if out is None:
        out = _new((R, c), X, torch.int32)
    elif tuple(out.shape) != (R, c) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError(f"dm_knn_ranks: out has shape {tuple(out.shape)}, need a contiguous int32 ({R}, {c})")
    namb, nredo = _new((1,), X, torch.int32), _new((1,), X, torch.int32)
    workspace = _knn_ws(lib.dm_knn_ranks_workspace_bytes(R, M, F, c, cap), workspace, X)
    L.check(lib.dm_knn_ranks(px, M, F, ldx, r0, R, _ptr(targets, torch.int32), c, _ptr(shift), cap, _ptr(out, torch.int32),
                             _ptr(namb, torch.int32), _ptr(nredo, torch.int32), _ptr(workspace, workspace.dtype),
                             workspace.numel() * workspace.element_size(), _stream()), "dm_knn_ranks")
    return out, namb, nredo


# ----------------------------------------------------------------------------- exact k-means of the latents
KMEANS_MAX_CLUSTERS = 1024     # DM_KMEANS_MAX_CLUSTERS


def kmeans_workspace(N, F, K, like):
    """A workspace dm_kmeans_assign and dm_kmeans_sums accept for the shape (uint8, 256-byte aligned by the allocator)."""
    nbytes = L.load().dm_kmeans_workspace_bytes(N, F, K)
    if nbytes < 0:
        raise ValueError(f"dm_kmeans: bad shape N = {N}, F = {F}, K = {K}")
    return torch.empty(max(int(nbytes), 256), device=like.device, dtype=torch.uint8)


def _kmeans_centres(C, F, who):
    if C.dim() != 2 or C.shape[1] != F:
        raise ValueError(f"{who}: C has shape {tuple(C.shape)}, need (K, {F})")
    return C.shape[0]


@_op
def kmeans_assign(X, C, shift=None, labels=None, dist=None, want_dist=True, workspace=None):
    """Per row of X (N, F) the centre of C (K, F) of smallest (exact-form fp32 distance, index) (dm_kmeans_assign): (labels (N,)
    int32, distances (N,) fp32 or None, rechecked rows (1,) int32 on the device).  shift (F,) fp32: subtracted in the
    filter's operand load; the results do not depend on it."""
    lib = L.load()
    px, N, F, ldx = _rows(X)
    K = _kmeans_centres(C, F, "dm_kmeans_assign")
    if shift is not None and shift.numel() != F:
        raise ValueError(f"dm_kmeans_assign: shift has {shift.numel()} entries, F = {F}")
    if labels is None:
        labels = _new((N,), X, torch.int32)
    elif tuple(labels.shape) != (N,):
        raise ValueError(f"dm_kmeans_assign: labels has shape {tuple(labels.shape)}, need ({N},)")
    if dist is None and want_dist:
        dist = _new((N,), X)
    elif dist is not None and tuple(dist.shape) != (N,):
        raise ValueError(f"dm_kmeans_assign: dist has shape {tuple(dist.shape)}, need ({N},)")
    n = _new((1,), X, torch.int32)
    workspace = _knn_ws(lib.dm_kmeans_workspace_bytes(N, F, K), workspace, X)
    L.check(lib.dm_kmeans_assign(px, N, F, ldx, _ptr(C), K, _ptr(shift), _ptr(labels, torch.int32), _ptr(dist),
                                 _ptr(n, torch.int32), _ptr(workspace, workspace.dtype),
                                 workspace.numel() * workspace.element_size(), _stream()), "dm_kmeans_assign")
    return labels, dist, n


@_op
def kmeans_sums(X, labels, K, sums=None, counts=None, workspace=None):
    """(sums (K, F) float64, counts (K,) int64) of the rows of X by label, in an order fixed by the shape and the labels
    (dm_kmeans_sums)."""
    lib = L.load()
    px, N, F, ldx = _rows(X)
    K = int(K)
    if tuple(labels.shape) != (N,):
        raise ValueError(f"dm_kmeans_sums: labels has shape {tuple(labels.shape)}, need ({N},)")
    if sums is None:
        sums = _new((max(K, 0), F), X, torch.float64)
    elif tuple(sums.shape) != (K, F):
        raise ValueError(f"dm_kmeans_sums: sums has shape {tuple(sums.shape)}, need ({K}, {F})")
    if counts is None:
        counts = _new((max(K, 0),), X, torch.int64)
    elif tuple(counts.shape) != (K,):
        raise ValueError(f"dm_kmeans_sums: counts has shape {tuple(counts.shape)}, need ({K},)")
    workspace = _knn_ws(lib.dm_kmeans_workspace_bytes(N, F, K), workspace, X)
    L.check(lib.dm_kmeans_sums(px, N, F, ldx, _ptr(labels, torch.int32), K, _ptr(sums, torch.float64),
                               _ptr(counts, torch.int64), _ptr(workspace, workspace.dtype),
                               workspace.numel() * workspace.element_size(), _stream()), "dm_kmeans_sums")
    return sums, counts


@_op
def kmeans_row_d2(X, C, labels=None, out=None):
    """d2 (N,) float64: the exact-form squared distance of every row to centre labels[row] of C, or to row 0 of C when labels
    is None (dm_kmeans_row_d2)."""
    lib = L.load()
    px, N, F, ldx = _rows(X)
    K = _kmeans_centres(C, F, "dm_kmeans_row_d2")
    if labels is not None and tuple(labels.shape) != (N,):
        raise ValueError(f"dm_kmeans_row_d2: labels has shape {tuple(labels.shape)}, need ({N},)")
    if out is None:
        out = _new((N,), X, torch.float64)
    elif tuple(out.shape) != (N,):
        raise ValueError(f"dm_kmeans_row_d2: out has shape {tuple(out.shape)}, need ({N},)")
    L.check(lib.dm_kmeans_row_d2(px, N, F, ldx, _ptr(C), K, _ptr(labels, torch.int32), _ptr(out, torch.float64), _stream()),
            "dm_kmeans_row_d2")
    return out


# ----------------------------------------------------------------------------- Y = A Q of the partial eigensolver
EIG_MAX_BLOCK = 256            # DM_EIG_MAX_BLOCK


def _rows64(X, who):
    """A 2-D float64 device matrix with unit column stride: (pointer, rows, columns, leading dimension)."""
    if not X.is_cuda:
        raise ValueError("dynamorph_amd: tensor is not on the GPU (the HIP path has no CPU fallback)")
    if X.dtype != torch.float64 or X.dim() != 2:
        raise ValueError(f"{who}: expected a 2-D float64 matrix, got {X.dtype} of shape {tuple(X.shape)}")
    if X.shape[1] > 1 and X.stride(1) != 1:
        raise ValueError(f"{who}: the matrix needs unit column stride")
    if X.shape[0] > 1 and X.stride(0) < X.shape[1]:
        raise ValueError(f"{who}: the rows of the matrix overlap")
    _note_device(X.device.index)
    return X.data_ptr(), X.shape[0], X.shape[1], max(X.stride(0), X.shape[1]) if X.shape[0] > 1 else X.shape[1]


def eig_workspace(n, b, like):
    """A workspace dm_eig_apply accepts for the shape (uint8, 256-byte aligned by the allocator)."""
    nbytes = L.load().dm_eig_apply_workspace_bytes(n, b)
    if nbytes < 0:
        raise ValueError(f"dm_eig_apply: bad shape n = {n}, b = {b}")
    return torch.empty(int(nbytes), device=like.device, dtype=torch.uint8)


def eig_plan(n, b):
    """(row_tiles, splits, tile_rows, stage) of dm_eig_apply for the shape (dm_eig_apply_plan; host only)."""
    out = [C.c_int(0) for _ in range(4)]
    L.check(L.load().dm_eig_apply_plan(n, b, *[C.addressof(o) for o in out]), "dm_eig_apply_plan")
    return tuple(o.value for o in out)


@_op
def eig_apply(A, Q, out=None, workspace=None):
    """Y (n, b) float64 = A Q (dm_eig_apply): A (n, n) and Q (n, b) float64 with unit column stride (row views are taken as
    they lie), b a multiple of 16 in 16 .. 256.  A is not assumed symmetric."""
    lib = L.load()
    pa, n, na, lda = _rows64(A, "dm_eig_apply")
    if na != n:
        raise ValueError(f"dm_eig_apply: A has shape {tuple(A.shape)}, need a square matrix")
    pq, nq, b, ldq = _rows64(Q, "dm_eig_apply")
    if nq != n:
        raise ValueError(f"dm_eig_apply: Q has shape {tuple(Q.shape)}, A has {n} rows")
    if out is None:
        out = _new((n, b), A, torch.float64)
    py, ny, by, ldy = _rows64(out, "dm_eig_apply")
    if (ny, by) != (n, b):
        raise ValueError(f"dm_eig_apply: out has shape {tuple(out.shape)}, need ({n}, {b})")
    workspace = _knn_ws(lib.dm_eig_apply_workspace_bytes(n, b), workspace, A)
    L.check(lib.dm_eig_apply(pa, n, lda, pq, b, ldq, py, ldy, _ptr(workspace, workspace.dtype),
                             workspace.numel() * workspace.element_size(), _stream()), "dm_eig_apply")
    return out


# ----------------------------------------------------------------------------- UMAP behind the k-NN graph
UMAP_MAX_K = 256               # DM_UMAP_MAX_K


def _umap_graph(dists, indices=None):
    if dists.dim() != 2 or (indices is not None and tuple(indices.shape) != tuple(dists.shape)):
        raise ValueError("dm_umap: knn_dists must be (N, k) and knn_indices of the same shape")
    N, k = dists.shape
    if k < 2 or k > UMAP_MAX_K or k > N:
        raise ValueError(f"dm_umap: k = {k} outside 2 .. min({UMAP_MAX_K}, N = {N})")
    return N, k


@_op
def umap_smooth(dists):
    """(rho (N,) fp32, sigma (N,) fp32, row_mean (N,) float64, global_mean (1,) float64) of the (N, k) fp32 distances of a
    k-NN graph with the row itself in column 0 (dm_umap_smooth)."""
    N, k = _umap_graph(dists)
    rho, sigma = _new((N,), dists), _new((N,), dists)
    row_mean, global_mean = _new((N,), dists, torch.float64), _new((1,), dists, torch.float64)
    L.check(L.load().dm_umap_smooth(_ptr(dists), N, k, _ptr(rho), _ptr(sigma), _ptr(row_mean, torch.float64),
                                    _ptr(global_mean, torch.float64), _stream()), "dm_umap_smooth")
    return rho, sigma, row_mean, global_mean


@_op
def umap_membership(indices, dists, rho, sigma):
    """The (N, k) fp32 membership strengths of the directed graph (dm_umap_membership); indices int32."""
    N, k = _umap_graph(dists, indices)
    if rho.numel() != N or sigma.numel() != N:
        raise ValueError(f"dm_umap_membership: rho / sigma need {N} entries")
    out = _new((N, k), dists)
    L.check(L.load().dm_umap_membership(_ptr(indices, torch.int32), _ptr(dists), N, k, _ptr(rho), _ptr(sigma), _ptr(out),
                                        _stream()), "dm_umap_membership")
    return out


@_op
def umap_epoch(indptr, cols, eps, eps_neg, nxt, nxt_neg, y_in, y_out, epoch, n_epochs, a, b, gamma, seed, group=0):
    """One epoch of the layout (dm_umap_epoch): y_out from y_in, the schedule state nxt / nxt_neg advanced in place.  The
    columns must lie in [0, N): the caller has checked them."""
    N, nnz = indptr.numel() - 1, cols.numel()
    if tuple(y_in.shape) != (N, 2) or tuple(y_out.shape) != (N, 2):
        raise ValueError(f"dm_umap_epoch: y_in / y_out must be ({N}, 2)")
    if not (eps.numel() == eps_neg.numel() == nxt.numel() == nxt_neg.numel() == nnz):
        raise ValueError(f"dm_umap_epoch: eps / eps_neg / next / next_neg need {nnz} entries")
    L.check(L.load().dm_umap_epoch(_ptr(indptr, torch.int64), _ptr(cols, torch.int32), N, nnz, _ptr(eps), _ptr(eps_neg),
                                   _ptr(nxt), _ptr(nxt_neg), _ptr(y_in), _ptr(y_out), int(epoch), int(n_epochs), float(a),
                                   float(b), float(gamma), int(seed) & 0xFFFFFFFFFFFFFFFF, int(group), _stream()),
            "dm_umap_epoch")
    return y_out


# ----------------------------------------------------------------------------- UMAP transform of new points
def _umap_query_graph(indices, dists, y_train):
    if dists.dim() != 2 or tuple(indices.shape) != tuple(dists.shape):
        raise ValueError("dm_umap_transform: knn_dists must be (R, k) and knn_indices of the same shape")
    if y_train.dim() != 2 or y_train.shape[1] != 2:
        raise ValueError(f"dm_umap_transform: y_train must be (M, 2), got {tuple(y_train.shape)}")
    R, k = dists.shape
    M = y_train.shape[0]
    if R < 1 or k < 2 or k > UMAP_MAX_K or k > M:
        raise ValueError(f"dm_umap_transform: R = {R}, k = {k} outside 2 .. min({UMAP_MAX_K}, M = {M})")
    return R, k, M


@_op
def umap_transform_prepare(indices, dists, y_train, n_epochs, negative_sample_rate=5):
    """(sigma (R,), membership (R, k), eps, eps_neg, next, next_neg (R, k), y0 (R, 2)), all fp32, of the (R, k) query graph
    (indices int32 into the M training rows, fp32 distances, rows sorted) against the fitted embedding y_train (M, 2)
    (dm_umap_transform_prepare).  The indices must lie in [0, M): the caller has checked them."""
    R, k, M = _umap_query_graph(indices, dists, y_train)
    sigma, y0 = _new((R,), dists), _new((R, 2), dists)
    memb, eps, eps_neg, nxt, nxt_neg = (_new((R, k), dists) for _ in range(5))
    L.check(L.load().dm_umap_transform_prepare(_ptr(indices, torch.int32), _ptr(dists), R, k, M, _ptr(y_train), int(n_epochs),
                                               int(negative_sample_rate), _ptr(sigma), _ptr(memb), _ptr(eps), _ptr(eps_neg),
                                               _ptr(nxt), _ptr(nxt_neg), _ptr(y0), _stream()), "dm_umap_transform_prepare")
    return sigma, memb, eps, eps_neg, nxt, nxt_neg, y0


@_op
def umap_transform_layout(indices, eps, eps_neg, nxt, nxt_neg, y_train, y, epoch_begin, epoch_end, n_epochs, row_offset, seed,
                          a, b, gamma, group=0):
    """Epochs [epoch_begin, epoch_end) of the transform's layout in one launch (dm_umap_transform_layout): y (R, 2) and the
    schedule state nxt / nxt_neg (R, k) advanced in place.  The indices must lie in [0, M): the caller has checked them."""
    R, k, M = _umap_query_graph(indices, eps, y_train)
    if tuple(y.shape) != (R, 2):
        raise ValueError(f"dm_umap_transform_layout: y must be ({R}, 2)")
    if not (tuple(eps_neg.shape) == tuple(nxt.shape) == tuple(nxt_neg.shape) == (R, k)):
        raise ValueError(f"dm_umap_transform_layout: eps / eps_neg / next / next_neg must be ({R}, {k})")
    L.check(L.load().dm_umap_transform_layout(_ptr(indices, torch.int32), _ptr(eps), _ptr(eps_neg), _ptr(nxt), _ptr(nxt_neg), R, k,
                                              M, _ptr(y_train), _ptr(y), int(epoch_begin), int(epoch_end), int(n_epochs),
                                              int(row_offset), float(a), float(b), float(gamma),
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(group), _stream()), "dm_umap_transform_layout")
    return y
