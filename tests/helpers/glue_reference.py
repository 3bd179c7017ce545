"""Float64 references and derived error bounds for the kernels between the convolutions: channel statistics, BatchNorm
finalisation (batch, per-sample, running-statistics replay, backward), the slab reductions, the plain reconstruction loss
and Adam.  Restated from include/dynamorph_hip.h and the kernels' header comments -- nothing here calls the library.

Pure CPU (torch on the host, no torch.cuda).  tests/test_glue_reference_host.py shows the references right (against
torch.nn.BatchNorm2d / torch.optim.Adam in float64), measures every bound constant against an fp32 restatement of the
kernel's operation order, and shows that the listed wrong kernels miss the bounds; tests/test_gpu_glue_kernels.py then holds
the kernels to the same references and bounds.

Bounds.  U = 2**-24 is the unit roundoff of fp32: one fp32 operation (or store) on a value x errs by at most U |x|.  A
constant counts the fp32 operations on the longest path to the output, in units of U times the magnitude of the TERMS of
that output (so that a result that cancels is not asked to be accurate relative to itself).  Constants marked "x2" are
twice the worst-case count: the host test demands that the fp32 restatement stays within a quarter of the bound, which a
bare worst-case count cannot give.  The worst restatement ratio measured on the host (tests/test_glue_reference_host.py
prints them) stands next to each constant.
"""
import math

import torch

U = 2.0 ** -24
DENORM = 2.0 ** -149      # smallest fp32 denormal: one denormal ulp
MUTATION_MARGIN = 20.0    # every mutation must miss the bound by this factor on at least one case of the grid
SENTINEL = 12345.0        # guard rows behind every output buffer
F64_SLOP = 2.0 ** -45     # float64 arithmetic on the (sum, sum of products) pairs: 256 double roundings on the terms

# ---- the constants -------------------------------------------------------------------------------------------------
# channel_stats: per group of four, four fp32 products and three fp32 adds, each rounding a value no larger than the
# group's sum |p q|; the groups are then added in double.              measured worst ratio 0.19
C_STATS = 7.0
# bn_finalize / bn_backward_finalize on given double sums: every output is a float64 expression stored once, except
# scale = fl(gamma * fl(invstd)): two roundings.                       measured worst ratio 1.00 (an exact count: held to <= 1)
C_FIN = 2.0
# coef[2] = fl(beta - fl(fl(mean) * scale)): mean 1, scale 2, product 1, difference 1, relative to |beta| + |mean scale|
#                                                                      measured worst ratio 0.57 (an exact count: held to <= 1)
C_FIN_SHIFT = 5.0
# running-statistics replay against the sequential float64 recurrence: the final store (1), a fed statistic that rounds to
# the neighbouring float where the double sums differ in their last bits (one ulp = 2, under weights m (1-m)^k that sum to
# at most 1), and the closed form's (1-m)^B by repeated squaring (< 1).  measured worst ratio 0.20
C_REPLAY = 4.0
# variance of a channel from the fp32-grouped sums: E[x^2] errs by C_STATS U E[x^2], mean^2 by 2 C_STATS U E[x^2], and
# E[x^2] = var (1 + r^2) with r = |mean| / std: relative error of var <= 3 C_STATS U (1 + r^2).
#                                                   measured on the chains with C_BWD: 0.12 (r = 0), 0.09 (3), 0.12 (30)
C_VAR = 3.0 * C_STATS
# fp32 evaluation of c0 p0 [+ c1 p1] + c2 by dm_apply: every coefficient carries at most C_FIN_SHIFT roundings, a product
# one more, the two adds one each on partial sums no larger than the sum of the terms' magnitudes: 5 + 1 + 2 = 8, relative
# to |c0 p0| + |c1 p1| + |c2| (for the backward that sum is ~ |A c2| (|x_hat| + 2 r): the cancellation of B a + C).
#                                                                      (measured with C_VAR, above)
C_BWD = 8.0
# float slabs: nslabs U sum |x| -- an element passes through at most nslabs / 16 + 6 fp32 adds (its accumulator, the pair
# sums, the sixteen group sums), each rounding a partial sum no larger than sum |x|
#                                                                      measured worst ratio 0.10
# reconstruction loss: t = fl(fl(d m) - fl(x m)) errs by 2 U s with s = |d m| + |x m|; t^2 / var by
# (4 |t| s + 2 t^2) U / var <= 6 U s^2 / var; the division and the fp32 store of the mean one more each:
C_RECON = 8.0             # relative to mean(s^2 / var)                measured worst ratio 0.07
# its gradient g = fl(fl(t m) sc), sc = fl(fl(fl(2 / N) gscale) / var): t 2, x m 1, sc 3, product 1 = 7; x2, rounded up
C_RECON_G = 16.0          # relative to s m |sc|                       measured worst ratio 0.19
# per-channel sums of g: the element errors, two fp32 adds per group of four (2 U sum |g|), one store of the sum
C_RECON_B = C_RECON_G + 3.0   # relative to sum s m |sc|               measured worst ratio 0.01
# Adam, first and second moment.  m' = m + w1 (gi - m): gi 1, difference 1 (+ gi's 1), w1 = fl(1 - b1) 1, product 1,
# sum 1: 6 relative to |m| + w1 (|gi| + |m|).  v' = v b2 + w2 gi^2: gi 1 -> gi^2 2 + 1, w2 1, product 1, sum 1: 6
# relative to v' (all terms positive).  x2 = 12, rounded up to 16.     measured worst ratio 0.17 (m), 0.22 (v)
C_ADAM_MV = 16.0
# Adam, parameter.  p' = p - ss (m' / den): den = sqrt(v') / bs + eps carries v' 6/2 = 3, sqrt 1, bs 1, quotient 1, sum 1
# = 7; m' 6 (relative to its terms); quotient 1, ss 1, product 1 = 16 on the update, 1 on the final difference: 17
# relative to |p| + ss (|m| + w1 (|gi| + |m|)) / den, the magnitude of the update's terms.  x2, rounded up = 40.
#                                                                      measured worst ratio 0.08
C_ADAM_P = 40.0


def f32(x):
    """x rounded to fp32, as float64 (a tensor) or float (a number)."""
    if isinstance(x, torch.Tensor):
        return x.to(torch.float32).to(torch.float64)
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def d(x):
    return None if x is None else x.detach().to("cpu", torch.float64)


# ---- channel statistics ------------------------------------------------------------------------------------------------
def channel_stats_ref(p, q=None):
    """(sum p, sum p q) per channel over the whole batch in float64, and the bound on each: (C,) tensors s1, s2, b1, b2."""
    P = d(p)
    Q = P if q is None else d(q)
    s1, s2 = P.sum((0, 2, 3)), (P * Q).sum((0, 2, 3))
    return s1, s2, C_STATS * U * P.abs().sum((0, 2, 3)), C_STATS * U * (P * Q).abs().sum((0, 2, 3))


def channel_stats_f32(p, q=None, drop_last_chunk=False, ignore_q=False):
    """The kernel's operation order in fp32 on the host: groups of four in fp32, the groups added in double, one slab per
    chunk of 32 samples -> (chunks, C, 2) float64.  drop_last_chunk / ignore_q: the wrong kernels of the mutation test."""
    B, Cn, H, W = p.shape
    q = p if (q is None or ignore_q) else q
    a, w = p.reshape(B, Cn, -1, 4), q.reshape(B, Cn, -1, 4)
    g1 = ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])).double()
    g2 = ((a[..., 0] * w[..., 0] + a[..., 1] * w[..., 1]) + (a[..., 2] * w[..., 2] + a[..., 3] * w[..., 3])).double()
    chunks = (B + 31) // 32
    out = torch.zeros(chunks, Cn, 2, dtype=torch.float64)
    for k in range(chunks - (1 if drop_last_chunk and chunks > 1 else 0)):
        out[k, :, 0] = g1[32 * k:32 * k + 32].sum((0, 2))
        out[k, :, 1] = g2[32 * k:32 * k + 32].sum((0, 2))
    return out


# ---- BatchNorm forward finalisation ------------------------------------------------------------------------------------
def _unbias(count):
    return count / (count - 1.0) if count > 1 else 1.0


def bn_finalize_ref(sums, count, gamma, beta, rm, rv, momentum, eps):
    """sums (..., C, 2) float64 = (sum x, sum x^2) per channel [per sample]; gamma / beta / rm / rv (C,) or None.
    Returns a dict of float64 tensors (NOT rounded: the bounds carry the stores): scale, shift (coef[..., 0], coef[..., 2]),
    mean, invstd (saved), var (biased), rm, rv (the new running statistics, batch mode: one update with this batch) and the
    bounds b_scale, b_shift, b_mean, b_invstd, b_rm, b_rv."""
    s = d(sums)
    n = float(count)
    mom, eps = f32(momentum), f32(eps)
    g = torch.ones(s.shape[-2], dtype=torch.float64) if gamma is None else d(gamma)
    bt = torch.zeros(s.shape[-2], dtype=torch.float64) if beta is None else d(beta)
    mean = s[..., 0] / n
    ex2 = s[..., 1] / n
    var = (ex2 - mean * mean).clamp(min=0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = g * invstd
    shift = bt - mean * scale
    slop = F64_SLOP * ex2                       # float64 cancellation of E[x^2] - mean^2, in units of var
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift,
               b_mean=U * mean.abs(), b_invstd=U * invstd + 0.5 * invstd ** 3 * slop,
               b_scale=C_FIN * U * scale.abs() + 0.5 * g.abs() * invstd ** 3 * slop)
    out["b_shift"] = C_FIN_SHIFT * U * (bt.abs() + (mean * scale).abs()) + mean.abs() * 0.5 * g.abs() * invstd ** 3 * slop
    if rm is not None:
        out["rm"] = mom * mean + (1.0 - mom) * d(rm)
        out["b_rm"] = C_FIN * U * out["rm"].abs() + F64_SLOP * (mean.abs() + d(rm).abs())
    if rv is not None:
        out["rv"] = mom * (var * _unbias(n)) + (1.0 - mom) * d(rv)
        out["b_rv"] = C_FIN * U * out["rv"].abs() + _unbias(n) * slop + F64_SLOP * d(rv).abs()
    return out


def bn_running_replay_ref(group_sums, count, rm0, rv0, momentum):
    """The SEQUENTIAL recurrence the closed form replaces: B batch-of-one updates r <- m x_b + (1 - m) r in float64, each
    fed the fp32-rounded mean and unbiased variance of sample b.  group_sums (B, C, 2) float64.  Returns rm, rv, b_rm, b_rv."""
    s = d(group_sums)
    n = float(count)
    mom = f32(momentum)
    mean = s[..., 0] / n
    var = (s[..., 1] / n - mean * mean).clamp(min=0.0)
    xm, xv = f32(mean), f32(var * _unbias(n))
    rm, rv = d(rm0).clone(), d(rv0).clone()
    for b in range(s.shape[0]):
        rm = mom * xm[b] + (1.0 - mom) * rm
        rv = mom * xv[b] + (1.0 - mom) * rv
    b_rm = C_REPLAY * U * torch.maximum(d(rm0).abs(), xm.abs().amax(0))
    b_rv = C_REPLAY * U * torch.maximum(d(rv0).abs(), xv.abs().amax(0))
    return rm, rv, b_rm, b_rv


def bn_running_replay_closed(group_sums, count, rm0, rv0, momentum, weight_shift=0, biased=False, bad_unbias=False):
    """The kernel's closed form (1-m)^B r0 + sum_b m (1-m)^(B-1-b) x_b in double with the one fp32 store.  The keyword
    arguments are the wrong kernels of the mutation test."""
    s = d(group_sums)
    n = float(count)
    B = s.shape[0]
    mom = f32(momentum)
    keep = 1.0 - mom
    mean = s[..., 0] / n
    var = (s[..., 1] / n - mean * mean).clamp(min=0.0)
    if bad_unbias:
        unb = n / (n - 1.0) if n != 1 else float("inf")
    else:
        unb = 1.0 if biased else _unbias(n)
    xm, xv = f32(mean), f32(var * unb)
    w = torch.tensor([mom * keep ** (B - 1 - b + weight_shift) for b in range(B)], dtype=torch.float64).unsqueeze(1)
    rm = keep ** B * d(rm0) + (w * xm).sum(0)
    rv = keep ** B * d(rv0) + (w * xv).sum(0)
    return f32(rm), f32(rv)


# ---- BatchNorm backward finalisation -----------------------------------------------------------------------------------
def bn_backward_ref(sums, count, gamma, saved):
    """sums (C, 2) float64 = (sum dy, sum dy a); saved (C, 2) = (mean, invstd) as stored (fp32).  count == 0: fixed
    statistics, da = gamma invstd dy.  Returns dgamma, dbeta, A, Bc, Cc (da = A dy + Bc a + Cc) and bounds b_*."""
    s, sv = d(sums), d(saved)
    g = torch.ones(s.shape[0], dtype=torch.float64) if gamma is None else d(gamma)
    inv_n = 1.0 / float(count) if count > 0 else 0.0
    mean, invstd = sv[:, 0], sv[:, 1]
    s1, s2 = s[:, 0], s[:, 1]
    dyxh = invstd * (s2 - mean * s1)
    A = g * invstd
    c1, c2 = s1 * inv_n, dyxh * inv_n
    Bc = -A * invstd * c2
    Cc = -A * c1 - Bc * mean
    t_dyxh = invstd * (s2.abs() + (mean * s1).abs())           # magnitude of the terms of the float64 differences
    t_Bc = A.abs() * invstd * t_dyxh * inv_n
    return dict(dgamma=dyxh, dbeta=s1, A=A, Bc=Bc, Cc=Cc,
                b_dgamma=C_FIN * U * dyxh.abs() + F64_SLOP * t_dyxh, b_dbeta=C_FIN * U * s1.abs(),
                b_A=C_FIN * U * A.abs(), b_Bc=C_FIN * U * Bc.abs() + F64_SLOP * t_Bc,
                b_Cc=C_FIN * U * Cc.abs() + F64_SLOP * ((A * c1).abs() + t_Bc * mean.abs()))


# ---- the two chains end to end -----------------------------------------------------------------------------------------
def bn_apply_chain_ref(a, dy, gamma, beta, eps, per_sample=False):
    """Float64 BatchNorm forward and backward by autograd (torch.nn.functional.batch_norm on doubles): the independent
    check of channel_stats -> bn_finalize -> apply and channel_stats(dy, a) -> bn_backward_finalize -> apply(AFFINE2).
    per_sample: every sample is its own batch.  Returns y, da, dgamma, dbeta and the bounds b_y, b_da, b_dgamma, b_dbeta,
    with r = |mean| / std of each channel [and sample] carried honestly (C_VAR (1 + r^2), C_BWD r)."""
    A, DY = d(a).clone().requires_grad_(True), d(dy)
    g, bt = d(gamma).clone().requires_grad_(True), d(beta).clone().requires_grad_(True)
    eps = f32(eps)
    if per_sample:
        y = torch.cat([torch.nn.functional.batch_norm(A[i:i + 1], None, None, g, bt, True, 0.0, eps) for i in range(A.shape[0])])
    else:
        y = torch.nn.functional.batch_norm(A, None, None, g, bt, True, 0.0, eps)
    y.backward(DY)
    a64 = A.detach()
    dims = (2, 3) if per_sample else (0, 2, 3)
    n = a64.numel() / a64.shape[1] / (a64.shape[0] if per_sample else 1)
    k = dict(dim=dims, keepdim=True)
    mean = a64.mean(**k)
    var = a64.var(unbiased=False, **k)
    std = torch.sqrt(var + eps)
    r2 = (a64 * a64).mean(**k) / (var + eps)                   # 1 + r^2 (eps keeps a constant channel finite)
    r = mean.abs() / std
    gg = g.detach().abs().reshape(1, -1, 1, 1)
    xh = ((a64 - mean) / std).abs()
    var_rel = C_VAR * U * r2
    # forward: invstd errs by var_rel / 2, the mean by C_STATS U E|a| <= C_STATS U std sqrt(1 + r^2); then the fp32 affine
    scale = gg / std
    b_y = gg * (0.5 * var_rel * xh + C_STATS * U * torch.sqrt(r2)) + \
        C_BWD * U * ((scale * a64).abs() + bt.detach().abs().reshape(1, -1, 1, 1) + (mean * scale).abs())
    # backward: da = A dy + Bc a + Cc with c1 = mean(dy), c2 = mean(dy x_hat)
    c1 = DY.mean(**k)
    c2 = (DY * (a64 - mean) / std).mean(**k)
    e_dy = DY.abs().mean(**k)
    e_dya = (DY * a64).abs().mean(**k)
    # c1 errs by C_STATS U E|dy|; c2 = invstd (E[dy a] - mean E[dy]) by C_STATS U invstd (E|dy a| + |mean| E|dy|) and the
    # stored mean's rounding U r |c1|; invstd enters da three times (scale, and squared in Bc)
    e_c1 = C_STATS * U * e_dy
    e_c2 = C_STATS * U * (e_dya + mean.abs() * e_dy) / std + U * r * c1.abs() + 0.5 * var_rel * c2.abs()
    Bc = scale * c2 / std
    terms = (scale * DY).abs() + (Bc * a64).abs() + (scale * c1).abs() + (Bc * mean).abs()
    b_da = 1.5 * var_rel * ((scale * DY).abs() + (scale * c1).abs() + (scale * xh * c2).abs()) + \
        scale * (e_c1 + xh * e_c2) + C_BWD * U * terms
    red = (lambda t: t.sum(0)) if per_sample else (lambda t: t)
    sq = (lambda t: red(t).reshape(-1))
    b_dbeta = sq(n * (e_c1 + U * c1.abs()))
    b_dgamma = sq(n * (e_c2 + C_FIN * U * c2.abs()))
    return dict(y=y.detach(), da=A.grad, dgamma=g.grad, dbeta=bt.grad, b_y=b_y, b_da=b_da, b_dgamma=b_dgamma,
                b_dbeta=b_dbeta, r=r)


def with_mean_over_std(x, r):
    """x (B, C, H, W) re-centred so that every channel has |mean| / std = r over the whole batch (r = 30: a post-ReLU
    channel with a large bias)."""
    x = x.double()
    m = x.mean((0, 2, 3), keepdim=True)
    s = x.std((0, 2, 3), unbiased=False, keepdim=True)
    return ((x - m) / s + r).float()


# ---- slab reductions ---------------------------------------------------------------------------------------------------
def reduce_slabs_ref(slabs):
    """(a) float64 column sums with the bound nslabs U sum |x|; (b) the promised ORDER in fp32 on the host: sixteen groups
    g of slabs g, g + 16, ..., four accumulators each (slabs i, i + 16, i + 32, i + 48 per round of 64, the rest into the
    first), (s0 + s1) + (s2 + s3) per group, the groups added in order."""
    s = slabs.detach().cpu().float()
    n, E = s.shape
    exact = s.double().sum(0)
    bound = n * U * s.double().abs().sum(0)
    return exact, bound, reduce_order_f32(s)


def reduce_order_f32(s, drop_partial_group=False):
    n, E = s.shape
    total = torch.zeros(E)
    for g in range(16):
        acc = [torch.zeros(E) for _ in range(4)]
        i = g
        while i + 48 < n:
            for j in range(4):
                acc[j] = acc[j] + s[i + 16 * j]
            i += 64
        while i < n and not drop_partial_group:
            acc[0] = acc[0] + s[i]
            i += 16
        total = total + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
    return total


def sum_slabs_ref(stats, scale=1.0):
    """dst[n] = scale * sum over slabs of stats[slab][n][0], float64 (scale crosses the ABI as a float); bound: the store."""
    t = d(stats)[:, :, 0].sum(0) * f32(scale)
    return t, C_FIN * U * t.abs() + F64_SLOP * d(stats)[:, :, 0].abs().sum(0)


# ---- reconstruction loss -----------------------------------------------------------------------------------------------
def recon_loss_ref(dec, x, mask, var, gscale=1.0):
    """mean(((dec m - x m)^2) / var[c]) in float64, its gradient with respect to dec times gscale and that gradient's
    per-channel sums; mask None, (B, 1, H, W) or (B, NIN, H, W).  Returns loss, g, bias and the bounds b_loss, b_g, b_bias."""
    D, X, V = d(dec), d(x), d(var).reshape(1, -1, 1, 1)
    M = torch.ones_like(D) if mask is None else d(mask).expand_as(D)
    N = D.numel()
    t = D * M - X * M
    s = (D * M).abs() + (X * M).abs()
    loss = (t * t / V).mean()
    sc = f32(gscale) * 2.0 / N / V
    g = t * M * sc
    bias = g.sum((0, 2, 3))
    return dict(loss=loss, g=g, bias=bias, b_loss=C_RECON * U * (s * s / V).mean(), b_g=C_RECON_G * U * s * M.abs() * sc.abs(),
                b_bias=C_RECON_B * U * (s * M.abs() * sc.abs()).sum((0, 2, 3)))


def recon_loss_f32(dec, x, mask, var, gscale=1.0, nblocks=None, one_mask_factor=False, wrong_channel=False):
    """The kernels' operation order in fp32 on the host -> (loss fp32, g, per-channel sums through bias slabs in double).
    nblocks: the launch's grid (planes walk blockIdx, blockIdx + grid, ...).  one_mask_factor / wrong_channel: the wrong
    kernels of the mutation test (the second credits a block's sums to the channel of its FIRST plane)."""
    B, NIN, H, W = dec.shape
    N = dec.numel()
    v = var.reshape(1, -1, 1, 1).float()
    if mask is None:
        t = dec - x
        tm = t
    else:
        m = mask.expand_as(dec)
        t = dec * m - x * m
        tm = t if one_mask_factor else t * m
    sq = t * t
    loss = torch.tensor((sq / v).double().sum().item() / N, dtype=torch.float64).float()
    gs = torch.tensor(2.0 / N, dtype=torch.float64).float() * torch.tensor(gscale, dtype=torch.float32)
    sc = gs / v
    g = tm * sc
    g4 = g.reshape(B * NIN, -1, 4)
    part = ((g4[..., 0] + g4[..., 1]) + (g4[..., 2] + g4[..., 3])).double().sum(1)          # per plane
    nblocks = min(B * NIN, 1024) if nblocks is None else nblocks
    slabs = torch.zeros(nblocks, NIN, dtype=torch.float64)
    for plane in range(B * NIN):
        blk = plane % nblocks
        c = (blk % NIN) if wrong_channel else plane % NIN
        slabs[blk, c] += part[plane]
    return loss, g, slabs.sum(0).float()


# ---- Adam --------------------------------------------------------------------------------------------------------------
def adam_ref(p, g, m, v, t, lr, b1, b2, eps, grad_scale=1.0):
    """The kernel's documented formula in float64, the hyper-parameters first rounded to fp32 (they cross the C ABI as
    float):  gi = g grad_scale;  m' = m + (1 - b1)(gi - m);  v' = v b2 + (1 - b2) gi^2;
    p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps).  Returns p', m', v' and the bounds b_p, b_m, b_v."""
    P, G, M, V = d(p), d(g), d(m), d(v)
    lr, b1, b2, eps, gs = f32(lr), f32(b1), f32(b2), f32(eps), f32(grad_scale)
    t = float(t)
    gi = G * gs
    m1 = M + (1.0 - b1) * (gi - M)
    v1 = V * b2 + (1.0 - b2) * gi * gi
    ss = lr / (1.0 - b1 ** t)
    den = torch.sqrt(v1) / math.sqrt(1.0 - b2 ** t) + eps
    p1 = P - ss * (m1 / den)
    tm = M.abs() + (1.0 - b1) * (gi.abs() + M.abs())
    return dict(p=p1, m=m1, v=v1, b_m=C_ADAM_MV * U * tm + DENORM, b_v=C_ADAM_MV * U * v1 + DENORM,
                b_p=C_ADAM_P * U * (P.abs() + ss * tm / den))


def adam_f32(p, g, m, v, t, lr, b1, b2, eps, grad_scale=1.0, mutation=None):
    """The kernel's operation order in fp32 on the host, one torch op per kernel statement (the bias corrections in double
    from the fp32 betas, as the kernel forms them).  mutation: 'bc_t_minus_1' | 'eps_inside' | 'no_grad_scale' | 'skip_tail'."""
    F = torch.float32
    c = lambda x: torch.tensor(x, dtype=torch.float64).to(F)                # noqa: E731
    lr_, b1_, b2_, eps_, gs_ = c(lr), c(b1), c(b2), c(eps), c(grad_scale)
    tt = float(t) - (1.0 if mutation == "bc_t_minus_1" else 0.0)
    bc1 = 1.0 - float(b1_) ** tt
    bc2 = 1.0 - float(b2_) ** tt
    step_size = c(float(lr_) / bc1) if bc1 != 0.0 else c(float("inf"))
    bc2_sqrt = c(math.sqrt(bc2))
    w1, w2 = c(1.0).to(F) - b1_, c(1.0).to(F) - b2_
    gi = g if mutation == "no_grad_scale" else g * gs_
    mi = m + w1 * (gi - m)
    vi = v * b2_ + w2 * (gi * gi)
    if mutation == "eps_inside":
        denom = (vi.sqrt() + eps_) / bc2_sqrt
    else:
        denom = vi.sqrt() / bc2_sqrt + eps_
    pn = p - step_size * (mi / denom)
    if mutation == "skip_tail":
        k = (p.numel() // 256) * 256
        pn[k:], mi[k:], vi[k:] = p[k:], m[k:], v[k:]
    return pn, mi, vi


def adam_state(n, t, gscale, seed):
    """Inputs of one Adam case: p ~ N(0, 1); g ~ gscale N(0, 1) with every seventh exactly 0; for t > 1 a pre-loaded state
    of the gradient's scale (m ~ 0.1 g-scale, v ~ m^2 + 0.1 g-scale^2: a state Adam can reach has v >= m^2 / 53 at the
    default betas, Cauchy-Schwarz on the two moving averages -- with v << m^2 one step would move p by many lr), zero state
    at t = 1."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * gscale
    g[::7] = 0.0
    if t > 1:
        m = torch.randn(n, generator=gen) * (0.1 * gscale)
        v = (torch.randn(n, generator=gen) * gscale) ** 2 * 0.1 + m * m
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, g, m, v


ADAM_STEPS = (1, 2, 10, 1000, 100000, 1000000)
ADAM_GSCALES = (1.0, 1e-3, 1e-6, 1e-12, 1e-20, 0.0)
ADAM_HYPER = ((1e-4, 0.9, 0.999, 1e-8), (1e-3, 0.8, 0.99, 1e-6))


# ---- the grids both test files walk ------------------------------------------------------------------------------------
def stats_cases(count=24, seed=20260101):
    """A thinned product of B x C x H*W x (q given) x r: every axis is drawn on its own by the seeded generator (its values
    repeated to `count` and shuffled, so every value of every axis occurs and no axis fixes another); the edges the kernel
    has -- q given at more than one chunk, a last chunk of one sample (B = 33), a plane of one float4 -- are asserted."""
    import random
    rng = random.Random(seed)

    def axis(values):
        col = [values[k % len(values)] for k in range(count)]
        rng.shuffle(col)
        return col
    Bs, Cs, HWs = axis((1, 31, 32, 33, 64, 100)), axis((1, 3, 16, 64)), axis((4, 64, 256, 4096))
    Qs, Rs = axis((False, True)), axis((0.0, 3.0, 30.0))
    cases = []
    for B, Cn, HW, q, r in zip(Bs, Cs, HWs, Qs, Rs):
        if B * Cn * HW > 4_000_000:
            B = 33
        cases.append((B, Cn, HW, q, r, rng.randrange(1 << 30)))
    assert any(c[3] and c[0] > 32 for c in cases) and any(c[0] == 33 for c in cases) and any(c[2] == 4 for c in cases)
    assert any(c[3] and c[0] in (33, 100) for c in cases) and any(c[3] for c in cases if c[0] == 1 or c[0] == 31)
    return cases


def stats_inputs(case):
    B, Cn, HW, with_q, r, seed = case
    gen = torch.Generator().manual_seed(seed)
    H = 2 if HW == 4 else int(math.isqrt(HW))
    p = torch.randn(B, Cn, H, HW // H, generator=gen)
    p = with_mean_over_std(p, r) if B * HW > 4 else p + r
    q = torch.randn(B, Cn, H, HW // H, generator=gen) if with_q else None
    return p, q


def synthetic_slabs(nslabs, Cn, seed, mean=0.5, spread=1.0, const_channel=None):
    """(nslabs, C, 2) float64 slabs of (sum x, sum x^2)-like values on a grid of 2**-16, so that their double sums are
    exact in ANY order: finalize is then tested apart from the statistics kernel and apart from summation order."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.round((torch.randn(nslabs, Cn, generator=gen, dtype=torch.float64) * spread + mean) * 65536) / 65536
    x2 = torch.round((x * x + torch.rand(nslabs, Cn, generator=gen, dtype=torch.float64)) * 65536) / 65536
    if const_channel is not None:
        x[:, const_channel] = 0.75
        x2[:, const_channel] = 0.5625
    return torch.stack([x, x2], -1).contiguous()


def finalize_slabs(nslabs, Cn, count, seed):
    """Synthetic slabs for a finalize of `count` values per channel: scaled by a power of two near count / nslabs (so the
    sums stay exact, the mean near 0.5 and the variance positive); channel 0 is CONSTANT 0.75 -- all of it in slab 0, so
    that E[x^2] - mean^2 is exactly 0 and the clamp and the 1 / sqrt(eps) path are reached."""
    slabs = synthetic_slabs(nslabs, Cn, seed) * 2.0 ** round(math.log2(count / nslabs))
    slabs[:, 0] = 0.0
    slabs[0, 0, 0], slabs[0, 0, 1] = 0.75 * count, 0.5625 * count
    return slabs


SLAB_COUNTS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2500)


def finalize_grid():
    """(nslabs, C, count, momentum, eps, form, seed) of the batch-mode finalize cases.  form 0: everything given; 1: gamma /
    beta NULL; 2: running tensors NULL, counter given; 3: running and counter NULL.  The axes advance at different rates,
    so every C meets every form and every count meets every momentum."""
    k = 0
    for nslabs in SLAB_COUNTS:
        for Cn in (1, 5, 64, 130):
            yield (nslabs, Cn, (1, 2, 2048 * 256)[k % 3], (0.1, 0.25, 1.0)[(k // 3) % 3], (1e-5, 1e-3)[(k // 2) % 2],
                   (k // 4) % 4, k + 1)
            k += 1


def per_sample_grid():
    """(B, slabs per sample, C, count, momentum, seed) of the per-sample finalize / replay cases."""
    k = 0
    for B in (1, 2, 255, 256, 257, 1024, 1025):
        for spg in (1, 7, 8, 9):
            yield B, spg, (3, 16, 64)[k % 3], (1, 7, 256)[(k // 3) % 3], (0.1, 0.25, 1.0)[k % 3] if B < 1000 else 0.1, 200 + k
            k += 1


CHAIN_SHAPES = [(2, 8, 16), (33, 16, 16), (70, 8, 32), (33, 8, 32), (2, 16, 32), (70, 16, 16)]      # (B, C, H = W)


def chain_inputs(B, Cn, h, r, seed):
    gen = torch.Generator().manual_seed(seed)
    a = with_mean_over_std(torch.randn(B, Cn, h, h, generator=gen), r)
    dy = torch.randn(B, Cn, h, h, generator=gen)
    return a, dy, torch.rand(Cn, generator=gen) + 0.5, torch.randn(Cn, generator=gen)


# (B, NIN, H = W, mask channels or None).  The launch has min(B NIN, 1024) blocks and a block walks planes blockIdx,
# blockIdx + grid, ...: the last two cases have more than 1024 planes and 1024 % NIN != 0, so a block there visits planes
# of several channels and its bias slab collects more than one channel's sum.
RECON_CASES = [(1, 1, 64, None), (3, 2, 64, 1), (70, 3, 64, 3), (3, 4, 128, 1), (1, 5, 128, 5), (3, 3, 8, 1), (70, 5, 64, None),
               (3, 3, 64, 3), (400, 3, 8, 1), (300, 5, 8, 5)]


def recon_blocks(B, NIN):
    """dm_recon_loss_num_blocks, restated."""
    return min(B * NIN, 1024)


def recon_inputs(B, NIN, h, mc, seed):
    gen = torch.Generator().manual_seed(seed)
    dec, x = torch.randn(B, NIN, h, h, generator=gen), torch.randn(B, NIN, h, h, generator=gen)
    mask = None if mc is None else torch.randint(0, 3, (B, mc, h, h), generator=gen).float() / 2
    var = torch.logspace(-1.3, 0.7, NIN) if NIN > 1 else torch.tensor([0.3])
    return dec, x, mask, var
