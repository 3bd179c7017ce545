"""Float64 references, derived error bounds and the case grids of the fused multi-layer kernels: the decoder tail
(csrc/dec_tail.hip: dec.4 + ReLU + dec.6 + masked loss, its backward and the one-kernel training form), the output head
(csrc/head.hip), the latent tail (csrc/latent_tail.hip) and the enc.0 / enc.1 composition kernels (csrc/optim.hip).
Restated from include/dynamorph_hip.h and the kernels' header comments -- nothing here calls the library.

Pure CPU.  tests/test_tail_reference_host.py shows the references right (against torch.nn.functional + autograd in
float64), proves the exact cases exact, measures every bound constant against an fp32 evaluation on the host and shows
that the listed wrong kernels miss; tests/test_gpu_tail_kernels.py then holds the kernels to the same references.

Two kinds of cases.
EXACT outputs: inputs on small dyadic grids (d2 and x small integers, weights in quarters / halves, mask in {0, 0.5, 1},
var and gscale powers of two, B, NIN and the image sides powers of two so that 2 / N is exact) for which every fp32
intermediate is exactly representable whatever the order of summation: the kernel must equal the float64 reference BIT
FOR BIT.  Which outputs of a case are held exactly is the case's `exact` tuple (the host test proves it per case: fp32 in
two summation orders and float64 must agree): the impulse cases hold every output exactly (their sums have one or a few
terms); the dense dyadic cases hold the per-element outputs (decoded, g2, g4) exactly and their sums -- which outgrow 24
bits of their finest unit -- to the counted bounds; NIN = 3 and batch sizes that are no power of two make 2 / N inexact
and leave only `decoded` exact.
BOUNDED outputs: counted bounds in units of U = 2**-24 times the sum of the magnitudes of the terms of that output.  The
host test demands that an fp32 evaluation (ATen's order for the products, the kernels' split for the sums: fp32 terms, long
sums in double) stays within a quarter of each bound; the worst ratio measured on the host stands next to each constant.

Gates (bounded cases).  A pre-ReLU value of dec.4 closer to zero than its own bound may fall on the other side of d4 > 0
in fp32: such positions are "undecided", every bound downstream of one is widened by the magnitude of the term the gate
would add or drop, and at most UNDECIDED_CAP of the positions of any case may be undecided (asserted from the reference
alone).  d2 > 0 (the tail) and d4 > 0 (the head) are gates on INPUTS: always decided.
"""
import torch
import torch.nn.functional as F

from glue_reference import U, F64_SLOP, MUTATION_MARGIN, SENTINEL, d, f32, with_mean_over_std  # noqa: F401

UNDECIDED_CAP = 1e-3

# ---- the constants -------------------------------------------------------------------------------------------------
# d4 = dec.4(d2) before the ReLU: sixteen products and the bias in one fused-multiply-add chain per accumulator (16), the
# own + side sums joined across the lanes (1), the EDGE seam term (1): 18, relative to |b4| + sum |d2 w4|
#                                     measured on decoded, which carries it: host 0.10, MI355X 0.09
C_TAIL_D4 = 18.0
# decoded = b6 + sum_co w6 d4: four fused multiply-adds (the head: C4 of them), relative to |b6| + sum |w6 d4|; on top of
# the error d4 brings along; x2                                        measured: host 0.10 (tail), 0.20 (head)
C_TAIL_DEC = 8.0
# t = fl(fl(dec m) - fl(x m)): 2 relative to s = |dec m| + |x m| (as C_RECON); loss term fl(fl(t t) fl(1 / var)) (the
# head: fl(fl(t t) / var)) 3 more, the pair sum 1, a lane's fp32 sum over the rows of a tile 5 NIN <= 20: 24 relative
# to t^2 / var, on top of what t brings along                          measured: host 0.004 (tail), 0.007 (head)
C_TAIL_LOSS = 24.0
# g_dec = fl(fl(t m) sc), sc = fl(fl(fl(2 / N) gscale) / var): t m 1, sc 3, product 1 (+ 1 for the head's + gdec_ext): 6
# relative to |t m sc| (+ |gdec_ext|), on top of what t brings along   measured with C_TAIL_G4, below
C_TAIL_GD = 6.0
# g4 = sum_c w6[c] g_dec[c]: NIN <= 4 multiply-adds relative to sum |w6 g_dec|; x2
#                                                                      measured (head g4): host 0.21
C_TAIL_G4 = 8.0
# g2 = sum over 64 terms g4 w4: four accumulators of sixteen fused multiply-adds (16), own + side (1), the lane exchange
# (1), the EDGE seam sum (its own chain of 16, then 1): 20 relative to sum |g4 w4|     measured: host 0.12
C_TAIL_G2 = 20.0
# per-lane fp32 partial sums of phase B (dW6, db6, db4): one product and at most five rows per tile; db2: eight rows per
# tile; times the tiles a workgroup walks (tail_launch: per_wg).  Relative to the sum of the terms' magnitudes.
#                                           measured: host 0.04 (dW6), 0.03 (db6), 0.03 (db4), 0.01 (db2)
C_TAIL_ROWS, C_TAIL_ROWS_G2 = 6.0, 8.0
# dW4 on the matrix unit: a wave's 39 steps of a tile go to two accumulators (20 each), a step adds four products (4):
# 80 per tile a workgroup walks, + 1 (the two accumulators) + 3 (the four waves); then dm_reduce_slabs: nslabs / 16 + 6
#                                                                      measured: host 0.02
C_TAIL_W4_TILE, C_TAIL_W4_FIX = 80.0, 10.0
# head: per-thread fp32 sums: product 1, three adds of the float4's lanes, one onto the accumulator, per grid-stride pass
#                                                                      measured: host 0.03 (dW6, db6), 0.02 (db4)
C_HEAD_ROWS = 5.0
# latent tail.  A counted worst-case envelope cannot be carried through this stack: every convolution multiplies it by the sum
# of the magnitudes of its weights against a signal that grows with their root sum of squares (about 10 per 3x3 product,
# 4.5 per 1x1), so after two residual layers it exceeds the activations.  What is propagated instead, layer by layer, is the
# STANDARD DEVIATION of each element's error under the standard model of rounding errors: independent, uniform within
# U |x| (variance U^2 x^2 / 3, taken as U^2 x^2).  A chain of cnt fused steps rounds partial sums that grow like sqrt(k) rms
# terms: variance U^2 cnt / 2 sum (t w)^2 (_lt_conv); input errors pass in quadrature through w^2; a patch's mean and variance
# are means of n = 256 values, their errors have the variance of the elements' over n (_lt_bn), and the normalised value
# inherits them through 1 / std of THAT patch (the C_VAR argument of glue_reference, in quadrature).  The bound is K_SIGMA
# standard deviations.  K_SIGMA = 32: an fp32 evaluation of 4 million elements reaches about 5 when the model holds and must
# stay within a quarter of the bound (8); errors that the model's independence misses (a coefficient shared by a channel)
# have a factor of six of room.                      measured worst ratio: host 0.02 (z), 0.03 (statistics)
K_SIGMA = 32.0
# chain lengths: a 3x3 product over 16 channels is 36 matrix steps of four products (144) and the bias; the 1x1 over 32
# channels 8 steps (32) + 1; enc.7 (4x4, 16 channels) 64 steps (256) + 1.  BatchNorm application scale v + shift: scale 2,
# mean 1, shift 2, product and sum 2, the residual join 1 = 8 (glue_reference.C_BWD), relative to the terms.
C_LT_CONV3, C_LT_CONV1, C_LT_BN = 145.0, 33.0, 8.0
# composition kernels: a double sum stored once (an exact count: held to <= 1)
C_E1 = 1.0


# ======================================================================================================= decoder tail
def tail_tiles_x(W2):
    return 1 if W2 == 64 else -(-W2 // 56)


def tail_grid(ntiles):
    return min(ntiles, 768)


def tail_bwd_occ(NIN, tiling):
    return 3 if (tiling == "full" and NIN <= 2) else 2


def tail_launch(B, NIN, H2, W2, fused):
    """tail_backward_launch, restated: the tiling a call takes, its tiles, grid, the slab count (sized for the forward
    grid over the WIDE tile count) and the tiles a workgroup walks at most."""
    ty = H2 // 8
    wide_tiles = B * ty * tail_tiles_x(W2)
    if W2 == 64:
        tiling, nt, tx = "full", wide_tiles, 1
    elif fused and W2 % 64 == 0:
        tiling, tx = "edge", W2 // 64
        nt = B * ty * tx
    else:
        tiling, nt, tx = "wide", wide_tiles, tail_tiles_x(W2)
    grid = min(nt, 256 * tail_bwd_occ(NIN, tiling))
    return dict(tiling=tiling, ntiles=nt, tiles_x=tx, tiles_y=ty, grid=grid, nslabs=tail_grid(wide_tiles),
                fwd_grid=tail_grid(wide_tiles), per_wg=-(-nt // grid))


def _dw4(d2, g4):
    """dW4[ci][co][ky][kx] = sum d2[ci][y][x] g4[co][2y - 1 + ky][2x - 1 + kx]."""
    gp = F.pad(g4, (1, 1, 1, 1))
    H, W = d2.shape[2:]
    out = torch.zeros(4, 4, 4, 4, dtype=d2.dtype)
    for ky in range(4):
        for kx in range(4):
            out[:, :, ky, kx] = torch.einsum("bcyx,bdyx->cd", d2, gp[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2])
    return out


def _bands(t, dim, width, fn):
    """fn applied to every band of `width` along `dim` on its own (what lies beyond a band reads as zero), re-joined."""
    return torch.cat([fn(b) for b in torch.split(t, width, dim)], dim)


TAIL_MUTATIONS = ("seam_d2_zero", "halo_row_d4", "g4_pad_zero", "halo_row_g4", "stale_seam", "halo_col_twice",
                  "ownerless_slab", "mask_ch0", "gate_ge", "g2_ungated", "db2_before_gate")


def dec_tail_ref(d2, w4, b4, w6, b6, x, mask, var, gscale, fused=True, dyadic=False, mut=None, dtype=torch.float64):
    """dec.4 (ConvTranspose2d(4, 4, 4, 2, 1)) + ReLU + dec.6 (1x1) + masked loss and the gradients of gscale * loss.
    d2 (B, 4, H2, W2); w4 (4, 4, 4, 4) [ci][co][ky][kx]; w6 (NIN, 4); b6 None = 0; mask None, (B, 1, ..) or (B, NIN, ..).
    x None: decoded only.  Returns a dict: decoded, loss, g2, dW4, dW6, db6, db4, db2 and b_<name> for each, `undecided`
    (share of d4 positions whose gate fp32 may decide the other way).  dyadic: the inputs are an exact case's (d4 is
    exact, no gate is undecided).  fused: the launch the sums' counts are taken for (tail_launch).
    dtype float32 evaluates the same expressions in fp32 (the host's exactness proof and quarter check).
    mut: one of TAIL_MUTATIONS, the wrong kernels of the mutation test."""
    c = (lambda t: None if t is None else t.detach().to("cpu", dtype))
    S = (lambda t: t.double())                # sums: in double over the terms as computed (the kernels' long sums are double)
    D2, W4, B4, W6, X, V = c(d2), c(w4), c(b4), c(w6).reshape(-1, 4), c(x), c(var)
    NIN = W6.shape[0]
    B6 = torch.zeros(NIN, dtype=dtype) if b6 is None else c(b6)
    B, _, H2, W2 = D2.shape
    L = tail_launch(B, NIN, H2, W2, fused)
    bw = 56 if L["tiling"] == "wide" else 64
    convT = lambda t, w, b: F.conv_transpose2d(t, w, b, stride=2, padding=1)        # noqa: E731
    if mut == "seam_d2_zero" and L["tiles_x"] > 1:
        d4pre = _bands(D2, 3, bw, lambda t: convT(t, W4, B4))
    elif mut == "halo_row_d4":
        d4pre = _bands(D2, 2, 8, lambda t: convT(t, W4, B4))
    elif mut == "stale_seam" and L["tiling"] == "edge" and L["ntiles"] > L["grid"]:
        d4pre = _stale_seam_d4(D2, W4, B4, L)
    else:
        d4pre = convT(D2, W4, B4)
    d4 = d4pre.clamp(min=0)
    dec = torch.einsum("bdhw,cd->bchw", d4, W6) + B6.reshape(1, -1, 1, 1)
    out = dict(decoded=dec, launch=L)
    m4 = convT(D2.abs(), W4.abs(), B4.abs())
    b_d4 = torch.zeros_like(m4) if dyadic else C_TAIL_D4 * U * m4
    mdec = torch.einsum("bdhw,cd->bchw", d4, W6.abs()) + B6.abs().reshape(1, -1, 1, 1)
    b_dec = C_TAIL_DEC * U * mdec + torch.einsum("bdhw,cd->bchw", b_d4, W6.abs())
    out["b_decoded"] = b_dec
    if X is None:
        return out
    Vc = V.reshape(1, -1, 1, 1)
    M = torch.ones_like(dec) if mask is None else c(mask).expand_as(dec)
    if mut == "mask_ch0" and mask is not None:
        M = c(mask)[:, :1].expand_as(dec)
    N = dec.numel()
    t = dec * M - X * M
    s = (dec * M).abs() + (X * M).abs()
    dt = M.abs() * b_dec + 2 * U * s
    lterm = t * t / Vc
    if mut == "halo_col_twice" and L["tiling"] == "wide":
        col = torch.arange(2 * W2) // 2
        twice = ((col % 56 >= 52) & (col + 4 < W2)) | ((col % 56 < 4) & (col >= 56))        # a neighbour tile's halo lanes
        lterm = lterm * (1 + twice.to(dtype))
    out["loss"] = S(lterm).sum() / N
    out["b_loss"] = ((2 * t.abs() * dt + dt * dt) / Vc + C_TAIL_LOSS * U * t * t / Vc).sum() / N
    gs = torch.tensor(2.0 / N, dtype=dtype) * torch.as_tensor(gscale, dtype=torch.float32).to(dtype).reshape(())
    sc = gs / Vc
    gd = t * M * sc
    b_gd = (M * sc).abs() * dt + C_TAIL_GD * U * gd.abs()
    g4u = torch.einsum("bchw,cd->bdhw", gd, W6)
    b_g4u = torch.einsum("bchw,cd->bdhw", b_gd, W6.abs()) + C_TAIL_G4 * U * torch.einsum("bchw,cd->bdhw", gd.abs(), W6.abs())
    gate = (d4pre >= 0) if mut == "gate_ge" else (d4pre > 0)
    und = (d4pre.abs() <= b_d4) & (not dyadic)
    out["undecided"] = float(und.double().mean())
    g4 = g4u * gate
    e_g4 = torch.where(und, g4u.abs() + b_g4u, b_g4u * gate)
    rows, rows2 = C_TAIL_ROWS * L["per_wg"], C_TAIL_ROWS_G2 * L["per_wg"]
    own = 1.0
    if mut == "halo_col_twice" and L["tiling"] == "wide":
        own = 1 + twice.to(dtype)
    out["db6"] = S(gd * own).sum((0, 2, 3))
    out["b_db6"] = b_gd.sum((0, 2, 3)) + rows * U * gd.abs().sum((0, 2, 3))
    out["dW6"] = torch.einsum("bchw,bdhw->cd", S(gd * own), S(d4))
    out["b_dW6"] = torch.einsum("bchw,bdhw->cd", b_gd, d4 + b_d4) + torch.einsum("bchw,bdhw->cd", gd.abs(), b_d4) + \
        rows * U * torch.einsum("bchw,bdhw->cd", gd.abs(), d4)
    out["db4"] = S(g4 * own).sum((0, 2, 3))
    out["b_db4"] = e_g4.sum((0, 2, 3)) + rows * U * g4.abs().sum((0, 2, 3))
    back = lambda t, w: F.conv2d(t, w, None, stride=2, padding=1)                  # noqa: E731   (w4 as (out = ci, in = co))
    if mut == "g4_pad_zero" and L["tiles_x"] > 1:
        g2pre = _bands(g4, 3, 2 * bw, lambda t: back(t, W4))
    elif mut == "halo_row_g4":
        g2pre = _bands(g4, 2, 16, lambda t: back(t, W4))
    else:
        g2pre = back(g4, W4)
    g2 = g2pre if mut == "g2_ungated" else g2pre * (D2 > 0)
    e_g2 = (back(e_g4, W4.abs()) + C_TAIL_G2 * U * back(g4.abs(), W4.abs())) * (D2 > 0)
    out["g2"], out["b_g2"] = g2, e_g2
    out["db2"] = S(g2pre if mut == "db2_before_gate" else g2).sum((0, 2, 3))
    out["b_db2"] = e_g2.sum((0, 2, 3)) + rows2 * U * g2.abs().sum((0, 2, 3))
    out["dW4"] = _dw4(S(D2), S(g4))
    cw4 = C_TAIL_W4_TILE * L["per_wg"] + C_TAIL_W4_FIX + L["nslabs"] / 16.0
    out["b_dW4"] = _dw4(D2.abs(), e_g4) + cw4 * U * _dw4(D2.abs(), g4.abs())
    if mut == "ownerless_slab" and L["nslabs"] > L["grid"]:
        # the slabs [grid, nslabs) keep what the buffer held: the test pre-fills it with the sentinel
        extra = (L["nslabs"] - L["grid"]) * SENTINEL
        for k in ("loss", "dW4", "dW6", "db6", "db4", "db2"):
            out[k] = out[k] + (extra / N if k == "loss" else extra)
    return out


def _stale_seam_d4(D2, W4, B4, L):
    """EDGE with the seam columns x0 - 1 / x0 + 64 of a workgroup's LATER tiles (tile >= grid) left at what its previous
    tile (tile - grid) fetched, on the rows of the tile's own band."""
    B, _, H2, W2 = D2.shape
    tx, ty, grid = L["tiles_x"], L["tiles_y"], L["grid"]
    Dp = F.pad(D2, (1, 1))
    left = torch.stack([Dp[..., 64 * k] for k in range(tx)], -1)               # (B, 4, H2, tx): column 64 k - 1
    right = torch.stack([Dp[..., 64 * k + 65] for k in range(tx)], -1)
    l2, r2 = left.clone(), right.clone()
    where = lambda t: ((t // tx) // ty, 8 * ((t // tx) % ty), t % tx)          # noqa: E731
    for t in range(grid, L["ntiles"]):
        (b, y0, k), (pb, py0, pk) = where(t), where(t - grid)
        l2[b, :, y0:y0 + 8, k] = left[pb, :, py0:py0 + 8, pk]
        r2[b, :, y0:y0 + 8, k] = right[pb, :, py0:py0 + 8, pk]
    parts = []
    for k in range(tx):
        ext = torch.cat([l2[..., k:k + 1], D2[..., 64 * k:64 * k + 64], r2[..., k:k + 1]], 3)
        parts.append(F.conv_transpose2d(ext, W4, B4, stride=2, padding=1)[..., 2:130])
    return torch.cat(parts, 3)


TAIL_SUMS = ("loss", "dW4", "dW6", "db6", "db4", "db2")
TAIL_ALL = ("decoded", "g2") + TAIL_SUMS


def _mask(gen, B, mc, H, W):
    if mc is None:
        return None
    return torch.randint(0, 3, (B, mc, H, W), generator=gen).float() / 2      # {0, 0.5, 1}: exact zeros included


def tail_inputs(case):
    """The inputs of a decoder-tail case: dict(d2, w4, b4, w6, b6, x, mask, var, gscale).
    kind 'randn': unit-scale inputs, weights of scale 0.3 (bounded).  kind 'dyadic': d2 integers in [0, 2] (half of them
    0), x integers in [-2, 2], w4 in quarters within +-0.5, w6 in halves within +-1, biases in halves, var powers of
    two, gscale 0.5.  kind 'impulse_d2': the dyadic weights with d2 zero but for ONE element (value 2) at (b, ci, y, x) =
    case['at'] and x = the decoded of that input, + 1 on the impulse's sample and on sample 0; kind 'impulse_x': dyadic d2 and x = decoded exactly
    but for ONE pixel (+ 2) at case['at']."""
    B, NIN, H2, W2, mc = case["B"], case["NIN"], case["H2"], case["W2"], case["mask"]
    mc = NIN if mc == "nin" else mc
    gen = torch.Generator().manual_seed(case["seed"])
    OH, OW = 2 * H2, 2 * W2
    if case["kind"] == "randn":
        d2 = torch.randn(B, 4, H2, W2, generator=gen).clamp(min=0)
        w4, b4 = torch.randn(4, 4, 4, 4, generator=gen) * 0.3, torch.randn(4, generator=gen)
        w6, b6 = torch.randn(NIN, 4, generator=gen), torch.randn(NIN, generator=gen)
        x = torch.randn(B, NIN, OH, OW, generator=gen)
        var = torch.logspace(-1.0, 0.5, NIN) if NIN > 1 else torch.tensor([0.3])
        return dict(d2=d2, w4=w4, b4=b4, w6=w6, b6=b6, x=x, mask=_mask(gen, B, mc, OH, OW), var=var, gscale=0.7)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()       # noqa: E731
    w4, b4 = ri(-2, 2, 4, 4, 4, 4) / 4, ri(-1, 2, 4) / 2
    w6, b6 = ri(-2, 2, NIN, 4) / 2, ri(-2, 2, NIN) / 2
    var = torch.tensor([0.5, 2.0, 1.0, 4.0])[:NIN]
    mask = _mask(gen, B, mc, OH, OW)
    d2 = ri(-2, 2, B, 4, H2, W2).clamp(min=0)
    if case["kind"] == "impulse_d2":
        b, ci, y, xx = case["at"]
        d2 = torch.zeros(B, 4, H2, W2)
        d2[b, ci, y, xx] = 2.0
    dec = dec_tail_ref(d2, w4, b4, w6, b6, None, None, var, 0.5)["decoded"].float()
    if case["kind"] == "dyadic":
        x = ri(-2, 2, B, NIN, OH, OW)
    elif case["kind"] == "impulse_d2":
        x = dec.clone()
        x[[0, case["at"][0]]] += 1.0      # x != decoded on every pixel of the impulse's sample and of sample 0 (a first tile)
    else:
        x = dec.clone()
        b, ch, y, xx = case["at"]
        x[b, ch, y, xx] += 2.0
        if mask is not None:
            mask[b, :, y, xx] = 1.0
    return dict(d2=d2, w4=w4, b4=b4, w6=w6, b6=b6, x=x, mask=mask, var=var, gscale=0.5)


def _case(kind, B, NIN, H2, W2, mask, seed, exact=(), at=None):
    name = f"{kind}-B{B}-n{NIN}-{H2}x{W2}-m{mask}" + ("" if at is None else "-at" + "_".join(map(str, at)))
    return dict(kind=kind, B=B, NIN=NIN, H2=H2, W2=W2, mask=mask, seed=seed, exact=tuple(exact), at=at, name=name)


def _pow2(n):
    return n & (n - 1) == 0


def tail_cases():
    """The decoder-tail grid.  Every case is run forward, backward (not fused) and as the training form.
    exact: the outputs the case holds bit for bit (module docstring); everything else to its bound."""
    cases = []
    masks = (None, 1, "nin")
    k = 0
    # every tiling, bounded: 64 wide; WIDE with one, two (a last tile of 4 and of 44 columns) and three tiles (the last owns
    # 8); EDGE with two, three and five tiles (the backward that is not fused takes WIDE there and must agree)
    for (H2, W2) in ((16, 64), (8, 4), (16, 60), (8, 100), (16, 120), (16, 128), (8, 192), (8, 320)):
        for j in range(2):
            NIN = 1 + (k % 4)
            cases.append(_case("randn", 2 + (k % 2), NIN, H2, W2, masks[k % 3], 1000 + k))
            k += 1
    # every instantiation: NIN 1 .. 4 x mask absent / 1 channel / NIN channels x {64 wide, WIDE 60, 128 (EDGE fused, WIDE not)}, small
    for NIN in (1, 2, 3, 4):
        for mk in masks:
            for W2 in (64, 60, 128):
                cases.append(_case("randn", 1, NIN, 8, W2, mk, 1500 + k))
                k += 1
    # the same tilings on the dyadic grid: per-element outputs bit for bit where 2 / N is exact
    for (B, NIN, H2, W2, mk) in ((2, 2, 16, 64, 1), (4, 4, 8, 64, "nin"), (2, 1, 8, 128, "nin"), (1, 2, 16, 256, None),
                                 (2, 3, 8, 64, "nin"), (2, 4, 8, 60, 1), (3, 2, 8, 128, 1)):
        pw = _pow2(B * NIN * H2 * W2)
        cases.append(_case("dyadic", B, NIN, H2, W2, mk, 2000 + k, exact=("decoded", "g2") if pw else ("decoded",)))
        k += 1
    # more tiles than the grid (H2 = 8: one band per sample), dyadic so that the per-element outputs stay exact:
    #   64 wide:  occ 3 (NIN <= 2): backward cap = forward cap = 768 -> B = 1024 (a power of two: g2 exact too);
    #             occ 2 (NIN 3, 4): backward cap 512 -> B = 520 (ownerless slabs 512 .. 519) and B = 776 (> 768 as well)
    #   WIDE 120: three tiles a row, occ 2 -> B = 172 (516 tiles) and B = 258 (774 > 768)
    #   EDGE 128: two tiles a row (slabs sized for WIDE's three) -> B = 258 (516 tiles, 768 slabs) and B = 386 (772 > 768);
    #             the backward that is not fused walks these as 774 / 1158 WIDE tiles
    for (B, NIN, W2, mk) in ((1024, 2, 64, 1), (520, 3, 64, "nin"), (776, 4, 64, None), (172, 1, 120, "nin"),
                             (258, 4, 120, 1), (258, 3, 128, 1), (386, 2, 128, "nin")):
        pw = _pow2(B * NIN * 8 * W2)
        cases.append(_case("dyadic", B, NIN, 8, W2, mk, 3000 + k, exact=("decoded", "g2") if pw else ("decoded",)))
        k += 1
    return cases


def tail_impulse_cases():
    """Impulse cases (every output exact): one nonzero d2 element, and separately one pixel with x != decoded, at each
    structural position -- columns 0, 55 / 56, 63 / 64, 111 / 112, 127 / 128, W2 - 1 and rows 0, 7 / 8, H2 - 1 -- for 64 wide and
    for 128 and 256 wide (powers of two, so that 2 / N is exact: the training form walks them as EDGE tiles, the backward that
    is not fused as WIDE tiles); and in a LATER tile of a workgroup: B = 1024 at 8 x 64 with the impulse in sample
    900 (tile 900 >= 768, the forward and every backward grid); B = 512 at 8 x 128 with the impulse in sample 300 / 511 at the seam
    columns 63 / 64 / 127 (EDGE tiles 600 .., 1022 .. of 1024 on a grid of 512; WIDE tiles 900 .., 1533 .. of 1536 on 768
    forward / 512 backward).  later_tile(case) tells."""
    cases = []
    k = 0
    for (NIN, H2, W2, mk) in ((2, 16, 64, 1), (4, 16, 128, "nin"), (1, 16, 256, None)):
        cols = sorted({cx for cx in (0, 55, 56, 63, 64, 111, 112, 127, 128, W2 - 1) if cx < W2})
        rows = (0, 7, 8, H2 - 1)
        for i, cx in enumerate(cols):
            y = rows[i % 4]
            cases.append(_case("impulse_d2", 2, NIN, H2, W2, mk, 4000 + k, TAIL_ALL, at=(1, i % 4, y, cx)))
            # the pixel of x: output column 2 cx + (i & 1) ^ 1 -- the odd column left of a seam, the even one right of it
            cases.append(_case("impulse_x", 2, NIN, H2, W2, mk, 4100 + k, TAIL_ALL,
                               at=(1, i % NIN, 2 * y + (i & 1), 2 * cx + 1 - (i & 1))))
            k += 1
    for (B, NIN, W2, b, cx) in ((1024, 2, 64, 900, 63), (1024, 4, 64, 900, 0), (512, 4, 128, 300, 64), (512, 2, 128, 300, 63),
                                (512, 1, 128, 511, 127)):
        cases.append(_case("impulse_d2", B, NIN, 8, W2, 1, 4200 + k, TAIL_ALL, at=(b, 1, 7, cx)))
        cases.append(_case("impulse_x", B, NIN, 8, W2, 1, 4300 + k, TAIL_ALL, at=(b, 0, 15, 2 * cx + 1)))
        k += 1
    return cases


def impulse_tiles(case, fused, forward=False):
    """The tile indices that own the impulse's column (d2 column; for impulse_x the output column halved) under the launch's
    tiling, and that launch's grid."""
    L = tail_launch(case["B"], case["NIN"], case["H2"], case["W2"], fused)
    b, _, y, cx = case["at"]
    if case["kind"] == "impulse_x":
        y, cx = y // 2, cx // 2
    w = {"full": 64, "edge": 64, "wide": 56}[L["tiling"]]
    t = ((b * L["tiles_y"]) + y // 8) * L["tiles_x"] + cx // w
    return t, (L["fwd_grid"] if forward else L["grid"])


# =============================================================================================================== head
HEAD_MAX_BLOCKS = 2048
HEAD_MUTATIONS = ("first4", "ext_ignored", "ext_before_scale", "skip_second_pass", "mask_ch0", "gate_ge")


def head_blocks(B, H, W):
    return min((B * H * W // 4 + 255) // 256, HEAD_MAX_BLOCKS)


def head_ref(d4, w6, b6, x, mask, var, gscale, gdec_ext, mut=None, dtype=torch.float64):
    """decoded = dec.6(d4) (+ b6; None = 0), loss = mean((dec m - x m)^2 / var), g_dec = gscale 2 (dec m - x m) m / (var N)
    (left out when gscale is None) + gdec_ext (when given), g4 = (W6^T g_dec)(d4 > 0), dW6, db6, sum g4 (db4).
    d4 (B, C4, H, W) is an INPUT: its gate is always decided."""
    c = (lambda t: None if t is None else t.detach().to("cpu", dtype))
    D4, W6, X, V, EXT = c(d4), c(w6), c(x), c(var), c(gdec_ext)
    W6 = W6.reshape(W6.shape[0], -1)
    NIN, C4 = W6.shape
    B6 = torch.zeros(NIN, dtype=dtype) if b6 is None else c(b6)
    B, _, H, Wd = D4.shape
    passes = -(-(B * H * Wd // 4) // (head_blocks(B, H, Wd) * 256))
    Wf = W6.clone()
    if mut == "first4":
        Wf[:, 4:] = 0
    dec = torch.einsum("bdhw,cd->bchw", D4, Wf) + B6.reshape(1, -1, 1, 1)
    b_dec = ((2 * C4 + 2) * U) * (torch.einsum("bdhw,cd->bchw", D4.abs(), W6.abs()) + B6.abs().reshape(1, -1, 1, 1))
    live = torch.ones(B * H * Wd, dtype=torch.bool)
    if mut == "skip_second_pass":
        live[head_blocks(B, H, Wd) * 256 * 4:] = False
    live = live.reshape(B, 1, H, Wd)
    out = dict(decoded=dec * live, b_decoded=b_dec, passes=passes)
    if X is None:
        return out
    Vc = V.reshape(1, -1, 1, 1)
    M = torch.ones_like(dec) if mask is None else c(mask).expand_as(dec)
    if mut == "mask_ch0" and mask is not None:
        M = c(mask)[:, :1].expand_as(dec)
    N = dec.numel()
    t = dec * M - X * M
    s = (dec * M).abs() + (X * M).abs()
    dt = M.abs() * b_dec + 2 * U * s
    out["loss"] = (t * t / Vc * live).double().sum() / N
    out["b_loss"] = ((2 * t.abs() * dt + dt * dt) / Vc + C_TAIL_LOSS * U * t * t / Vc).sum() / N
    gd, b_gd = torch.zeros_like(dec), torch.zeros_like(dec)
    if gscale is not None:
        sc = torch.tensor(2.0 / N, dtype=dtype) * torch.as_tensor(gscale, dtype=torch.float32).to(dtype).reshape(()) / Vc
        if mut == "ext_before_scale" and EXT is not None:
            gd = (t * M + EXT) * sc
        else:
            gd = t * M * sc
        b_gd = (M * sc).abs() * dt + C_TAIL_GD * U * gd.abs()
    if EXT is not None and mut not in ("ext_ignored", "ext_before_scale"):
        gd = gd + EXT
        b_gd = b_gd + U * (gd.abs() + EXT.abs())
    gd = gd * live
    gate = (D4 >= 0) if mut == "gate_ge" else (D4 > 0)
    g4 = torch.einsum("bchw,cd->bdhw", gd, Wf) * gate
    b_g4 = (torch.einsum("bchw,cd->bdhw", b_gd, W6.abs()) + C_TAIL_G4 * U * torch.einsum("bchw,cd->bdhw", gd.abs(), W6.abs())) * gate
    rows = C_HEAD_ROWS * passes
    out.update(g4=g4, b_g4=b_g4, gdec=gd,
               dW6=torch.einsum("bchw,bdhw->cd", gd.double(), D4.double()),
               b_dW6=torch.einsum("bchw,bdhw->cd", b_gd, D4.abs()) + rows * U * torch.einsum("bchw,bdhw->cd", gd.abs(), D4.abs()),
               db6=gd.double().sum((0, 2, 3)), b_db6=b_gd.sum((0, 2, 3)) + rows * U * gd.abs().sum((0, 2, 3)),
               db4=g4.double().sum((0, 2, 3)), b_db4=b_g4.sum((0, 2, 3)) + rows * U * g4.abs().sum((0, 2, 3)))
    return out


HEAD_SUMS = ("loss", "dW6", "db6", "db4")


def head_cases():
    """(kind, B, C4, NIN, H, W, mask, form, seed, exact): form 'g' gscale only, 'e' gdec_ext only, 'ge' both.  C4 in
    {4, 8, 16} x NIN 1 .. 4 (thinned so that every pair occurs, bounded and dyadic alternating), one size below a single
    workgroup (B = 1 at 8 x 8: 16 float4s), one whose total4 exceeds HEAD_MAX_BLOCKS * 256 (B = 130 at 128 x 128:
    532 480 > 524 288, the grid-stride loop runs twice for the first 8 192 threads)."""
    cases, k = [], 0
    masks, forms = (None, 1, "nin"), ("g", "e", "ge")
    for C4 in (4, 8, 16):
        for NIN in (1, 2, 3, 4):
            B, h = (2, 32) if k % 2 else (3, 16)
            kind = "dyadic" if k % 2 else "randn"
            exact = ("decoded", "g4") if (kind == "dyadic" and _pow2(NIN)) else (("decoded",) if kind == "dyadic" else ())
            cases.append(dict(kind=kind, B=B, C4=C4, NIN=NIN, H=h, W=h, mask=masks[(k // 2) % 3], form=forms[k % 3],
                              seed=5000 + k, exact=exact))
            k += 1
    # every C4 meets every mask layout and every form (small: 16 float4s, below a single workgroup)
    for C4 in (4, 8, 16):
        for mk in masks:
            for form in forms:
                cases.append(dict(kind="randn", B=1, C4=C4, NIN=1 + (k % 4), H=8, W=8, mask=mk, form=form, seed=5200 + k, exact=()))
                k += 1
    cases.append(dict(kind="randn", B=1, C4=8, NIN=3, H=8, W=8, mask="nin", form="ge", seed=5100, exact=()))
    cases.append(dict(kind="dyadic", B=1, C4=4, NIN=2, H=8, W=8, mask=1, form="g", seed=5101, exact=("decoded", "g4")))
    cases.append(dict(kind="randn", B=130, C4=4, NIN=2, H=128, W=128, mask=1, form="ge", seed=5102, exact=()))
    cases.append(dict(kind="dyadic", B=130, C4=16, NIN=1, H=128, W=128, mask="nin", form="g", seed=5103, exact=("decoded",)))
    for cs in cases:
        cs["name"] = f"{cs['kind']}-B{cs['B']}-c{cs['C4']}-n{cs['NIN']}-{cs['H']}-m{cs['mask']}-{cs['form']}"
    assert any(c["B"] * c["H"] * c["W"] // 4 > HEAD_MAX_BLOCKS * 256 for c in cases)
    assert any(c["B"] * c["H"] * c["W"] // 4 < 256 for c in cases)
    return cases


def head_inputs(case):
    B, C4, NIN, H, W = case["B"], case["C4"], case["NIN"], case["H"], case["W"]
    mc = NIN if case["mask"] == "nin" else case["mask"]
    gen = torch.Generator().manual_seed(case["seed"])
    if case["kind"] == "randn":
        d4 = torch.randn(B, C4, H, W, generator=gen).clamp(min=0)
        w6, b6 = torch.randn(NIN, C4, generator=gen) * 0.5, torch.randn(NIN, generator=gen)
        x = torch.randn(B, NIN, H, W, generator=gen)
        ext = torch.randn(B, NIN, H, W, generator=gen) * (1.0 / x.numel())
        var = torch.logspace(-1.0, 0.5, NIN) if NIN > 1 else torch.tensor([0.3])
        gs = 0.7
    else:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()       # noqa: E731
        d4 = ri(-2, 2, B, C4, H, W).clamp(min=0)
        w6, b6 = ri(-2, 2, NIN, C4) / 2, ri(-2, 2, NIN) / 2
        x = ri(-2, 2, B, NIN, H, W)
        ext = ri(-2, 2, B, NIN, H, W) / 2 ** 20
        var, gs = torch.tensor([0.5, 2.0, 1.0, 4.0])[:NIN], 0.5
    mask = _mask(gen, B, mc, H, W)
    f = case["form"]
    return dict(d4=d4, w6=w6, b6=b6, x=x, mask=mask, var=var, gscale=gs if "g" in f else None, gdec_ext=ext if "e" in f else None)


# ======================================================================================================== latent tail
LT_GRID = 512
LT_MUTATIONS = ("stats_b_minus_512", "unbiased", "no_eps", "slab_wrong_patch")


def _lt_bn(v, e, gamma, beta, eps, mut=None):
    """Per-patch BatchNorm by hand (mean and biased variance over the patch's own 256 positions): v (B, C, H, W) with the
    standard deviation e of its error.  Returns y, its standard deviation, the (B, C, 2) sums and their bounds."""
    lo = v.dtype == torch.float32           # the fp32 evaluation: sums in double of the fp32 values, coefficients stored fp32
    v32, v, e = v, v.double(), e.double()
    n = v.shape[2] * v.shape[3]
    s1, s2 = v.sum((2, 3)), (v * v).sum((2, 3))
    b_s1 = K_SIGMA * torch.sqrt((e * e).sum((2, 3))) + F64_SLOP * v.abs().sum((2, 3))
    b_s2 = K_SIGMA * torch.sqrt((4 * v * v * e * e).sum((2, 3))) + K_SIGMA ** 2 * (e * e).sum((2, 3)) + F64_SLOP * s2
    sums, b_sums = torch.stack([s1, s2], -1), torch.stack([b_s1, b_s2], -1)
    u1, u2 = s1, s2
    if mut == "stats_b_minus_512" and v.shape[0] > LT_GRID:
        u1, u2 = s1.clone(), s2.clone()
        u1[LT_GRID:], u2[LT_GRID:] = s1[:-LT_GRID], s2[:-LT_GRID]
    mean = (u1 / n).reshape(*u1.shape, 1, 1)
    var = ((u2 / n).reshape(*u2.shape, 1, 1) - mean * mean).clamp(min=0)
    if mut == "unbiased":
        var = var * n / (n - 1)
    ve = var + (0.0 if mut == "no_eps" else f32(eps))
    invstd = 1.0 / torch.sqrt(ve)
    g = torch.ones(v.shape[1], dtype=torch.float64) if gamma is None else d(gamma)
    bt = torch.zeros(v.shape[1], dtype=torch.float64) if beta is None else d(beta)
    g, bt = g.reshape(1, -1, 1, 1), bt.reshape(1, -1, 1, 1)
    scale = g * invstd
    y = scale * (v - mean) + bt
    if lo:
        y = scale.float() * v32 + (bt.float() - mean.float() * scale.float())
    em2 = (e * e).mean((2, 3), keepdim=True) / n                                  # variance of the mean's error
    dvar2 = (4 * (v - mean) ** 2 * e * e).mean((2, 3), keepdim=True) / n           # ... of the variance's
    rel2 = 0.25 * dvar2 / (ve * ve)                                                # ... of invstd's, relative
    rnd = C_LT_BN * U * ((scale * v).abs() + bt.abs() + (mean * scale).abs())
    ey = torch.sqrt(scale * scale * (e * e + em2) + (scale * (v - mean)) ** 2 * rel2 + rnd * rnd)
    if mut == "slab_wrong_patch":
        sums = torch.roll(sums, 1, 0)
    return y, (ey.float() if lo else ey), sums, b_sums


def _lt_conv(t, e, w, b, cnt, **kw):
    W, Bv = d(w).to(t.dtype), (None if b is None else d(b).to(t.dtype))
    v = F.conv2d(t, W, Bv, **kw)
    var = F.conv2d(e * e + 0.5 * cnt * U * U * t * t, W * W, None if Bv is None else 0.5 * cnt * U * U * Bv * Bv, **kw)
    return v, torch.sqrt(var)


def latent_tail_ref(a3, coef3, w10, b10, gamma4, beta4, eps4, res, mut=None, dtype=torch.float64):
    """enc.10 .. enc.12 of EVERY patch of the batch at once, each BatchNorm with that patch's own statistics (by hand in
    float64, no loop of batch-of-one calls).  res: per residual layer (wa, ba, gamma_a, beta_a, eps_a, wb, bb, gamma_b,
    beta_b, eps_b), 0 .. 4 of them.
    Returns dict(z, b_z, stats=[(name, sums (B, C, 2), bound)]) in the order the wrapper returns the slabs: stats4, then
    (stats_a, stats_b) per residual layer."""
    stats = []
    A3, C3 = d(a3).to(dtype), d(coef3).to(dtype)
    c0, c2 = C3[:, :, 0, None, None], C3[:, :, 2, None, None]
    t, e = (c0 * A3 + c2).clamp(min=0), U * ((c0 * A3).abs() + c2.abs())
    v, e = _lt_conv(t, e, w10, b10, C_LT_CONV3, padding=1)
    h, eh, s, bs = _lt_bn(v, e, gamma4, beta4, eps4, mut)
    stats.append(("stats4", s, bs))
    for i, (wa, ba, ga, bea, epsa, wb, bb, gb, beb, epsb) in enumerate(res):
        v, e = _lt_conv(h.clamp(min=0), eh, wa, ba, C_LT_CONV3, padding=1)
        y, e, s, bs = _lt_bn(v, e, ga, bea, epsa, mut)
        stats.append((f"stats_a{i}", s, bs))
        v, e = _lt_conv(y.clamp(min=0), e, wb.reshape(16, 32, 1, 1), bb, C_LT_CONV1)
        y, e, s, bs = _lt_bn(v, e, gb, beb, epsb, mut)
        stats.append((f"stats_b{i}", s, bs))
        h = h + y
        eh = torch.sqrt(eh * eh + e * e + (U * h.abs()) ** 2)
    return dict(z=h, b_z=K_SIGMA * eh.double(), stats=stats)


LT_BATCHES = (1, 2, 511, 512, 513, 600, 1025)


def lt_cases():
    """B x nres 0 .. 4 (the grid is min(B, 512): 511 / 512 / 513 and 1025 lie around one and two full passes).  Every patch
    is compared."""
    return [(B, nres) for B in LT_BATCHES for nres in range(5)]


def lt_patch_scale(B):
    """Patch b is scaled by 4^((3 b mod 5) - 2): neighbours differ by up to 256, and patch b and patch b + 512 always
    differ (3 * 512 mod 5 = 1), so statistics or coefficients carried over from the previous pass cannot pass."""
    return 4.0 ** ((3 * torch.arange(B) % 5) - 2).double()


def lt_inputs(B, nres):
    """The kernel's arguments on the host.  The input channels get |mean| / std of 0, 3 and 30 (with_mean_over_std) and the
    patches scales from 1 / 16 to 16; a conv bias of the scale of the layer's spread keeps |mean| / std of the deeper layers
    around 1 .. 10; eps 1e-5 against variances down to ~1e-3 (the smallest patches)."""
    gen = torch.Generator().manual_seed(7000 + 10 * B + nres)
    C, CR = 16, 32
    r = lambda *s, k=1.0: torch.randn(*s, generator=gen) * k                              # noqa: E731
    scale = lt_patch_scale(B).float().reshape(B, 1, 1, 1)
    a = torch.randn(B, C, 16, 16, generator=gen)
    ratio = torch.tensor([0.0, 3.0, 30.0]).repeat(6)[:C].reshape(1, C, 1, 1)
    a = (with_mean_over_std(a, 0.0) + ratio) * scale
    # the on-load affine undoes most of the offset (as enc.8's BatchNorm would): c2 = -c0 mean + noise
    c0 = r(B, C).abs() + 0.5
    c2 = (-c0 * ratio.reshape(1, C) + r(B, C, k=0.3)) * scale.reshape(B, 1)
    coef = torch.stack([c0, torch.zeros(B, C), c2, torch.zeros(B, C)], 2).contiguous()
    bn = lambda n: (r(n).abs() + 0.5, r(n, k=0.3))                                         # noqa: E731
    w10, b10 = r(C, C, 3, 3, k=0.15), r(C, k=0.5)
    g4, be4 = bn(C)
    res = []
    for i in range(nres):
        ga, bea = bn(CR)
        gb, beb = bn(C)
        res.append((r(CR, C, 3, 3, k=0.15), r(CR, k=1.0 if i % 3 == 1 else 0.2), ga, bea, 1e-5,
                    r(C, CR, k=0.2), r(C, k=0.2), gb, beb, 1e-5))
    return dict(a3=a, coef3=coef, w10=w10, b10=b10, gamma4=g4, beta4=be4, eps4=1e-5, res=res)


# ================================================================================================= enc.0 o enc.1
def e1_compose_ref(w0, b0, w1):
    """Weff (C1, NIN + 1, 4, 4): enc.1's weights times enc.0's (C0, NIN) matrix, the last channel times enc.0's bias."""
    W0, B0, W1 = d(w0).reshape(w0.shape[0], -1), d(b0), d(w1)
    m = torch.cat([W0, B0.reshape(-1, 1)], 1)                                  # (C0, NIN + 1)
    weff = torch.einsum("ocyx,ci->oiyx", W1, m)
    mag = torch.einsum("ocyx,ci->oiyx", W1.abs(), m.abs())
    return weff, C_E1 * U * weff.abs() + F64_SLOP * mag


def e1_compose_border_ref(w0, b0, w1, b1, mut=None):
    """bias_border (3, 3, C1): b1 (None = 0) + the ones-channel weights of the taps inside the image per row / column class
    (class 0: the first output row / column misses ky / kx = 0; class 2: the last misses 3).
    mut 'no_b0_corner': enc.0's bias missing from class (0, 0)."""
    weff, _ = e1_compose_ref(w0, b0, w1)
    ones = weff[:, -1]                                                         # (C1, 4, 4)
    mag_all = torch.einsum("ocyx,c->oyx", d(w1).abs(), d(b0).abs())
    B1 = torch.zeros(ones.shape[0], dtype=torch.float64) if b1 is None else d(b1)
    table, mag = torch.zeros(3, 3, ones.shape[0], dtype=torch.float64), torch.zeros(3, 3, ones.shape[0], dtype=torch.float64)
    keep = {0: slice(1, 4), 1: slice(0, 4), 2: slice(0, 3)}
    for ry in range(3):
        for rx in range(3):
            table[ry, rx] = B1 + ones[:, keep[ry], keep[rx]].sum((1, 2))
            mag[ry, rx] = B1.abs() + mag_all[:, keep[ry], keep[rx]].sum((1, 2))
    if mut == "no_b0_corner":
        table[0, 0] = B1
    return table, C_E1 * U * table.abs() + F64_SLOP * mag


def e1_chain_ref(dweff, w0, b0, w1):
    """dW1 = dWeff . (W0 | b0)^T, (dW0 | db0) = sum over (c1, tap) of W1 dWeff -> dw0 (C0, NIN), db0 (C0), dw1 with bounds."""
    DW, W0, B0, W1 = d(dweff), d(w0).reshape(w0.shape[0], -1), d(b0), d(w1)
    m = torch.cat([W0, B0.reshape(-1, 1)], 1)
    dw1 = torch.einsum("oiyx,ci->ocyx", DW, m)
    dm = torch.einsum("ocyx,oiyx->ci", W1, DW)
    b = lambda v, mag: C_E1 * U * v.abs() + F64_SLOP * mag                                 # noqa: E731
    mag1, magm = torch.einsum("oiyx,ci->ocyx", DW.abs(), m.abs()), torch.einsum("ocyx,oiyx->ci", W1.abs(), DW.abs())
    return dict(dw0=dm[:, :-1], db0=dm[:, -1], dw1=dw1, b_dw0=b(dm, magm)[:, :-1], b_db0=b(dm, magm)[:, -1], b_dw1=b(dw1, mag1))


# enc.0 is Conv2d(NIN, C0, 1) and enc.1 Conv2d(C0, C1, 4, 2, 1) with C0 = num_hiddens // 2, C1 = num_hiddens (engine.py hands
# the stored parameters over as they are): num_hiddens 16, 32, 64 x NIN 1 .. 4
E1_SHAPES = [(nin, nh // 2, nh) for nh in (16, 32, 64) for nin in (1, 2, 3, 4)]


def e1_inputs(NIN, C0, C1, kind, seed):
    """kind 'dyadic': weights in eighths within +-1 (sums of at most 32 * 16 products of 3-bit numbers: exact in double AND
    after the one fp32 store); 'randn': unit scale."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "dyadic":
        ri = lambda *s: torch.randint(-8, 9, s, generator=gen).float() / 8                 # noqa: E731
        return ri(C0, NIN, 1, 1), ri(C0), ri(C1, C0, 4, 4), ri(C1), ri(C1, NIN + 1, 4, 4)
    r = lambda *s: torch.randn(*s, generator=gen)                                          # noqa: E731
    return r(C0, NIN, 1, 1), r(C0), r(C1, C0, 4, 4) * 0.2, r(C1), r(C1, NIN + 1, 4, 4)
