"""The wide family's persistent streaming kernels where a walker (a wave, or a workgroup that walks together) takes several
units: one table of cases and the pure functions the host test (tests/test_stream_walk_host.py) and the GPU test
(tests/test_gpu_stream_walk.py) share.

csrc/wide_stream.hip's ten kernels and wgrad_wide1_kernel (csrc/conv_wide.hip) carry state from one unit to the next: the
next unit's operand loads are requested inside the current unit's K loop, border flags and row offsets are computed one unit
ahead, the gate of the next unit is requested after this unit's epilogue, the two streaming weight gradients keep a register
ring of `ring` stages in flight across sample boundaries, the fused 1x1 backward accumulates dW and statistics over all of a
wave's units.  The launch plan (ops.*_plan: dm_conv4x4s2_plan / dm_conv3x3_plan / dm_wgrad_plan / dm_conv1x1_bwd_fused_plan,
host only, the decision code the launches themselves read) says which kernel a call runs and how its units are dealt; both
tests assert conditions() from it, so a later change of a grid cap cannot quietly turn these cases back into one-unit tests.

Planes are the smallest each kernel accepts, so the batch carries the unit count and no tensor is large:
  kernel                     plane              B      units   dealt to                      units per walker
  conv1x1_stream             8 x 16             2600   5200    512 workgroups x 4 waves      2-3
  conv_s2_thin_stream        16 x 128 in        800    6400    768 x 4                       2-3
  convT_thin_stream          8 x 64             4100   8200    1024 x 4, grid-strided        2-3
  conv_s2_wide_stream        64 x 64 in         300    4800    256 x 8                       2-3
  convT_wide / conv3x3_wide  32 x 32            300    4800    256 x 8                       2-3
  conv1x1_bwd_wide_stream    8 x 16             2600   5200    512 x 4, a range per wave     2-3
  wgrad1x1_stream            8 x 16             1100   4400    768 workgroups                5-6 stages (ring 2)
  wgrad_s2_thin_stream       8 x 32 (S grid)    2000   16000   768 x 4, a range per wave     5-6 stages (ring 1)
  wgrad_wide1                8 x 16 (S grid)    800    800     256 workgroups, grid-strided  3-4

Border units.  The request for these cases was for ONE wave to walk a top-border, an interior and a bottom-border unit.
No launch of these kernels can do that: a walker's units are a fixed stride apart (4 or 8 inside a workgroup's range, the whole
grid for convT_thin_stream), the units of a sample are a multiple of that stride or share a factor 2 with it (8 output rows
and stride 4; 16 two-row units and stride 8; H / 4 even and an even grid), so a walker only ever sees two residues -- r and
r + stride -- and the top unit (residue 0) and the bottom unit (residue -1) never meet in one walker.  What can go wrong in the
carried flags is a flag that arrives one unit late or sticks, and that shows wherever a flag CHANGES between consecutive
units of one walker; so conditions() asks, per kernel with carried border state, for a walker whose consecutive units go
top -> interior, one that goes interior -> top, and the same two for the bottom border.  convT_thin_stream carries no
border state (it computes its rows per unit) and its walkers keep their residue: there the three classes must all occur in
the launch.
"""
import collections

# dm_launch_plan's `kernel` and `dealing` (include/dynamorph_hip.h); the host test checks them against dynamorph_amd._lib
KERNELS = dict(resident=0, patch=1, wide_tiled=2, generic=3, conv1x1_bwd_tiled=4, conv1x1_stream=16, conv_s2_thin_stream=17,
               convT_thin_stream=18, conv_s2_wide_stream=19, convT_wide_stream=20, conv3x3_wide_stream=21,
               conv1x1_bwd_wide_stream=22, wgrad1x1_stream=23, wgrad_s2_thin_stream=24, wgrad_wide1=25)
DEAL_RANGE_STRIDED, DEAL_RANGE, DEAL_GRID_STRIDED = 1, 2, 3
IDENT, RELU, AFFINE, AFFINE_RELU, AFFINE2 = range(5)

# api: "conv4" (ops.conv4x4s2), "conv3" (ops.conv3x3, k = taps), "convT" (ops.conv3x3 with pixel_shuffle; b = output channels),
# "wgrad" (ops.wgrad; a, b = S, T channels; h, w = the S grid; mode, mode2 = S, T operand modes), "bwd1x1" (ops.conv1x1_bwd_fused)
# epi: "none", "stats", "bias+stats", "gate+q" (AFFINE gate whose tensor is also stat_q), "bias+relu+resid",
#      "all" (gate, residual, statistics against a third tensor)
Case = collections.namedtuple("Case", "kernel api B a b h w k mode mode2 epi")


def _cases():
    out = []
    # 1x1: forward (BatchNorm + ReLU on the load, statistics; ring of 8), data gradient (AFFINE2, transposed view, gate,
    # statistics against the gate's tensor; ring of 4), both for all four channel pairs; bias + ReLU + residual
    for cin, nout in ((64, 64), (32, 64), (64, 32), (32, 32)):
        out.append(Case("conv1x1_stream", "conv3", 2600, cin, nout, 8, 16, 1, AFFINE_RELU, None, "stats"))
        out.append(Case("conv1x1_stream", "conv3", 2600, cin, nout, 8, 16, 1, AFFINE2, None, "gate+q"))
    out.append(Case("conv1x1_stream", "conv3", 2600, 64, 64, 8, 16, 1, IDENT, None, "bias+relu+resid"))
    out.append(Case("conv1x1_stream", "conv3", 2600, 32, 32, 8, 16, 1, AFFINE2, None, "bias+relu+resid"))
    # 4x4 / stride 2 from the image side
    for cin, nout, mode, epi in ((1, 32, IDENT, "bias+stats"), (2, 32, IDENT, "gate+q"), (3, 32, AFFINE_RELU, "bias+stats"),
                                 (4, 32, RELU, "gate+q"), (2, 64, AFFINE, "bias+stats"), (2, 64, IDENT, "gate+q")):
        out.append(Case("conv_s2_thin_stream", "conv4", 800, cin, nout, 16, 128, 16, mode, None, epi))
    # the last transposed convolution (channel counts no register-resident kernel takes: 8 -> 1 / 2 is one of theirs)
    out.append(Case("convT_thin_stream", "convT", 4100, 12, 1, 8, 64, 9, AFFINE_RELU, None, "none"))
    out.append(Case("convT_thin_stream", "convT", 4100, 24, 2, 8, 64, 9, IDENT, None, "none"))
    # the three weights-in-LDS kernels
    out.append(Case("conv_s2_wide_stream", "conv4", 300, 32, 64, 64, 64, 16, IDENT, None, "none"))
    out.append(Case("conv_s2_wide_stream", "conv4", 300, 32, 64, 64, 64, 16, AFFINE_RELU, None, "bias+stats"))
    out.append(Case("conv_s2_wide_stream", "conv4", 300, 32, 64, 64, 64, 16, AFFINE2, None, "gate+q"))
    out.append(Case("convT_wide_stream", "convT", 300, 64, 32, 32, 32, 9, IDENT, None, "bias+stats"))
    out.append(Case("convT_wide_stream", "convT", 300, 64, 32, 32, 32, 9, AFFINE2, None, "gate+q"))
    out.append(Case("conv3x3_wide_stream", "conv3", 300, 64, 64, 32, 32, 9, RELU, None, "stats"))
    out.append(Case("conv3x3_wide_stream", "conv3", 300, 64, 64, 32, 32, 9, AFFINE2, None, "all"))      # data-gradient form
    # fused backward of the 1x1 layer, 64 -> 64
    out.append(Case("conv1x1_bwd_wide_stream", "bwd1x1", 2600, 64, 64, 8, 16, 1, AFFINE2, None, None))
    out.append(Case("conv1x1_bwd_wide_stream", "bwd1x1", 2600, 64, 64, 8, 16, 1, IDENT, None, None))
    # weight gradients
    for cs, ct in ((64, 64), (64, 32), (32, 64), (32, 32)):
        out.append(Case("wgrad1x1_stream", "wgrad", 1100, cs, ct, 8, 16, 1, AFFINE2, AFFINE_RELU, None))
        out.append(Case("wgrad1x1_stream", "wgrad", 1100, cs, ct, 8, 16, 1, RELU, IDENT, None))
    for cs, ct, sm, tm in ((32, 1, AFFINE2, IDENT), (32, 2, AFFINE_RELU, IDENT), (32, 3, AFFINE2, AFFINE_RELU), (16, 4, IDENT, RELU),
                           (64, 1, AFFINE2, AFFINE)):
        out.append(Case("wgrad_s2_thin_stream", "wgrad", 2000, cs, ct, 8, 32, 4, sm, tm, None))
    out.append(Case("wgrad_wide1", "wgrad", 800, 64, 64, 8, 16, 3, AFFINE2, RELU, None))
    out.append(Case("wgrad_wide1", "wgrad", 800, 64, 64, 8, 16, 3, IDENT, AFFINE_RELU, None))
    out.append(Case("wgrad_wide1", "wgrad", 800, 64, 32, 8, 16, 4, AFFINE2, IDENT, None))
    out.append(Case("wgrad_wide1", "wgrad", 800, 64, 32, 8, 16, 4, IDENT, AFFINE2, None))
    return out


CASES = _cases()
CONV_CASES = [c for c in CASES if c.api in ("conv4", "conv3", "convT")]
BWD_CASES = [c for c in CASES if c.api == "bwd1x1"]
WGRAD_CASES = [c for c in CASES if c.api == "wgrad"]


def case_id(c):
    m = f"m{c.mode}" + (f"t{c.mode2}" if c.mode2 is not None else "")
    return f"{c.kernel}-{c.a}x{c.b}-k{c.k}-{c.h}x{c.w}-B{c.B}-{m}" + (f"-{c.epi}" if c.epi else "")


def epilogue_flags(c):
    """The epilogue of a convolution case as ops.*_plan takes it: True stands for a tensor, mask is the gate's mode."""
    gate_mode = IDENT if c.kernel == "conv3x3_wide_stream" else AFFINE
    return {"none": {}, "stats": dict(stats=True), "bias+stats": dict(bias=True, stats=True),
            "gate+q": dict(mask=gate_mode, stat_q="gate", stats=True), "bias+relu+resid": dict(bias=True, relu=True, resid=True),
            "all": dict(mask=gate_mode, resid=True, stat_q=True, stats=True)}[c.epi]


def plan(ops, c, B=None):
    """The launch plan of the case (of a batch of B samples of it), described by modes and flags alone."""
    B = c.B if B is None else B
    if c.api == "conv4":
        return ops.conv4x4s2_plan(c.mode, B, c.a, c.b, c.h, c.w, **epilogue_flags(c))
    if c.api == "conv3":
        return ops.conv3x3_plan(c.mode, B, c.a, c.b, c.h, c.w, taps=c.k, **epilogue_flags(c))
    if c.api == "convT":
        return ops.conv3x3_plan(c.mode, B, c.a, 4 * c.b, c.h, c.w, taps=9, pixel_shuffle=True, **epilogue_flags(c))
    if c.api == "wgrad":
        return ops.wgrad_plan(c.mode, c.mode2, B, c.a, c.b, c.h, c.w, c.k)
    return ops.conv1x1_bwd_fused_plan(c.mode, B, c.a, c.b, c.h, c.w)


# ---- the walk: a plain restatement of "units of walker j of workgroup g" for the three dealing forms -----------------------
def walkers(p):
    return p.workgroups * p.walkers


def walker_units(p, v):
    """Units of walker v (walker j of workgroup g is v = g * p.walkers + j), in the order it takes them."""
    G, J, U = p.workgroups, p.walkers, p.units
    g, j = divmod(v, J)
    if p.dealing == DEAL_RANGE_STRIDED:         # the workgroup's contiguous range, dealt round-robin to its walkers
        return range(U * g // G + j, U * (g + 1) // G, J)
    if p.dealing == DEAL_RANGE:                 # a contiguous range per walker
        return range(U * v // (G * J), U * (v + 1) // (G * J))
    assert p.dealing == DEAL_GRID_STRIDED, p
    return range(v, U, G * J)


def max_units_per_walker(p):
    return max(len(walker_units(p, v)) for v in range(walkers(p)))


def units_per_sample(c, p):
    assert p.units % c.B == 0
    return p.units // c.B


# kernels whose units differ by border: unit r of a sample's n is a top-border unit when r == 0, a bottom-border one when r == n - 1
BORDER_KERNELS = ("conv_s2_thin_stream", "convT_thin_stream", "conv_s2_wide_stream", "convT_wide_stream", "conv3x3_wide_stream")
CARRIES_BORDER_STATE = ("conv_s2_thin_stream", "conv_s2_wide_stream", "convT_wide_stream", "conv3x3_wide_stream")


def border_class(r, n):
    return "top" if r == 0 else ("bottom" if r == n - 1 else "interior")


def conditions(c, p):
    """What makes a case a case (see the module docstring for the border conditions)."""
    cid = case_id(c)
    assert p.kernel == KERNELS[c.kernel], (cid, p)
    V = walkers(p)
    walks = [walker_units(p, v) for v in range(V)]
    assert sorted(u for w in walks for u in w) == list(range(p.units)), cid            # every unit once
    counts = [len(w) for w in walks if len(w)]
    assert min(counts) >= 2 and max(counts) >= 3, (cid, min(counts), max(counts))
    dealt_among = p.workgroups if p.dealing == DEAL_RANGE_STRIDED else V
    assert p.units % dealt_among != 0, (cid, p.units, dealt_among)                      # ranges of unequal length
    ups = units_per_sample(c, p)
    assert any(w[0] // ups != w[-1] // ups for w in walks if len(w)), cid             # a walk crosses a sample boundary
    if c.kernel in BORDER_KERNELS:
        assert ups >= 2
        steps = {(border_class(a % ups, ups), border_class(b % ups, ups)) for w in walks for a, b in zip(w, w[1:])}
        if c.kernel in CARRIES_BORDER_STATE:
            for need in (("top", "interior"), ("interior", "top"), ("bottom", "interior"), ("interior", "bottom")):
                assert need in steps, (cid, need, sorted(steps))
        else:
            classes = {border_class(u % ups, ups) for w in walks for u in w}
            assert {"top", "bottom"} <= classes, (cid, classes)
    if p.ring:
        assert max(counts) >= 2 * p.ring + 1, (cid, max(counts), p.ring)              # every ring slot refills twice
    else:
        assert c.kernel not in ("wgrad1x1_stream", "wgrad_s2_thin_stream"), cid


def slice_batch(ops, c):
    """Largest batch (up to the case's) whose launch runs the same kernel with at most one unit per walker: the regime the
    float64 kernel tests of tests/test_gpu_kernels.py cover."""
    lo, hi = 1, c.B                       # (units per walker grow with the batch)
    assert max_units_per_walker(plan(ops, c, 1)) <= 1, case_id(c)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if max_units_per_walker(plan(ops, c, mid)) <= 1:
            lo = mid
        else:
            hi = mid - 1
    return lo


def slices(B, per):
    """Consecutive batch slices [b0, b1) of at most `per` samples each, covering [0, B)."""
    return [(b0, min(B, b0 + per)) for b0 in range(0, B, per)]


def reference_samples(c, p):
    """The samples held to float64: the first, the one in which workgroup 0 / walker 0's second unit lies (often the first
    again: a sample has 2 to 16 units), the one in which the middle walker's second unit lies, the last."""
    ups = units_per_sample(c, p)
    return sorted({0, walker_units(p, 0)[1] // ups, walker_units(p, walkers(p) // 2)[1] // ups, c.B - 1})


# ---- existing cases of tests/test_gpu_kernels.py filed under "stream" tests: the kernel each really runs -------------------
# (B, cin, nout, h, w, mode, epi) of test_stream_conv_4x4s2_few_input_channels; (B, ci, co, h, mode, relu) of
# test_stream_conv_transpose_to_few_channels.  H / 2 (or H) not a multiple of 8: no wide tiling, the generic kernel;
# 1 -> 16 channels at H = 16: a register-resident kernel.
OLD_S2_THIN = {(3, 2, 32, 128, 128, 0, "bias"): "conv_s2_thin_stream", (2, 2, 32, 128, 128, 0, "gate+q"): "conv_s2_thin_stream",
               (2, 1, 16, 16, 128, 3, "all"): "resident", (2, 4, 32, 8, 128, 1, "gate"): "generic",
               (1, 3, 16, 4, 128, 3, "all"): "generic", (20, 2, 64, 32, 128, 0, "bias"): "conv_s2_thin_stream",
               (2, 2, 32, 6, 128, 2, "none"): "generic",
               # the nearest wide-tileable shapes that do reach the streaming kernel (rows 0 and OH - 1 of an 8-row output)
               (2, 4, 32, 16, 128, 1, "gate"): "conv_s2_thin_stream", (1, 3, 32, 16, 128, 3, "all"): "conv_s2_thin_stream",
               (2, 2, 32, 16, 128, 2, "none"): "conv_s2_thin_stream", (2, 1, 32, 16, 128, 3, "all"): "conv_s2_thin_stream"}
OLD_CONVT_THIN = {(3, 32, 2, 64, 3, False): "convT_thin_stream", (2, 32, 1, 8, 0, True): "convT_thin_stream",
                  (5, 64, 2, 16, 1, False): "convT_thin_stream", (1, 8, 2, 4, 2, False): "generic",
                  (2, 17, 2, 12, 3, True): "generic", (70, 32, 2, 64, 3, False): "convT_thin_stream",
                  (1, 12, 2, 8, 2, False): "convT_thin_stream", (2, 17, 2, 16, 3, True): "convT_thin_stream"}
