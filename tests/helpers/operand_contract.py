"""The operand / epilogue contract of include/dynamorph_hip.h as data: a table of the routes behind dm_conv4x4s2, dm_conv3x3,
dm_wgrad and dm_apply, the cases each route is asked to honour or refuse, a float64 reference of every case, an
accumulation-error bound, and the mutated references a kernel that silently ignored a feature would produce.

Pure CPU (torch on the host, no torch.cuda): tests/test_operand_contract_host.py checks the table and that every mutation is
visible; tests/test_gpu_operand_contract.py runs the cases on the device (tests/helpers/operand_contract_run.py).

Arithmetic restated from the header:
  load     IDENT p0 | RELU max(p0,0) | AFFINE c0 p0 + c2 | AFFINE_RELU max(c0 p0 + c2, 0) | AFFINE2 c0 p0 + c1 p1 + c2,
           coefficients [C][4] or [B][C][4] (coef_bstride = 4 C); a ones channel is 1 inside the image, 0 in the padding
  epilogue v = acc + bias (or bias_border[row class][column class]); relu; mask: c0 m + c2 > 0 on the raw mask (IDENT:
           m > 0); + resid; stats (sum v, sum v q), q = stat_q raw or v, one slab set per sample when per_tile
  wgrad    R[cs][ct][ky][kx] = sum_{b,y,x} S[b,cs,y,x] T[b,ct,y s+ky-p,x s+kx-p]
"""
import math
import random
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

U = 2.0 ** -24
C_BOUND = 16.0          # the bound's constant, one value for every route
MUTATION_MARGIN = 20.0  # every mutation must miss the true reference by this many bounds somewhere
SENTINEL = 12345.0      # value of the slab past the declared ones


# ------------------------------------------------------------------------------------------------------------ routes
@dataclass(frozen=True)
class Route:
    name: str
    entry: str            # s2 (dm_conv4x4s2) | s1 (dm_conv3x3) | pix (dm_conv3x3 pixel shuffle) | wgrad | apply
    kernel: str           # kernel template the BASE case launches (rocprofv3 name prefix); a feature the kernel's guard
                          # declines takes the entry's next route, so a feature case checks the entry at this shape
    shape: tuple          # s2/s1/pix: (B, CIN, NOUT, H, W, taps); wgrad: (B, CS, CT, Hs, Ws, k); apply: (B, C, H, W)
    scratch: bool = True  # False: a weight view without scratch (the generic kernels)
    env: str = ""         # "tiled": run in a child process with DM_WIDE_STREAM=0 DM_WIDE_WGRAD1=0
    base: tuple = ()      # features every case of the route carries (the border-bias and pair forms)


TILED_ENV = {"DM_WIDE_STREAM": "0", "DM_WIDE_WGRAD1": "0"}

ROUTES = [
    # ---- dm_conv4x4s2 ----------------------------------------------------------------------------------------------
    Route("s2_patch16", "s2", "conv4x4s2_patch_forward_kernel", (2, 16, 16, 32, 32, 16)),
    Route("s2_conv4_c1", "s2", "conv4x4s2_kernel<1,", (2, 1, 8, 128, 128, 16)),
    Route("s2_conv4_c2", "s2", "conv4x4s2_kernel<2,", (2, 2, 8, 64, 128, 16)),
    Route("s2_conv4_c3", "s2", "conv4x4s2_kernel<3,", (2, 3, 16, 64, 64, 16)),
    Route("s2_conv4_c4", "s2", "conv4x4s2_kernel<4,", (2, 4, 8, 32, 64, 16)),
    Route("s2_conv4_c5", "s2", "conv4x4s2_kernel<5,", (2, 5, 8, 64, 128, 16)),
    Route("s2_conv4_c8", "s2", "conv4x4s2_kernel<8,", (2, 8, 16, 32, 64, 16)),
    Route("s2_conv4_c16", "s2", "conv4x4s2_kernel<16,", (2, 16, 16, 64, 64, 16)),
    Route("s2_conv4_border", "s2", "conv4x4s2_kernel<3,", (2, 3, 16, 32, 128, 16), base=("border",)),
    Route("s2_conv4_pair", "s2", "conv4x4s2_pair_kernel", (2, 3, 8, 32, 128, 16), base=("border",)),
    Route("s2_stream_wide", "s2", "conv_s2_wide_stream_kernel", (2, 32, 64, 64, 64, 16)),
    Route("s2_stream_thin", "s2", "conv_s2_thin_stream_kernel", (2, 2, 32, 32, 128, 16)),
    Route("s2_wide", "s2", "conv_wide_kernel<0,", (2, 24, 40, 32, 32, 16)),
    Route("s2_wide_tiled", "s2", "conv_wide_kernel<0,", (2, 32, 64, 64, 64, 16), env="tiled"),
    Route("s2_generic", "s2", "conv_generic_kernel<0", (2, 24, 20, 20, 36, 16), scratch=False),
    # ---- dm_conv3x3 ------------------------------------------------------------------------------------------------
    Route("pix_convT_phase", "pix", "convT_phase_kernel", (2, 16, 32, 16, 16, 9)),
    Route("s1_conv3_c16", "s1", "conv3x3_kernel<16, 1, 1, 9, false", (2, 16, 16, 16, 16, 9)),
    Route("s1_conv3_c16n2", "s1", "conv3x3_kernel<16, 2, 1, 9, false", (2, 16, 32, 16, 32, 9)),
    Route("s1_conv3_c32", "s1", "conv3x3_kernel<32, 1, 1, 9, false", (2, 32, 16, 16, 16, 9)),
    Route("s1_conv1_c32", "s1", "conv3x3_kernel<32, 1, 1, 1, false", (2, 32, 16, 16, 16, 1)),
    Route("s1_conv1_c16", "s1", "conv3x3_kernel<16, 2, 1, 1, false", (2, 16, 32, 16, 32, 1)),
    Route("pix_conv3_c16n4", "pix", "conv3x3_kernel<16, 2, 2, 9, true", (2, 16, 64, 16, 16, 9), base=("per_tile",)),
    Route("pix_conv3_c8", "pix", "conv3x3_kernel<8, 1, 1, 9, true", (2, 8, 16, 16, 64, 9)),
    Route("pix_conv3_c4", "pix", "conv3x3_kernel<4, 1, 1, 9, true", (2, 4, 16, 8, 64, 9)),
    Route("s1_stream_3x3", "s1", "conv3x3_wide_stream_kernel", (2, 64, 64, 32, 32, 9)),
    Route("pix_stream_convT", "pix", "convT_wide_stream_kernel", (2, 64, 128, 32, 32, 9)),
    Route("pix_stream_thin", "pix", "convT_thin_stream_kernel", (2, 16, 8, 16, 64, 9)),
    Route("s1_stream_1x1", "s1", "conv1x1_stream_kernel", (2, 64, 64, 32, 32, 1)),
    Route("s1_wide", "s1", "conv_wide_kernel<1,", (2, 48, 24, 16, 16, 9)),
    Route("s1_wide_1x1", "s1", "conv_wide_kernel<1,", (2, 40, 24, 16, 32, 1)),
    Route("pix_wide", "pix", "conv_wide_kernel<2,", (2, 24, 48, 16, 16, 9)),
    Route("s1_wide_tiled", "s1", "conv_wide_kernel<1,", (2, 64, 64, 32, 32, 9), env="tiled"),
    Route("pix_wide_tiled", "pix", "conv_wide_kernel<2,", (2, 64, 128, 32, 32, 9), env="tiled"),
    Route("s1_generic", "s1", "conv_generic_kernel<1", (2, 24, 20, 12, 20, 9), scratch=False),
    Route("pix_generic", "pix", "conv_generic_kernel<2", (2, 12, 24, 12, 20, 9), scratch=False),
    # ---- dm_wgrad --------------------------------------------------------------------------------------------------
    Route("wg_8x3_k4", "wgrad", "wgrad_ys_kernel<3,", (2, 8, 3, 16, 64, 4)),
    Route("wg_16x8_k4", "wgrad", "wgrad_kernel<16, 8, 4", (2, 16, 8, 16, 32, 4)),
    Route("wg_4x4_k4", "wgrad", "wgrad_kernel<4, 4, 4,", (2, 4, 4, 8, 64, 4)),
    Route("wg_16x16_k3", "wgrad", "wgrad_kernel<16, 16, 3", (2, 16, 16, 16, 16, 3)),
    Route("wg_32x16_k3", "wgrad", "wgrad_kernel<32, 16, 3", (2, 32, 16, 16, 16, 3)),
    Route("wg_16x32_k1", "wgrad", "wgrad_kernel<16, 32, 1", (2, 16, 32, 16, 16, 1)),
    Route("wg_stream_1x1", "wgrad", "wgrad1x1_stream_kernel", (2, 64, 64, 16, 16, 1)),
    Route("wg_stream_s2_thin", "wgrad", "wgrad_s2_thin_stream_kernel", (2, 16, 2, 16, 32, 4)),
    Route("wg_wide1_k3", "wgrad", "wgrad_wide1_kernel<3, 64", (2, 64, 64, 16, 16, 3)),
    Route("wg_wide1_k4", "wgrad", "wgrad_wide1_kernel<4, 32", (2, 64, 32, 16, 16, 4)),
    Route("wg_wide1_t_affine2", "wgrad", "wgrad_wide1_kernel<4, 32, false, true>", (2, 64, 32, 16, 16, 4),
          base=("tmode4",)),
    Route("wg_wide_k4", "wgrad", "wgrad_wide_kernel<4>", (2, 24, 12, 16, 16, 4)),
    Route("wg_wide_k3", "wgrad", "wgrad_wide_kernel<3>", (2, 48, 24, 16, 16, 3)),
    Route("wg_wide_k1", "wgrad", "wgrad_wide_kernel<1>", (2, 48, 40, 16, 16, 1)),
    Route("wg_wide_tiled_k3", "wgrad", "wgrad_wide_kernel<3>", (2, 64, 64, 16, 16, 3), env="tiled"),
    Route("wg_wide_tiled_1x1", "wgrad", "wgrad_wide_kernel<1>", (2, 64, 64, 16, 16, 1), env="tiled"),
    Route("wg_generic", "wgrad", "wgrad_generic_kernel", (2, 8, 6, 10, 12, 3)),
    # ---- dm_apply --------------------------------------------------------------------------------------------------
    Route("apply", "apply", "apply_kernel", (2, 16, 16, 16)),
]

# One base case per register-resident table row (DM_CONV4_ROWS, DM_CONVT_PHASE_ROWS, DM_CONV3_ROWS in conv_mfma.hip,
# DM_WGRAD_ROWS in wgrad_mfma.hip) that no route above selects, at the smallest shape that does: two samples of one tile,
# as wide as the row's tile.  (The rows with 64-wide tiles from 16 channels and 32-wide tiles from 32 channels cannot be
# selected by any shape: conv3_tw caps those widths at 32 and 16.)
def _row(name, entry, kernel, shape, base=()):
    return Route("row_" + name, entry, kernel, shape, base=base)


ROW_ROUTES = (
    # dm_conv4x4s2, row (CIN, TW): output of 8 x TW
    [_row(f"s2_c{c}_tw{tw}", "s2", f"conv4x4s2_kernel<{c},", (2, c, 16 if c == 8 else 8, 16, 2 * tw, 16))
     for c, tw in ((3, 16), (4, 64), (4, 16), (5, 32), (5, 16), (2, 32), (2, 16), (1, 32), (1, 16), (8, 16))]
    # dm_conv3x3 pixel shuffle on the phase kernel, row (COUT, TW): 16 rows with 16-wide tiles, else 8
    + [_row(f"convT_phase_co{co}_tw{tw}", "pix", f"convT_phase_kernel<16, {co},", (2, 16, 4 * co, 16 if tw == 16 else 8, tw, 9))
       for co, tw in ((8, 32), (16, 16), (16, 32))]
    # dm_conv3x3, row (CIN, NTOT, taps, pix, TW); the 16-channel pixel-shuffle rows are reached with per-tile statistics only
    + [_row("s1_c16_tw32", "s1", "conv3x3_kernel<16, 1, 1, 9, false", (2, 16, 16, 8, 32, 9)),
       _row("s1_c16n2_tw16", "s1", "conv3x3_kernel<16, 2, 1, 9, false", (2, 16, 32, 16, 16, 9)),
       _row("s1_1x1_c16n2_tw16", "s1", "conv3x3_kernel<16, 2, 1, 1, false", (2, 16, 32, 16, 16, 1)),
       _row("pix_c16n2_tw32", "pix", "conv3x3_kernel<16, 2, 1, 9, true", (2, 16, 32, 8, 32, 9), base=("per_tile",)),
       _row("pix_c16n4_tw32", "pix", "conv3x3_kernel<16, 2, 2, 9, true", (2, 16, 64, 8, 32, 9), base=("per_tile",)),
       _row("pix_c8_tw32", "pix", "conv3x3_kernel<8, 1, 1, 9, true", (2, 8, 16, 8, 32, 9))]
    # dm_wgrad, row (CS, CT, k, TW): S grid of 8 x TW
    + [_row(f"wg_{cs}x{ct}_k{k}_tw{tw}", "wgrad", ("wgrad_ys_kernel<%d," % ct) if cs == 8 else f"wgrad_kernel<{cs}, {ct}, {k}",
            (2, cs, ct, 8, tw, k))
       for cs, ct, k, tw in ((8, 3, 4, 32), (8, 3, 4, 16), (8, 5, 4, 64), (8, 2, 4, 64), (8, 4, 4, 64), (8, 1, 4, 64),
                             (16, 8, 4, 64), (16, 8, 4, 16), (16, 16, 4, 16), (16, 16, 4, 32), (16, 16, 3, 32),
                             (32, 16, 3, 32), (16, 32, 1, 32), (8, 4, 4, 32))]
)
ROUTE = {r.name: r for r in ROUTES + ROW_ROUTES}

# ---------------------------------------------------------------------------------------------------------- features
MODES = ("mode0", "mode1", "mode2", "mode3", "mode4")
CONV_EPI = ("bias", "relu", "mask_id", "mask_aff", "mask_aff_ps", "resid", "stats", "stat_q", "stat_q_mask", "per_tile")
CONV_FEATURES = MODES + ("ps", "view") + CONV_EPI
S2_FEATURES = CONV_FEATURES + ("ones", "border")
WG_FEATURES = ("smode1", "smode2", "smode3", "smode4", "sps", "tmode1", "tmode2", "tmode3", "tmode4", "tps", "tones")
APPLY_FEATURES = MODES + ("ps", "resid")
# asked of every route of the entry, expected to be refused before any launch
_MASK_REFUSED = {"mask_ones": "a mask with a ones channel", "mask_relu": "a RELU mask",
                 "mask_affine_relu": "an AFFINE_RELU mask", "mask_affine2": "an AFFINE2 mask"}
REFUSED = {
    "s2": dict(_MASK_REFUSED),
    "s1": {"ones": "dm_conv3x3 takes no ones channel", "border": "bias_border is dm_conv4x4s2 only", **_MASK_REFUSED},
    "pix": {"ones": "dm_conv3x3 takes no ones channel", "border": "bias_border is dm_conv4x4s2 only", **_MASK_REFUSED},
    "wgrad": {"sones": "S cannot carry a ones channel"},
    "apply": {"ones": "dm_apply takes no ones channel"},
}


def entry_features(entry):
    return {"s2": S2_FEATURES, "s1": CONV_FEATURES, "pix": CONV_FEATURES, "wgrad": WG_FEATURES,
            "apply": APPLY_FEATURES}[entry]


def t_affine2_route(route):
    """dm_wgrad_t_affine2_supported: the one-pass kernel's 64 x 32, k = 4 shape, with the one-pass kernels switched on."""
    return route.entry == "wgrad" and route.shape[1:3] == (64, 32) and route.shape[5] == 4 and route.env != "tiled"


def normalize(route, feats):
    """Implied features: one operand mode, stats under stat_q / per_tile, a mask under stat_q_mask, bias_border replaces
    bias, per-sample coefficients only with an AFFINE* mode; T = AFFINE2 only on the route built for it."""
    f = set(route.base) | set(feats)
    if route.entry == "wgrad":
        if "tmode4" in f and not t_affine2_route(route):
            f.discard("tps")       # refused anyway; keep the case minimal
        if "sps" in f and not any(m in f for m in ("smode2", "smode3", "smode4")):
            f.add("smode2")
        if "tps" in f and not any(m in f for m in ("tmode2", "tmode3", "tmode4")):
            f.add("tmode2")
        for side in "st":
            ms = sorted(m for m in f if m.startswith(side + "mode"))
            for m in ms[:-1]:
                f.discard(m)
        if "tmode4" in f:
            f.discard("tones")
        return frozenset(f)
    modes = sorted(m for m in f if m in MODES)
    for m in modes[:-1]:
        f.discard(m)
    if "ps" in f and not any(m in f for m in ("mode2", "mode3", "mode4")):
        f.add("mode2")
    if not any(m in f for m in MODES):
        f.add("mode0")
    if f & {"stat_q", "stat_q_mask", "per_tile"}:
        f.add("stats")
    if "stat_q_mask" in f:
        f.discard("stat_q")
        if not f & {"mask_id", "mask_aff", "mask_aff_ps"}:
            f.add("mask_id")
    masks = sorted(m for m in f if m in ("mask_id", "mask_aff", "mask_aff_ps"))
    for m in masks[:-1]:
        f.discard(m)
    if "border" in f:
        f.discard("bias")
    if "ones" in f and route.shape[1] == 1:
        f.discard("ones")
    return frozenset(f)


@dataclass(frozen=True)
class Case:
    route: str
    feats: frozenset
    B: int
    expect: str           # "match" | "refuse"
    why: str = ""

    @property
    def id(self):
        fs = "+".join(sorted(self.feats)) or "base"
        return f"{self.route}-B{self.B}-{fs}"


def expect_of(route, feats):
    """("refuse", why) where the header or a DM_REQUIRE turns the call away, else ("match", "")."""
    for k, why in REFUSED[route.entry].items():
        if k in feats:
            return "refuse", why
    if route.entry == "wgrad" and "tmode4" in feats:
        if not t_affine2_route(route):
            return "refuse", "T = AFFINE2 outside dm_wgrad_t_affine2_supported"
        if "smode4" in feats:
            return "refuse", "T = AFFINE2 with S = AFFINE2"
    return "match", ""


def _pairwise(route, rng):
    """Seeded greedy covering of (operand mode x epilogue feature) and (per-sample x epilogue feature) pairs."""
    ent = route.entry
    if ent == "wgrad":
        a = ("smode0", "smode1", "smode2", "smode3", "smode4")
        b = ("tmode0", "tmode1", "tmode2", "tmode3") + (("tmode4",) if t_affine2_route(route) else ())
        c = ("sps", "tps", "tones", "")
        need = {(x, y) for x in a for y in b} | {(x, z) for x in a for z in c} | {(y, z) for y in b for z in c}
    elif ent == "apply":
        return [frozenset({m, "resid"} | ({"ps"} if m in ("mode2", "mode3", "mode4") else set())) for m in MODES]
    else:
        a = MODES
        epi = CONV_EPI + (("ones", "border") if ent == "s2" else ()) + ("view",)
        need = {(m, e) for m in a for e in epi} | {(p, e) for p in ("ps", "") for e in epi}
    out = []
    while need:
        best, best_cov = None, -1
        for _ in range(40):
            if ent == "wgrad":
                m_s, m_t, z = rng.choice(a), rng.choice(b), rng.choice(c)
                cand = {m_s, m_t, z} - {"", "smode0", "tmode0"}
                cov = {(m_s, m_t), (m_s, z), (m_t, z)}
            else:
                m = rng.choice(a)
                es = rng.sample(epi, 3)
                ps = "ps" if (m in ("mode2", "mode3", "mode4") and rng.random() < 0.5) else ""
                cand = {m, *es} | ({ps} if ps else set())
                cov = {(m, e) for e in es} | {(ps, e) for e in es}
            n = len(cov & need)
            if n > best_cov:
                best, best_cov, best_set = cand, n, cov
        if best_cov <= 0:
            break
        need -= best_set
        out.append(frozenset(best))
    return out


def cases_for(route):
    """Base case, every feature alone, the entry's refusals, a seeded pairwise covering, and one persistent-grid case."""
    B = route.shape[0]
    raw = [frozenset()]
    raw += [frozenset({f}) for f in entry_features(route.entry)]
    raw += [frozenset({f}) for f in REFUSED[route.entry]]
    if route.entry != "wgrad" and route.entry != "apply":
        raw += [frozenset({"stat_q_mask", "mask_aff"}), frozenset({"stat_q_mask", "mask_aff_ps"}),
                frozenset({"per_tile", "stat_q"})]
    else:
        raw += [frozenset({"sps", "tps", "smode3", "tmode3"})] if route.entry == "wgrad" else []
    if t_affine2_route(route):       # per-sample coefficients leave the one-pass kernel for the tiled one, which must read T.p1
        raw += [frozenset({"tmode4", "tps"}), frozenset({"tmode4", "sps", "smode2"}), frozenset({"tmode4", "smode4"})]
    rng = random.Random(zlib.crc32(route.name.encode()))
    raw += _pairwise(route, rng)
    seen, out = set(), []
    for r in raw:
        f = normalize(route, r)
        if f in seen:
            continue
        seen.add(f)
        ex, why = expect_of(route, f)
        out.append(Case(route.name, f, B, ex, why))
    if route.entry != "apply":
        f = normalize(route, persistent_features(route))
        ex, why = expect_of(route, f)
        out.append(Case(route.name, f, persistent_B(route), ex, why))
    return out


# ------------------------------------------------------------------------------------- persistent-grid (big batch) cases
_NO_PER_SAMPLE = ("conv_s2_wide_stream", "conv_s2_thin_stream", "conv3x3_wide_stream", "convT_wide_stream",
                  "convT_thin_stream", "conv1x1_stream", "wgrad1x1_stream", "wgrad_s2_thin_stream", "wgrad_wide1")


def takes_per_sample(route):
    """False for the kernels whose guard sends per-sample coefficients to another route (streaming, one-pass)."""
    return not (route.env != "tiled" and route.kernel.startswith(_NO_PER_SAMPLE))


def persistent_features(route):
    """Features of the big-batch case, chosen so that the case stays on the route's kernel: per-sample coefficients
    where the kernel takes them, shared ones (still more units than workgroups) where it does not."""
    ps = takes_per_sample(route)
    if route.entry == "wgrad":
        if "tmode4" in route.base:
            return {"smode3"}
        return {"smode3", "sps", "tmode2", "tps"} if ps else {"smode3", "tmode2"}
    if not ps:
        return {"mode3", "bias"} | (set() if route.kernel.startswith("convT_thin_stream") else {"stats"})
    if route.kernel.startswith("conv4x4s2_patch") or "border" in route.base:
        return {"mode3", "ps", "stats", "bias"}
    return {"mode3", "ps", "stats", "bias", "mask_aff_ps"}


def _conv3_tile(CIN, W):
    cap = 16 if CIN >= 32 else (32 if CIN >= 16 else 64)
    TW = min(W, cap)
    return (16 if (TW == 16 and CIN < 32) else 8), TW


def declared_units(route, B):
    """(tile units, cap) of the route's dm_*_num_blocks formula: the slabs the call declares are min(units, cap) and the
    kernel's persistent grid is at most the cap, so units > cap puts several units on a workgroup."""
    k = route.kernel
    if route.entry == "wgrad":
        _, CS, CT, Hs, Ws, kk = route.shape
        if k.startswith(("wgrad_kernel", "wgrad_ys_kernel")):
            return B * (Hs // 8) * (Ws // min(Ws, 64)), 512          # 8-row tiles: a lower bound (4-row tiles double it)
        if k.startswith("wgrad1x1_stream"):
            return B * Hs * Ws // 32, 768
        if k.startswith("wgrad_s2_thin_stream"):
            return (B * Hs * (Ws // 32) + 3) // 4, 768
        if k.startswith("wgrad_wide1"):
            return B * (Hs // 8) * (Ws // 16), 256
        if k.startswith("wgrad_wide_kernel"):
            return B * (Hs // 8) * (Ws // 16), 512
        return B, 512                                                # wgrad_generic_kernel
    _, CIN, NOUT, H, W, taps = route.shape
    if k.startswith("conv4x4s2_patch"):
        return B, 768            # one patch per unit on min(B, 256) workgroups; the declared slabs are min(2 B, 768)
    if k.startswith("conv4x4s2_"):
        Ho, Wo = H // 2, W // 2
        return B * (Ho // 8) * (Wo // min(Wo, 64 if CIN <= 5 else (32 if CIN <= 8 else 16))), 768
    if k.startswith(("conv3x3_kernel", "convT_phase")):
        TH, TW = _conv3_tile(CIN, W)
        units = B * (H // TH) * (W // TW)
        return units, (units if "per_tile" in route.base else 768)   # per-tile slabs: one workgroup per tile, no grid cap
    if k.startswith("conv_generic"):
        return B, 768
    BH, BW = (H // 2, W // 2) if route.entry == "s2" else (H, W)
    return B * (BH // 8) * (BW // 16), 768                           # conv_wide_kernel and the streaming forms


def persistent_B(route):
    """The smallest batch with more units than the cap, plus a quarter."""
    u1, cap = declared_units(route, 1)
    if "per_tile" in route.base:
        cap = 768                                                    # the same batch as the persistent form of the shape
    return (cap // max(u1, 1) + 1) * 5 // 4 + 1


def row_cases():
    """The base case of every ROW_ROUTES entry."""
    return [Case(r.name, normalize(r, ()), r.shape[0], "match") for r in ROW_ROUTES]


def all_cases(env=None):
    """Every case; env None: all, "" : in-process routes (and the table-row cases), "tiled": the child's."""
    return [c for r in ROUTES if env is None or r.env == env for c in cases_for(r)] + (row_cases() if not env else [])


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _coef(C, Bc, g, two):
    """(Bc, C, 4) coefficients: c0 in [0.5, 2], c1 of the same order (AFFINE2), c2 shifting the mean; sample b scaled by
    (1 + 0.5 b) with a shift of its own."""
    c0 = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
    c1 = (0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)) * torch.where(
        torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double() if two else torch.zeros(C, dtype=torch.float64)
    c2 = (0.2 + 0.4 * torch.rand(C, generator=g, dtype=torch.float64)) * torch.where(
        torch.rand(C, generator=g) < 0.5, -1.0, 1.0).double()
    rows = []
    for b in range(Bc):
        s = 1.0 + 0.5 * b
        sh = 0.3 * torch.randn(C, generator=g, dtype=torch.float64) if b else torch.zeros(C, dtype=torch.float64)
        rows.append(torch.stack([c0 * s, c1 * s, c2 * s + sh, torch.zeros(C, dtype=torch.float64)], 1))
    return torch.stack(rows).float()


def _act(shape, g):
    """Activations with a nonzero mean and both signs (a ReLU clamps about 40 %)."""
    return (torch.randn(*shape, generator=g) + 0.3).float()


def _mask(shape, coef, g):
    """Raw mask values whose decision c0 m + c2 > 0 sits at least 0.05 from the threshold, with either coefficient form
    (coef None: IDENT)."""
    t = (0.05 + torch.rand(*shape, generator=g, dtype=torch.float64)) * torch.where(
        torch.rand(*shape, generator=g) < 0.45, -1.0, 1.0).double()
    if coef is None:
        return t.float()
    c = coef.double()
    if c.shape[0] == 1:
        c = c.expand(shape[0], -1, -1)
    c0, c2 = c[..., 0][..., None, None], c[..., 2][..., None, None]
    m = ((t - c2) / c0).float()
    val = c0 * m.double() + c2
    assert bool(((val > 0) == (t > 0)).all()) and float(val.abs().min()) > 1e-3
    return m


def conv_geometry(route, B=None):
    b, CIN, NOUT, H, W, taps = route.shape
    B = b if B is None else B
    e = route.entry
    if e == "s2":
        return dict(B=B, CIN=CIN, NOUT=NOUT, H=H, W=W, taps=taps, co=NOUT, Ho=H // 2, Wo=W // 2, k=4)
    if e == "pix":
        return dict(B=B, CIN=CIN, NOUT=NOUT, H=H, W=W, taps=taps, co=NOUT // 4, Ho=2 * H, Wo=2 * W, k=4)
    return dict(B=B, CIN=CIN, NOUT=NOUT, H=H, W=W, taps=taps, co=NOUT, Ho=H, Wo=W, k=3 if taps == 9 else 1)


def make_inputs(case, B=None, hw=None):
    """Host float32 tensors of one case.  B / hw shrink the batch / grid (the host test: the same construction at a
    size the CPU checks quickly)."""
    route = ROUTE[case.route]
    f = case.feats
    B = case.B if B is None else B
    g = _gen(zlib.crc32(case.id.encode()))
    X = {}
    if route.entry == "wgrad":
        _, CS, CT, Hs, Ws, k = route.shape
        if hw is not None:
            Hs, Ws = hw
        s = 2 if k == 4 else 1
        ctp = CT - (1 if "tones" in f else 0)
        X["S"] = _act((B, CS, Hs, Ws), g)
        X["T"] = _act((B, ctp, Hs * s, Ws * s), g)
        for side, C, shp in (("s", CS, (B, CS, Hs, Ws)), ("t", ctp, (B, ctp, Hs * s, Ws * s))):
            mode = _mode(f, side + "mode")
            if mode >= 2:
                X[side + "coef"] = _coef(C, B if side + "ps" in f else 1, g, mode == 4)
            if mode == 4:
                X[side + "p1"] = _act(shp, g)
        X["geom"] = dict(B=B, CS=CS, CT=CT, Hs=Hs, Ws=Ws, k=k)
        return X
    if route.entry == "apply":
        _, C, H, W = route.shape
        if hw is not None:
            H, W = hw
        mode = _mode(f, "mode")
        X["x"] = _act((B, C, H, W), g)
        if mode >= 2:
            X["coef"] = _coef(C, B if "ps" in f else 1, g, mode == 4)
        if mode == 4:
            X["p1"] = _act((B, C, H, W), g)
        if "resid" in f:
            X["resid"] = torch.randn(B, C, H, W, generator=g)
        X["geom"] = dict(B=B, C=C, H=H, W=W)
        return X
    G = conv_geometry(route, B)
    if hw is not None:
        G["H"], G["W"] = hw
        G["Ho"], G["Wo"] = (hw[0] // 2, hw[1] // 2) if route.entry == "s2" else ((2 * hw[0], 2 * hw[1]) if route.entry == "pix" else hw)
    CIN, NOUT, co, k = G["CIN"], G["NOUT"], G["co"], G["k"]
    cphys = CIN - (1 if "ones" in f else 0)
    mode = _mode(f, "mode")
    X["x"] = _act((B, cphys, G["H"], G["W"]), g)
    if mode >= 2:
        X["coef"] = _coef(cphys, B if "ps" in f else 1, g, mode == 4)
    if mode == 4:
        X["p1"] = _act((B, cphys, G["H"], G["W"]), g)
    # logical weight: s2/s1 [NOUT][CIN][k][k]; pix [co][CIN][4][4] (ConvTranspose2d [CIN][co] seen through the view)
    taps_k = 1 if G["taps"] == 1 else (3 if route.entry == "s1" else 4)
    nlog = co if route.entry == "pix" else NOUT
    K = CIN * (taps_k * taps_k if route.entry != "pix" else 4)
    wl = torch.randn(nlog, CIN, taps_k, taps_k, generator=g) / math.sqrt(K)
    X["wlog"] = wl
    X["wflat"], X["wview"] = _store_weight(route, wl, "view" in f)
    oshape = (B, co, G["Ho"], G["Wo"])
    if "bias" in f:
        X["bias"] = torch.randn(co, generator=g)
    if "border" in f:
        X["bias_border"] = (torch.randn(3, 3, co, generator=g) + torch.arange(9).view(3, 3, 1) * 0.25).float()
        X["bias_centre"] = X["bias_border"][1, 1].clone()
    if "mask_id" in f or "mask_relu" in f or "mask_ones" in f or "mask_affine2" in f or "mask_affine_relu" in f:
        X["mask"] = _mask(oshape, None, g)
    if "mask_aff" in f or "mask_aff_ps" in f:
        X["mcoef"] = _coef(co, B if "mask_aff_ps" in f else 1, g, False)
        X["mask"] = _mask(oshape, X["mcoef"], g)
    if "mask_affine2" in f or "mask_affine_relu" in f:
        X["mcoef"] = _coef(co, 1, g, True)
    if "resid" in f:
        X["resid"] = torch.randn(*oshape, generator=g)
    if "stat_q" in f:
        X["stat_q"] = torch.randn(*oshape, generator=g) + 0.5
    G["cphys"] = cphys
    X["geom"] = G
    return X


def _mode(f, prefix):
    for m in range(4, -1, -1):
        if f"{prefix}{m}" in f:
            return m
    return 0


def _store_weight(route, wl, noncanonical):
    """(flat tensor, (off, sn, sc, sky, skx)) such that w[off + n sn + c sc + ky sky + kx skx] = wl[n][c][ky][kx].
    Canonical: the PyTorch layout of the layer ([co][ci][k][k]; ConvTranspose2d [ci][co][k][k]).  Non-canonical: the
    transposed / flipped views data gradients use."""
    N, C, kh, kw = wl.shape
    e = route.entry
    if not noncanonical:
        if e == "pix":
            st = wl.permute(1, 0, 2, 3).contiguous()          # [C][N][4][4]
            return st.flatten(), (0, kh * kw, N * kh * kw, kw, 1)
        return wl.contiguous().flatten(), (0, C * kh * kw, kh * kw, kw if kh > 1 else 0, 1 if kw > 1 else 0)
    if e == "s2":                                              # transposed: stored [C][N][4][4]
        st = wl.permute(1, 0, 2, 3).contiguous()
        return st.flatten(), (0, kh * kw, N * kh * kw, kw, 1)
    if e == "pix":                                             # flipped taps: stored [C][N][3-ky][3-kx]
        st = wl.permute(1, 0, 2, 3).flip(2, 3).contiguous()
        return st.flatten(), (kh * kw - 1, kh * kw, N * kh * kw, -kw, -1)
    if kh == 1:                                                # 1x1 data gradient: stored [C][N]
        st = wl.permute(1, 0, 2, 3).contiguous()
        return st.flatten(), (0, 1, N, 0, 0)
    st = wl.permute(1, 0, 2, 3).flip(2, 3).contiguous()        # 3x3 data gradient: stored [C][N][2-ky][2-kx]
    return st.flatten(), (kh * kw - 1, kh * kw, N * kh * kw, -kw, -1)


def view_weight(wflat, view, shape):
    off, sn, sc, sky, skx = view
    N, C, kh, kw = shape
    idx = (off + torch.arange(N).view(N, 1, 1, 1) * sn + torch.arange(C).view(1, C, 1, 1) * sc
           + torch.arange(kh).view(1, 1, kh, 1) * sky + torch.arange(kw).view(1, 1, 1, kw) * skx)
    return wflat.double()[idx]


# --------------------------------------------------------------------------------------------------------- reference
MUTATIONS = ("coef_sample0", "no_c1p1", "no_c2", "no_load_relu", "no_ones", "no_mask", "mask_as_ident", "no_resid",
             "no_stat_q", "border_as_centre", "tile_wrong_sample", "no_bias", "no_relu")


def mutations_of(case):
    f = case.feats
    m = []
    if f & {"ps", "mask_aff_ps", "sps", "tps"}:
        m.append("coef_sample0")
    if f & {"mode4", "smode4", "tmode4"}:
        m.append("no_c1p1")
    if f & {"mode2", "mode3", "mode4", "smode2", "smode3", "smode4", "tmode2", "tmode3", "tmode4"}:
        m.append("no_c2")
    if f & {"mode1", "mode3", "smode1", "smode3", "tmode1", "tmode3"}:
        m.append("no_load_relu")
    if f & {"ones", "tones"}:
        m.append("no_ones")
    if f & {"mask_id", "mask_aff", "mask_aff_ps"}:
        m.append("no_mask")
    if f & {"mask_aff", "mask_aff_ps"}:
        m.append("mask_as_ident")
    for feat, mut in (("resid", "no_resid"), ("border", "border_as_centre"), ("per_tile", "tile_wrong_sample"),
                      ("bias", "no_bias"), ("relu", "no_relu")):
        if feat in f:
            m.append(mut)
    if f & {"stat_q", "stat_q_mask"}:
        m.append("no_stat_q")
    return m


def _load(p0, mode, coef, p1, mut, absval=False):
    """load_ref in float64 (absval: the magnitude sum |c0 p0| + |c1 p1| + |c2| of the same expression)."""
    x = p0.double()
    if mode == 0:
        return x.abs() if absval else x
    if mode == 1:
        return x.abs() if absval else (x if mut == "no_load_relu" else x.clamp(min=0))
    c = coef.double()
    if mut == "coef_sample0":
        c = c[:1]
    c0, c1, c2 = (c[..., i][..., None, None] for i in range(3))
    if mut == "no_c2":
        c2 = torch.zeros_like(c2)
    if absval:
        v = (c0 * x).abs() + c2.abs()
        if mode == 4:
            v = v + (c1 * p1.double()).abs()
        return v
    v = c0 * x + c2
    if mode == 4 and mut != "no_c1p1":
        v = v + c1 * p1.double()
    if mode == 3 and mut != "no_load_relu":
        v = v.clamp(min=0)
    return v


def _with_ones(v, ones, B, H, W, mut, absval=False):
    if not ones:
        return v
    one = torch.zeros(B, 1, H, W, dtype=torch.float64) if mut == "no_ones" else torch.ones(B, 1, H, W, dtype=torch.float64)
    return torch.cat([v, one], 1)


def _conv(route, xin, wl):
    e = route.entry
    if e == "s2":
        return F.conv2d(xin, wl, stride=2, padding=1)
    if e == "pix":
        return F.conv_transpose2d(xin, wl.permute(1, 0, 2, 3), stride=2, padding=1)
    return F.conv2d(xin, wl, padding=1 if wl.shape[-1] == 3 else 0)


def reference(case, X, mut=None):
    """float64 result of the case: dict with "out" and, where the case declares them, "stats" ((N, 2) totals or
    (B, N, 2) per sample); and the same keys with "_bound" (the accumulation bound of each element)."""
    route = ROUTE[case.route]
    f = case.feats
    if route.entry == "wgrad":
        return _wgrad_reference(case, X, mut)
    if route.entry == "apply":
        mode = _mode(f, "mode")
        v = _load(X["x"], mode, X.get("coef"), X.get("p1"), mut)
        a = _load(X["x"], mode, X.get("coef"), X.get("p1"), None, absval=True)
        if "resid" in f:
            a = a + X["resid"].double().abs()
            if mut != "no_resid":
                v = v + X["resid"].double()
        return {"out": v, "out_bound": C_BOUND * U * a * 2 + 1e-30}
    G = X["geom"]
    B, Ho, Wo, co = G["B"], G["Ho"], G["Wo"], G["co"]
    mode = _mode(f, "mode")
    xin = _with_ones(_load(X["x"], mode, X.get("coef"), X.get("p1"), mut), "ones" in f, B, G["H"], G["W"], mut)
    xab = _with_ones(_load(X["x"], mode, X.get("coef"), X.get("p1"), None, absval=True), "ones" in f, B, G["H"], G["W"], None)
    wl = X["wlog"].double()
    acc = _conv(route, xin, wl)
    A = _conv(route, xab, wl.abs())
    K = G["CIN"] * (16 if route.entry == "s2" else (4 if route.entry == "pix" else G["taps"]))
    if "bias" in f:
        A = A + X["bias"].double().abs().view(1, -1, 1, 1)
        if mut != "no_bias":
            acc = acc + X["bias"].double().view(1, -1, 1, 1)
    if "border" in f:
        bb = X["bias_centre"].double().view(1, 1, -1).expand(3, 3, -1) if mut == "border_as_centre" else X["bias_border"].double()
        ry = torch.ones(Ho, dtype=torch.long)
        ry[0], ry[-1] = 0, 2
        rx = torch.ones(Wo, dtype=torch.long)
        rx[0], rx[-1] = 0, 2
        table = bb[ry][:, rx]                                   # (Ho, Wo, co)
        acc = acc + table.permute(2, 0, 1).unsqueeze(0)
        A = A + X["bias_border"].double().abs().max(0).values.max(0).values.view(1, -1, 1, 1)
    v = acc
    if "relu" in f and mut != "no_relu":
        v = v.clamp(min=0)
    if "mask" in X and f & {"mask_id", "mask_aff", "mask_aff_ps"} and mut != "no_mask":
        if "mcoef" in X and mut != "mask_as_ident":
            mc = X["mcoef"].double()
            if mut == "coef_sample0":
                mc = mc[:1]
            keep = mc[..., 0][..., None, None] * X["mask"].double() + mc[..., 2][..., None, None] > 0
        else:
            keep = X["mask"].double() > 0
        v = torch.where(keep, v, torch.zeros_like(v))
    if "resid" in f:
        A = A + X["resid"].double().abs()
        if mut != "no_resid":
            v = v + X["resid"].double()
    ob = C_BOUND * math.sqrt(K) * U * A + 1e-30
    R = {"out": v, "out_bound": ob}
    if "stats" in f:
        if "stat_q" in f and mut != "no_stat_q":
            q, qa = X["stat_q"].double(), X["stat_q"].double().abs()
        elif "stat_q_mask" in f and mut != "no_stat_q":
            q, qa = X["mask"].double(), X["mask"].double().abs()
        else:
            q, qa = v, 2 * A
        s = torch.stack([v.sum((2, 3)), (v * q).sum((2, 3))], -1)             # (B, co, 2)
        P = Ho * Wo * (1 if "per_tile" in f else B)
        sb = torch.stack([(ob + C_BOUND * math.sqrt(P) * U * A).sum((2, 3)),
                          (ob * qa + C_BOUND * math.sqrt(P) * U * A * qa).sum((2, 3))], -1)
        if "per_tile" in f:
            if mut == "tile_wrong_sample":
                s = s.roll(1, 0)
            R["stats"], R["stats_bound"] = s, sb + 1e-30
        else:
            R["stats"], R["stats_bound"] = s.sum(0), sb.sum(0) + 1e-30
    return R


def _wgrad_reference(case, X, mut):
    f = case.feats
    G = X["geom"]
    B, CS, CT, Hs, Ws, k = G["B"], G["CS"], G["CT"], G["Hs"], G["Ws"], G["k"]
    s, p = (2, 1) if k == 4 else ((1, 1) if k == 3 else (1, 0))
    sm, tm = _mode(f, "smode"), _mode(f, "tmode")
    Sv = _load(X["S"], sm, X.get("scoef"), X.get("sp1"), mut)
    Sa = _load(X["S"], sm, X.get("scoef"), X.get("sp1"), None, absval=True)
    Tv = _load(X["T"], tm, X.get("tcoef"), X.get("tp1"), mut)
    Ta = _load(X["T"], tm, X.get("tcoef"), X.get("tp1"), None, absval=True)
    Tv = _with_ones(Tv, "tones" in f, B, Hs * s, Ws * s, mut)
    Ta = _with_ones(Ta, "tones" in f, B, Hs * s, Ws * s, None)

    def wg(Sx, Tx):
        # R[cs][ct] = sum_b conv2d(T_b, S_b as weight): the weight gradient of a Conv2d with input T and output grad S
        return torch.nn.grad.conv2d_weight(Tx, (CS, Tx.shape[1], k, k), Sx, stride=s, padding=p)

    out = wg(Sv, Tv)
    A = wg(Sa, Ta)
    K = B * Hs * Ws
    return {"out": out, "out_bound": C_BOUND * math.sqrt(K) * U * A + 1e-30}


def max_ratio(R, Rm):
    """Largest |mutated - true| / bound over every declared output of the case."""
    r = 0.0
    for key in ("out", "stats"):
        if key in R:
            r = max(r, float(((Rm[key] - R[key]).abs() / R[key + "_bound"]).max()))
    return r


def feature_axes():
    return {"s2": set(S2_FEATURES), "s1": set(CONV_FEATURES), "pix": set(CONV_FEATURES), "wgrad": set(WG_FEATURES),
            "apply": set(APPLY_FEATURES)}


def table_summary():
    return {r.name: len(cases_for(r)) for r in ROUTES}


if __name__ == "__main__":
    n = table_summary()
    print(sum(n.values()), "cases", n)
