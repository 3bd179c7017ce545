"""The fused backward entries of include/dynamorph_hip.h against float64: every accepted dy mode (IDENT, AFFINE2), the
epilogue inputs each entry takes, and the refusals (per-sample coefficients, other dy modes, a ones channel, side inputs
the entry does not take).  Pure CPU; tests/helpers/operand_contract_run.py runs the cases on the device.

  entry   shape                               arithmetic (t = relu(c0 x + c2), or relu(x) without xcoef)
  bwd_s2  dm_conv_bwd_s2_fused (CD, CX, H, W)   dx = [load(mask) > 0] conv2d_input(load(dy), w); stats (sum dx, sum dx x);
                                                dW = conv2d_weight(load(in), load(dy)), stride 2
  c1x1    dm_conv1x1_bwd_fused                  dx = [t > 0] w^T load(dy); stats (sum dx, sum dx x); dW = sum load(dy) t
  c3x3    dm_conv3x3_bwd_fused                  dx = [t > 0] conv2d_input(load(dy), w) + resid; stats (sum dx, sum dx q), q or dx
  c4s2    dm_conv4x4s2_bwd_fused                as c1x1 with a 4x4 / stride 2 convolution (H, W: the output grid)
  convt   dm_convt_bwd_fused                    gin = [S > 0] conv2d(G, w, stride 2); stats (sum gin, 0); dW = sum S G
"""
import math
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as F

import operand_contract as OC

# (name, entry, shape (B, CD|CI, CX|CO, H, W), kernel the base case launches (rocprofv3 name prefix))
FUSED_ROUTES = [
    ("bwd_s2", "bwd_s2", (2, 16, 8, 8, 32), "bwd_s2_"),
    ("c1x1", "c1x1", (2, 16, 32, 16, 16), "conv1x1_bwd_kernel<16, 32>"),
    ("c1x1_stream64", "c1x1", (2, 64, 64, 16, 16), "conv1x1_bwd_wide_stream_kernel"),
    ("c3x3_16", "c3x3", (2, 16, 16, 16, 16), "conv3x3_bwd_kernel<16, 256, false>"),
    ("c3x3_32", "c3x3", (2, 32, 16, 16, 16), "conv3x3_bwd_kernel<32, 512, false>"),
    ("c3x3_band", "c3x3", (2, 32, 16, 32, 32), "conv3x3_bwd_kernel<32, 512, true>"),
    ("c4s2", "c4s2", (2, 16, 16, 16, 16), "conv4x4s2_bwd_kernel"),
    ("convt_8x4", "convt", (2, 8, 4, 8, 32), "convT_bwd"),
    ("convt_16x8", "convt", (2, 16, 8, 8, 16), "convT_bwd"),
]
FROUTE = {r[0]: r for r in FUSED_ROUTES}

# features an entry accepts (match) and asks to refuse
ACCEPT = {
    "bwd_s2": [(), ("dy4",), ("in0",), ("mask_aff",), ("dy4", "mask_aff"), ("no_stat_q",)],
    "c1x1": [(), ("dy4",)],
    "c3x3": [(), ("dy4",), ("no_xcoef",), ("resid",), ("q",), ("no_stats",), ("dy4", "resid", "q")],
    "c4s2": [(), ("dy4",)],
    "convt": [(), ("mask_relu",), ("no_stats",), ("mask_relu", "no_stats")],
}
REFUSE = {
    "bwd_s2": {("dy4", "dy_ps"): "per-sample dy coefficients", ("in_ps",): "per-sample input coefficients",
               ("in4",): "an AFFINE2 layer input", ("resid",): "a residual", ("dy_ones",): "a ones channel on dy"},
    "c1x1": {("dy4", "dy_ps"): "per-sample dy coefficients", ("dy1",): "a RELU dy", ("dy2",): "an AFFINE dy",
             ("dy_ones",): "a ones channel on dy"},
    "c3x3": {("dy4", "dy_ps"): "per-sample dy coefficients", ("dy1",): "a RELU dy", ("dy3",): "an AFFINE_RELU dy",
             ("dy_ones",): "a ones channel on dy"},
    "c4s2": {("dy4", "dy_ps"): "per-sample dy coefficients", ("dy1",): "a RELU dy", ("dy2",): "an AFFINE dy",
             ("dy_ones",): "a ones channel on dy"},
    "convt": {},
}


@dataclass(frozen=True)
class FusedCase:
    route: str
    feats: frozenset
    B: int
    expect: str
    why: str = ""

    @property
    def id(self):
        return f"{self.route}-B{self.B}-{'+'.join(sorted(self.feats)) or 'base'}"


def fused_cases():
    out = []
    for name, entry, shape, _ in FUSED_ROUTES:
        for f in ACCEPT[entry]:
            out.append(FusedCase(name, frozenset(f), shape[0], "match"))
        for f, why in REFUSE[entry].items():
            out.append(FusedCase(name, frozenset(f), shape[0], "refuse", why))
    return out


def _dy_mode(f):
    for m in (4, 3, 2, 1):
        if f"dy{m}" in f:
            return m
    return 0


def make_fused_inputs(case):
    name, entry, shape, _ = FROUTE[case.route]
    _, CD, CX, H, W = shape
    B = case.B
    f = case.feats
    g = torch.Generator().manual_seed(zlib.crc32(case.id.encode()))
    X = {"geom": dict(B=B, CD=CD, CX=CX, H=H, W=W)}
    if entry == "convt":
        CI, CO = CD, CX
        X["S"] = OC._mask((B, CI, H, W), None, g)            # kept away from the ReLU threshold
        X["G"] = OC._act((B, CO, 2 * H, 2 * W), g)
        X["w"] = torch.randn(CI, CO, 4, 4, generator=g) / math.sqrt(CO * 4)
        return X
    ho, wo = (H, W)
    xh, xw = (2 * H, 2 * W) if entry in ("bwd_s2", "c4s2") else (H, W)
    k = {"bwd_s2": 4, "c4s2": 4, "c1x1": 1, "c3x3": 3}[entry]
    dm = _dy_mode(f)
    X["dy"] = OC._act((B, CD, ho, wo), g)
    if dm >= 2:
        X["dycoef"] = OC._coef(CD, B if "dy_ps" in f else 1, g, dm == 4)
    if dm == 4:
        X["dyp1"] = OC._act((B, CD, ho, wo), g)
    X["xcoef"] = None if "no_xcoef" in f else OC._coef(CX, B if "in_ps" in f else 1, g, "in4" in f)
    mc = X["xcoef"] if (entry != "bwd_s2" or "mask_aff" in f) else None
    X["x"] = OC._mask((B, CX, xh, xw), mc, g)                 # every ReLU / mask decision away from its threshold
    if "in4" in f:
        X["xp1"] = OC._act((B, CX, xh, xw), g)
    X["w"] = torch.randn(CD, CX, k, k, generator=g) / math.sqrt(CD * k * k)
    if "resid" in f:
        X["resid"] = torch.randn(B, CX, xh, xw, generator=g)
    if "q" in f:
        X["q"] = torch.randn(B, CX, xh, xw, generator=g) + 0.5
    X["geom"].update(k=k, xh=xh, xw=xw)
    return X


def fused_reference(case, X, mut=None):
    """float64 (dx, stats totals (CX, 2) or None, dW) with their bounds; mut: no_c1p1 / no_c2 / no_mask / no_resid."""
    name, entry, shape, _ = FROUTE[case.route]
    f = case.feats
    G = X["geom"]
    d = lambda t: t.double()                                  # noqa: E731
    if entry == "convt":
        S, Gr, w = d(X["S"]), d(X["G"]), d(X["w"])
        gin = F.conv2d(Gr, w, stride=2, padding=1)
        A = F.conv2d(Gr.abs(), w.abs(), stride=2, padding=1)
        if "mask_relu" in f and mut != "no_mask":
            gin = gin * (S > 0)
        dw = torch.nn.grad.conv2d_weight(Gr, w.shape, S, stride=2, padding=1)
        dwA = torch.nn.grad.conv2d_weight(Gr.abs(), w.shape, S.abs(), stride=2, padding=1)
        K, Kw = G["CX"] * 16, G["B"] * G["H"] * G["W"]
        stats = None if "no_stats" in f else torch.stack([gin.sum((0, 2, 3)), torch.zeros(gin.shape[1], dtype=torch.float64)], 1)
        return _pack(gin, A, K, stats, None, dw, dwA, Kw, q_is_dx=False)
    dm = _dy_mode(f)
    dyv = OC._load(X["dy"], dm, X.get("dycoef"), X.get("dyp1"), mut)
    dya = OC._load(X["dy"], dm, X.get("dycoef"), X.get("dyp1"), None, absval=True)
    x = d(X["x"])
    xc = X["xcoef"]
    s, p = (2, 1) if G["k"] == 4 else (1, 1 if G["k"] == 3 else 0)
    w = d(X["w"])
    dx = torch.nn.grad.conv2d_input(x.shape, w, dyv, stride=s, padding=p)
    A = torch.nn.grad.conv2d_input(x.shape, w.abs(), dya, stride=s, padding=p)
    if entry == "bwd_s2":
        tmode = 0 if "in0" in f else (4 if "in4" in f else 3)
        t = OC._load(X["x"], tmode, xc, X.get("xp1"), None)
        keep = (OC._load(X["x"], 2, xc, None, None) > 0) if "mask_aff" in f else (x > 0)
    else:
        t = OC._load(X["x"], 3, xc, None, None) if xc is not None else x.clamp(min=0)
        keep = t > 0
    ta = OC._load(X["x"], 2, xc, None, None, absval=True) if xc is not None else x.abs()    # magnitude of t before rounding
    if mut != "no_mask":
        dx = dx * keep
    if "resid" in f:
        A = A + d(X["resid"]).abs()
        if mut != "no_resid":
            dx = dx + d(X["resid"])
    dw = torch.nn.grad.conv2d_weight(t, w.shape, dyv, stride=s, padding=p)
    dwA = torch.nn.grad.conv2d_weight(ta, w.shape, dya, stride=s, padding=p)
    K, Kw = G["CD"] * G["k"] * G["k"], G["B"] * G["H"] * G["W"]
    stats, q, q_is_dx = None, None, False
    if not f & {"no_stats"}:
        if entry == "c3x3":
            q, q_is_dx = (d(X["q"]), False) if "q" in f else (dx, True)
        elif entry == "bwd_s2" and "no_stat_q" in f:
            q, q_is_dx = dx, True
        else:
            q = x
        stats = torch.stack([dx.sum((0, 2, 3)), (dx * q).sum((0, 2, 3))], 1)
    return _pack(dx, A, K, stats, None if q is None else (2 * A if q_is_dx else q.abs()), dw, dwA, Kw, q_is_dx)


def _pack(dx, A, K, stats, qa, dw, dwA, Kw, q_is_dx):
    ob = OC.C_BOUND * math.sqrt(K) * OC.U * A + 1e-30
    R = {"dx": dx, "dx_bound": ob, "dw": dw, "dw_bound": OC.C_BOUND * math.sqrt(Kw) * OC.U * dwA + 1e-30}
    if stats is not None:
        P = dx.shape[0] * dx.shape[2] * dx.shape[3]
        qa = torch.zeros_like(A) if qa is None else qa
        R["stats"] = stats
        R["stats_bound"] = torch.stack([(ob + OC.C_BOUND * math.sqrt(P) * OC.U * A).sum((0, 2, 3)),
                                        (ob * qa + OC.C_BOUND * math.sqrt(P) * OC.U * A * qa).sum((0, 2, 3))], 1) + 1e-30
    return R


def fused_mutations(case):
    f = case.feats
    m = []
    if "dy4" in f:
        m += ["no_c1p1", "no_c2"]
    name, entry, _, _ = FROUTE[case.route]
    if entry != "convt" or "mask_relu" in f:
        m.append("no_mask")
    if "resid" in f:
        m.append("no_resid")
    return m


def fused_max_ratio(R, Rm):
    r = 0.0
    for key in ("dx", "dw", "stats"):
        if key in R:
            r = max(r, float(((Rm[key] - R[key]).abs() / R[key + "_bound"]).max()))
    return r
