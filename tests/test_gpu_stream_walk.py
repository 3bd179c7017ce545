"""The wide family's streaming kernels (csrc/wide_stream.hip, wgrad_wide1_kernel) at batch sizes where every walker takes
two units or more -- the loop the z32ex workload spends its time in.  Cases, walk arithmetic and conditions:
tests/helpers/stream_walk.py; tests/test_stream_walk_host.py checks them without a GPU.

Convolutions and data gradients: the whole run must be BIT-EQUAL to the same call on consecutive batch slices small enough
that the plan reports at most one unit per walker (the regime tests/test_gpu_kernels.py holds against float64): an output
element's products run in one fixed order whichever unit it falls in.  Three or four samples are also held to a float64 CPU
reference at the kernel tests' bound, and the statistics slabs to float64 sums of the fp32 output at close_stats' bound.

Weight gradients: the partition changes with the batch, so whole run and slices differ in their last bits.  The reference is
float64 on the GPU; the bound is four times the error, against that reference, of the sum of the sliced runs' gradients (each a
launch of the regime the kernel tests cover) -- measured in the test, printed, recorded per case in HISTORY.md.  Two whole
runs are bit-equal."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import stream_walk as SW  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from dynamorph_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV) * scale


def load_ref(p0, mode, coef=None, p1=None):
    """dm_operand's transform in the dtype of its arguments; coef (C, 4)."""
    if mode == 0:
        return p0
    if mode == 1:
        return p0.clamp(min=0)
    c0, c1, c2 = (coef[:, i].view(1, -1, 1, 1) for i in range(3))
    if mode == 4:
        return c0 * p0 + c1 * p1 + c2
    v = c0 * p0 + c2
    return v.clamp(min=0) if mode == 3 else v


def close(a, b, rtol, atol, what="", where=None):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    if where is not None:
        bad &= where
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max():.3e} (ref max {b.abs().max():.3e})"


def close_stats_gpu(st, out, q, what):
    """tests/test_gpu_kernels.py's close_stats with the float64 sums taken on the GPU: error against the sum of magnitudes."""
    o, qq = out.double(), (out if q is None else q).double()
    ref = torch.stack([o.sum((0, 2, 3)), (o * qq).sum((0, 2, 3))], 1)
    mag = torch.stack([o.abs().sum((0, 2, 3)), (o * qq).abs().sum((0, 2, 3))], 1)
    err = (st.double() - ref).abs()
    print(f"{what}: worst {float((err / (mag + 1e-30)).max()):.2e} of the magnitude sum (bound 3e-5)")
    bad = err > 3e-5 * mag + 1e-9
    assert not bad.any(), f"{what}: {int(bad.sum())} sums off, worst {float((err / (mag + 1e-30)).max()):.2e} of the magnitude sum"


def coef_table(c, seed, c1=True):
    return torch.stack([rnd(c, seed=seed).abs() + 0.5, rnd(c, seed=seed + 1) * 0.2 if c1 else torch.zeros(c, device=DEV),
                        rnd(c, seed=seed + 2) * 0.3 + 0.1, torch.zeros(c, device=DEV)], 1)


def assert_plan(ops, case, plan):
    """The kernel and the multi-unit walk, from the query, for the call as it is made (real operands) -- and the same answer
    as the description by modes and flags the host test walks."""
    SW.conditions(case, plan)
    assert plan == SW.plan(ops, case), (SW.case_id(case), plan)


# ============================================================================ convolutions and data gradients
class ConvCall:
    """One convolution case: its tensors on the GPU, the call on a batch slice, the float64 reference of one sample."""

    def __init__(self, ops, c):
        self.ops, self.c = ops, c
        B, cin, h, w = c.B, c.a, c.h, c.w
        self.co = co = c.b
        self.x = rnd(B, cin, h, w, seed=1)
        self.x1 = rnd(B, cin, h, w, seed=2) if c.mode == 4 else None
        self.coef = coef_table(cin, 3, c1=c.mode == 4) if c.mode >= 2 else None
        self.dgrad = c.mode == 4 and c.api == "conv3"              # data-gradient forms: transposed (and flipped) weight view
        if c.api == "conv4":
            self.wt = rnd(co, cin, 4, 4, seed=6, scale=0.1)
            self.wv = ops.weight_view(self.wt, cin * 16, 16, 4, 1)
            self.oh, self.ow = h // 2, w // 2
        elif c.api == "convT":
            self.wt = rnd(cin, co, 4, 4, seed=6, scale=0.1)
            self.wv = ops.weight_view(self.wt, 16, co * 16, 4, 1)
            self.oh, self.ow = 2 * h, 2 * w
        elif c.k == 1:
            self.wt = rnd(cin, co, 1, 1, seed=6, scale=0.2) if self.dgrad else rnd(co, cin, 1, 1, seed=6, scale=0.2)
            self.wv = ops.weight_view(self.wt, 1, co, 0, 0) if self.dgrad else ops.weight_view(self.wt, cin, 1, 0, 0)
            self.oh, self.ow = h, w
        else:
            self.wt = rnd(co, cin, 3, 3, seed=6, scale=0.05)
            self.wv = ops.weight_view(self.wt, 9, cin * 9, -3, -1, off=8) if self.dgrad else ops.weight_view(self.wt, cin * 9, 9, 3, 1)
            self.oh, self.ow = h, w
        e = c.epi
        self.bias = rnd(co, seed=7) if "bias" in e else None
        self.relu = "relu" in e
        self.gate = rnd(B, co, self.oh, self.ow, seed=8) if e in ("gate+q", "all") else None
        self.gate_mode = SW.IDENT if c.kernel == "conv3x3_wide_stream" else SW.AFFINE
        self.mcoef = torch.stack([rnd(co, seed=11), torch.zeros(co, device=DEV), rnd(co, seed=12) * 0.3, torch.zeros(co, device=DEV)], 1)
        self.resid = rnd(B, co, self.oh, self.ow, seed=10) if "resid" in e or e == "all" else None
        self.q = rnd(B, co, self.oh, self.ow, seed=9) if e == "all" else None
        self.want_stats = e in ("stats", "bias+stats", "gate+q", "all")

    def args(self, b0, b1):
        c = self.c
        inp = self.ops.Op(self.x[b0:b1], c.mode, self.coef, p1=self.x1[b0:b1] if self.x1 is not None else None)
        kw = {}
        if self.bias is not None:
            kw.update(bias=self.bias)
        if self.relu:
            kw.update(relu=True)
        if self.gate is not None:
            kw.update(mask=self.ops.Op(self.gate[b0:b1], self.gate_mode, self.mcoef if self.gate_mode >= 2 else None))
        if self.resid is not None:
            kw.update(resid=self.resid[b0:b1])
        if c.epi == "gate+q":
            kw.update(stat_q=kw["mask"].p0)                        # the training step's form: the gate's own tensor
        elif self.q is not None:
            kw.update(stat_q=self.q[b0:b1])
        return inp, kw

    def plan(self, b0, b1):
        c, (inp, kw) = self.c, self.args(b0, b1)
        if self.want_stats:
            kw.update(stats=True)
        if c.api == "conv4":
            return self.ops.conv4x4s2_plan(inp, b1 - b0, c.a, c.b, c.h, c.w, **kw)
        if c.api == "convT":
            return self.ops.conv3x3_plan(inp, b1 - b0, c.a, 4 * c.b, c.h, c.w, taps=9, pixel_shuffle=True, **kw)
        return self.ops.conv3x3_plan(inp, b1 - b0, c.a, c.b, c.h, c.w, taps=c.k, **kw)

    def run(self, b0, b1):
        c, (inp, kw) = self.c, self.args(b0, b1)
        if c.api == "conv4":
            return self.ops.conv4x4s2(inp, self.wv, b1 - b0, c.a, c.b, c.h, c.w, want_stats=self.want_stats, **kw)
        if c.api == "convT":
            return self.ops.conv3x3(inp, self.wv, b1 - b0, c.a, 4 * c.b, c.h, c.w, taps=9, pixel_shuffle=True,
                                    want_stats=self.want_stats, **kw)
        return self.ops.conv3x3(inp, self.wv, b1 - b0, c.a, c.b, c.h, c.w, taps=c.k, want_stats=self.want_stats, **kw)

    def stat_q(self):
        return self.gate if self.c.epi == "gate+q" else self.q

    def reference(self, b):
        """float64 on the CPU (F.conv2d / conv_transpose2d as tests/test_gpu_kernels.py builds it) of sample b, and where
        the gate is decided beyond rounding (its value is c0 * gate + c2 in fp32 on the device)."""
        c = self.c
        d = lambda t: None if t is None else t.cpu().double()      # noqa: E731
        xin = load_ref(d(self.x[b:b + 1]), c.mode, d(self.coef), d(self.x1[b:b + 1]) if self.x1 is not None else None)
        wt, bias = d(self.wt), d(self.bias)
        if c.api == "conv4":
            ref = F.conv2d(xin, wt, bias, stride=2, padding=1)
        elif c.api == "convT":
            ref = F.conv_transpose2d(xin, wt, bias, stride=2, padding=1)
        elif c.k == 1:
            ref = F.conv2d(xin, wt.permute(1, 0, 2, 3) if self.dgrad else wt, bias)
        else:
            ref = F.conv_transpose2d(xin, wt, bias, padding=1) if self.dgrad else F.conv2d(xin, wt, bias, padding=1)
        if self.relu:
            ref = F.relu(ref)
        sure = None
        if self.gate is not None:
            g = d(self.gate[b:b + 1])
            if self.gate_mode >= 2:
                g = d(self.mcoef)[:, 0].view(1, -1, 1, 1) * g + d(self.mcoef)[:, 2].view(1, -1, 1, 1)
            ref = ref * (g > 0)
            sure = g.abs() > 1e-6
            assert float(sure.double().mean()) > 0.999
        if self.resid is not None:
            ref = ref + d(self.resid[b:b + 1])
        return ref, sure


@pytest.mark.parametrize("case", SW.CONV_CASES, ids=SW.case_id)
def test_convolution_walk_is_bit_equal_to_one_unit_launches(ops, case):
    call = ConvCall(ops, case)
    plan = call.plan(0, case.B)
    assert_plan(ops, case, plan)
    out, st = call.run(0, case.B)
    # slices: the same kernel, at most one unit per walker
    per = SW.slice_batch(ops, case)
    parts = []
    for b0, b1 in SW.slices(case.B, per):
        q = call.plan(b0, b1)
        assert q.kernel == plan.kernel and SW.max_units_per_walker(q) <= 1, (SW.case_id(case), b0, b1, q)
        o, s = call.run(b0, b1)
        assert torch.equal(out[b0:b1], o), f"{SW.case_id(case)}: samples [{b0}, {b1}) differ from their one-unit launch: " \
                                           f"{int((out[b0:b1] != o).sum())} elements, max {float((out[b0:b1] - o).abs().max()):.3e}"
        parts.append(s)
    for b in SW.reference_samples(case, plan):
        ref, sure = call.reference(b)
        close(out[b:b + 1], ref, 5e-5, 5e-5, f"{SW.case_id(case)} sample {b}", sure)
    if st is not None:
        assert st.shape[0] >= plan.workgroups
        close_stats_gpu(st.sum(0), out, call.stat_q(), SW.case_id(case))
        assert all(s is not None for s in parts)
    else:
        assert not call.want_stats
    out2, st2 = call.run(0, case.B)
    assert torch.equal(out, out2) and (st is None or torch.equal(st, st2))


# ============================================================================ fused backward of the 1x1 layer
@pytest.mark.parametrize("case", SW.BWD_CASES, ids=SW.case_id)
def test_fused_1x1_backward_walk(ops, case):
    B, C, H, W = case.B, case.a, case.h, case.w
    two = case.mode == 4
    dy, y = rnd(B, C, H, W, seed=1), rnd(B, C, H, W, seed=2)
    coef = torch.stack([rnd(C, seed=3), rnd(C, seed=4) * 0.1, rnd(C, seed=5) * 0.1, torch.zeros(C, device=DEV)], 1)
    x = rnd(B, C, H, W, seed=6)
    xcoef = torch.stack([rnd(C, seed=7).abs() + 0.5, torch.zeros(C, device=DEV), rnd(C, seed=8) * 0.3, torch.zeros(C, device=DEV)], 1)
    w = rnd(C, C, 1, 1, seed=9, scale=0.1)

    def run(b0, b1):
        op = ops.Op(dy[b0:b1], 4, coef, p1=y[b0:b1]) if two else ops.Op(dy[b0:b1])
        dst = torch.empty(C, C, 1, 1, device=DEV)
        dx, st = ops.conv1x1_bwd_fused(op, x[b0:b1], xcoef, w, dst, b1 - b0, C, C, H, W)
        return dx, st, dst, ops.conv1x1_bwd_fused_plan(op, b1 - b0, C, C, H, W)

    dx, st, dw, plan = run(0, B)
    assert_plan(ops, case, plan)
    per = SW.slice_batch(ops, case)
    dw_parts = torch.zeros(C, C, 1, 1, device=DEV, dtype=torch.float64)
    for b0, b1 in SW.slices(B, per):
        dxs, _, dws, q = run(b0, b1)
        assert q.kernel == plan.kernel and SW.max_units_per_walker(q) <= 1
        assert torch.equal(dx[b0:b1], dxs), f"dx of samples [{b0}, {b1}) differs from its one-unit launch"
        dw_parts += dws.double()
    # float64: dx on three samples (CPU), dW over the whole batch (GPU)
    d = lambda t: t.cpu().double()      # noqa: E731
    for b in SW.reference_samples(case, plan):
        da = load_ref(d(dy[b:b + 1]), 4, d(coef), d(y[b:b + 1])) if two else d(dy[b:b + 1])
        t = d(xcoef)[:, 0].view(1, -1, 1, 1) * d(x[b:b + 1]) + d(xcoef)[:, 2].view(1, -1, 1, 1)
        ref = F.conv_transpose2d(da, d(w)) * (t > 0)
        close(dx[b:b + 1], ref, 5e-5, 5e-5, f"fused 1x1 backward: dx of sample {b}", t.abs() > 1e-6)
    close_stats_gpu(st.sum(0), dx, x, "fused 1x1 backward statistics")
    da = load_ref(dy.double(), 4, coef.double(), y.double()) if two else dy.double()
    t = (xcoef[:, 0].double().view(1, -1, 1, 1) * x.double() + xcoef[:, 2].double().view(1, -1, 1, 1)).clamp(min=0)
    ref = torch.einsum("bop,bip->oi", da.flatten(2), t.flatten(2)).view(C, C, 1, 1)
    check_wgrad(dw, dw_parts, ref, SW.case_id(case))
    dx2, st2, dw2, _ = run(0, B)
    assert torch.equal(dx, dx2) and torch.equal(st, st2) and torch.equal(dw, dw2)


# ============================================================================ weight gradients
def check_wgrad(whole, sliced_sum, ref, what):
    """The whole run within four times the error of the summed one-unit launches, both against float64."""
    e_sliced = float((sliced_sum - ref).abs().max())
    e_whole = float((whole.double() - ref).abs().max())
    print(f"{what}: max|dW| {float(ref.abs().max()):.4e}  sliced-sum error {e_sliced:.3e}  whole-run error {e_whole:.3e}  "
          f"bound {4 * e_sliced:.3e}")
    assert e_sliced > 0
    assert e_whole <= 4 * e_sliced, f"{what}: whole-run error {e_whole:.3e} above 4 x {e_sliced:.3e}"


def wgrad_reference(S, T, k, chunk=200):
    """sum_{b,y,x} S[b,cs,y,x] * T[b,ct,y*s+ky-p,x*s+kx-p] in float64 on the GPU: einsum for 1x1, unfold + matmul else."""
    cs, ct = S.shape[1], T.shape[1]
    ref = torch.zeros(cs, ct * k * k, device=S.device, dtype=torch.float64)
    for b0 in range(0, S.shape[0], chunk):
        s, t = S[b0:b0 + chunk].flatten(2), T[b0:b0 + chunk]
        cols = t.flatten(2) if k == 1 else F.unfold(t, k, padding=1, stride=2 if k == 4 else 1)
        ref += torch.einsum("bsl,bkl->sk", s, cols)
    return ref.view(cs, ct, k, k)


@pytest.mark.parametrize("case", SW.WGRAD_CASES, ids=SW.case_id)
def test_weight_gradient_walk(ops, case):
    B, cs, ct, hs, ws, k = case.B, case.a, case.b, case.h, case.w, case.k
    sc = 2 if k == 4 else 1
    dy = rnd(B, cs, hs, ws, seed=1)
    a = rnd(B, cs, hs, ws, seed=2) if case.mode == 4 else None
    coef = torch.stack([rnd(cs, seed=3), rnd(cs, seed=4) * 0.1, rnd(cs, seed=5) * 0.1, torch.zeros(cs, device=DEV)], 1)
    t = rnd(B, ct, sc * hs, sc * ws, seed=6)
    t1 = rnd(B, ct, sc * hs, sc * ws, seed=9) if case.mode2 == 4 else None
    tcoef = torch.stack([rnd(ct, seed=7), rnd(ct, seed=10) * 0.3 if case.mode2 == 4 else torch.zeros(ct, device=DEV),
                         rnd(ct, seed=8) * 0.2 + 0.3, torch.zeros(ct, device=DEV)], 1)

    def run(b0, b1):
        S = ops.Op(dy[b0:b1], case.mode, coef if case.mode >= 2 else None, p1=a[b0:b1] if a is not None else None)
        T = ops.Op(t[b0:b1], case.mode2, tcoef if case.mode2 >= 2 else None, p1=t1[b0:b1] if t1 is not None else None)
        dst = torch.empty(cs, ct, k, k, device=DEV)
        ops.wgrad(S, T, dst, b1 - b0, cs, ct, hs, ws, k)
        return dst, ops.wgrad_plan(S, T, b1 - b0, cs, ct, hs, ws, k)

    dw, plan = run(0, B)
    assert_plan(ops, case, plan)
    per = SW.slice_batch(ops, case)
    parts = torch.zeros(cs, ct, k, k, device=DEV, dtype=torch.float64)
    for b0, b1 in SW.slices(B, per):
        d, q = run(b0, b1)
        assert q.kernel == plan.kernel and SW.max_units_per_walker(q) <= 1, (SW.case_id(case), q)
        parts += d.double()
    Sd = load_ref(dy.double(), case.mode, coef.double(), a.double() if a is not None else None)
    Td = load_ref(t.double(), case.mode2, tcoef.double(), t1.double() if t1 is not None else None)
    check_wgrad(dw, parts, wgrad_reference(Sd, Td, k), SW.case_id(case))
    dw2, _ = run(0, B)
    assert torch.equal(dw, dw2)
