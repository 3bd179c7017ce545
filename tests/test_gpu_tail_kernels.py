"""The fused decoder tail (forward, backward, training form), the output head and the enc.0 / enc.1 composition kernels
against the float64 references, exact outputs and counted bounds of tests/helpers/tail_reference.py, over the grids defined
there: every tiling, more tiles than the grid, impulses at every seam, every head arm, masks with NIN channels and exact
zeros.  The slab buffers are the caller's: pre-filled with the sentinel (raw _lib calls), so an ownerless slab that was
not zeroed, or a row nobody wrote (NaN), shows.  No bound here comes from a GPU run (tests/test_tail_reference_host.py
derives and checks them on the host)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tail_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
GUARD = 64


@pytest.fixture(scope="module")
def ops():
    from dynamorph_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from dynamorph_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(*shape, dtype=torch.float32, fill=NAN):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    buf[n:] = T.SENTINEL
    return buf, buf[:n].view(*shape)


def guard_ok(buf, what):
    assert bool((buf[-GUARD:] == T.SENTINEL).all()), f"{what}: the guard row behind the output was written"


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def check(name, got, ref, case_exact, what):
    """Bit for bit where the case holds `name` exactly, else within its bound; names the first column that differs."""
    want, got = ref[name], got.detach().cpu().double().reshape(ref[name].shape)
    assert not torch.isnan(got).any(), f"{what} {name}: {int(torch.isnan(got).sum())} elements unwritten or NaN"
    if name in case_exact:
        if not torch.equal(got, want):
            idx = (got != want).nonzero()
            cols = sorted(set(idx[:, -1].tolist()))[:8] if idx.shape[1] else []
            raise AssertionError(f"{what} {name}: {idx.shape[0]} elements differ from the exact reference, first at "
                                 f"{idx[0].tolist()}, columns {cols}")
        return 0.0
    err, bound = (got - want).abs(), ref["b_" + name]
    worst = float(torch.nan_to_num(err / bound, nan=0.0).max())
    print(f"[tail gpu] {what} {name}: worst error / bound {worst:.3f}")
    assert not (err > bound).any(), f"{what} {name}: worst {worst:.2f} bounds (max err {float(err.max()):.3e})"
    return worst


# =============================================================================================== decoder tail
def raw_tail(lib, a, which):
    """which: 'forward' -> (decoded, loss slabs); 'backward' (needs a['dec']) / 'train' -> (g2, part, wsl[, loss slabs]).
    Every output buffer is the test's: NaN in the per-element outputs, the sentinel in the slabs."""
    d2 = a["d2"]
    B, _, H2, W2 = d2.shape
    NIN = a["w6"].shape[0]
    nb = lib.dm_dec_tail_num_blocks(B, H2, W2)
    mc = 0 if a["mask"] is None else a["mask"].shape[1]
    if which == "forward":
        dbuf, dec = guarded(B, NIN, 2 * H2, 2 * W2)
        lbuf, ls = guarded(nb, dtype=torch.float64, fill=T.SENTINEL)
        rc = lib.dm_dec_tail_forward(ptr(d2), ptr(a["w4"]), ptr(a["b4"]), ptr(a["w6"]), ptr(a["b6"]), ptr(a["x"]), ptr(a["mask"]),
                                     mc, ptr(a["var"]), ptr(dec), ptr(ls), B, 4, NIN, H2, W2, stream())
        assert rc == 0
        guard_ok(dbuf, "decoded"), guard_ok(lbuf, "loss slabs")
        return dec, ls
    gbuf, g2 = guarded(B, 4, H2, W2)
    pbuf, part = guarded(nb, NIN * 4 + NIN + 8, 2, dtype=torch.float64, fill=T.SENTINEL)
    wbuf, wsl = guarded(nb, 256, fill=T.SENTINEL)
    lbuf, ls = guarded(nb, dtype=torch.float64, fill=T.SENTINEL)
    if which == "backward":
        rc = lib.dm_dec_tail_backward(ptr(d2), ptr(a["w4"]), ptr(a["b4"]), ptr(a["w6"]), ptr(a["dec"]), ptr(a["x"]), ptr(a["mask"]),
                                      mc, ptr(a["var"]), ptr(a["gs"]), ptr(g2), ptr(part), ptr(wsl), B, 4, NIN, H2, W2, stream())
    else:
        rc = lib.dm_dec_tail_train(ptr(d2), ptr(a["w4"]), ptr(a["b4"]), ptr(a["w6"]), ptr(a["b6"]), ptr(a["x"]), ptr(a["mask"]),
                                   mc, ptr(a["var"]), ptr(a["gs"]), ptr(g2), ptr(part), ptr(wsl), ptr(ls), B, 4, NIN, H2, W2,
                                   stream())
    assert rc == 0
    for b_, n_ in ((gbuf, "g2"), (pbuf, "part slabs"), (wbuf, "dW4 slabs"), (lbuf, "loss slabs")):
        guard_ok(b_, n_)
    return g2, part, wsl, ls


def tail_sums(part, wsl, NIN):
    """The slabs reduced on the host in float64 (every slab counts: one that kept the sentinel shows)."""
    flat = part.cpu()[:, :, 0].sum(0)
    assert float(part.cpu()[:, :, 1].abs().max()) == 0.0
    c = 4
    return dict(dW6=flat[:NIN * c].reshape(NIN, c), db6=flat[NIN * c:NIN * c + NIN], db4=flat[NIN * c + NIN:NIN * c + NIN + c],
                db2=flat[NIN * c + NIN + c:], dW4=wsl.cpu().double().sum(0).reshape(4, 4, 4, 4))


@pytest.mark.parametrize("case", T.tail_cases() + T.tail_impulse_cases(), ids=lambda c: c["name"])
def test_dec_tail_against_float64(lib, ops, case):
    a = T.tail_inputs(case)
    dy = case["kind"] != "randn"
    ex = case["exact"]
    NIN, N = case["NIN"], a["x"].numel()
    g = {k: dev(v) for k, v in a.items() if k != "gscale"}
    g["gs"] = torch.tensor([a["gscale"]], device=DEV)
    name = case["name"]
    ref_t = T.dec_tail_ref(**a, fused=True, dyadic=dy)
    ref_b = T.dec_tail_ref(**a, fused=False, dyadic=dy)

    # forward, with and without a loss
    dec, ls = raw_tail(lib, g, "forward")
    check("decoded", dec, ref_t, ex, name + " forward")
    check("loss", ls.cpu().sum() / N, ref_t, ex, name + " forward")
    g0 = dict(g, x=None, mask=None)
    dec_only, ls0 = raw_tail(lib, g0, "forward")
    assert torch.equal(dec_only, dec) and bool((ls0 == 0).all()), "x = NULL: same decoded; loss slabs, where given, are zeros"
    dec2, ls2 = raw_tail(lib, g, "forward")
    assert torch.equal(dec2, dec) and torch.equal(ls2, ls), "forward: not bitwise reproducible"

    # backward (not fused: WIDE tiles wherever the row is not 64 wide) and the training form (EDGE at multiples of 64)
    g["dec"] = dec
    outs = {}
    for which, ref in (("backward", ref_b), ("train", ref_t)):
        g2, part, wsl, lsl = raw_tail(lib, g, which)
        sums = tail_sums(part, wsl, NIN)
        what = f"{name} {which} ({ref['launch']['tiling']}, {ref['launch']['ntiles']} tiles on {ref['launch']['grid']})"
        check("g2", g2, ref, ex, what)
        for k in ("dW4", "dW6", "db6", "db4", "db2"):
            check(k, sums[k], ref, ex, what)
        if which == "train":
            check("loss", lsl.cpu().sum() / N, ref, ex, what)
        else:
            assert bool((lsl == T.SENTINEL).all())
        again = raw_tail(lib, g, which)
        assert all(torch.equal(p, q) for p, q in zip((g2, part, wsl, lsl), again)), which + ": not bitwise reproducible"
        outs[which] = (g2, sums, lsl)
    # the two agree with one another: each within its bound of the same reference (above), and bit for bit where g2 is exact
    if "g2" in ex:
        assert torch.equal(outs["backward"][0], outs["train"][0]), "backward and train disagree on g2"
    # forward / backward / train agree on what they share: bit for bit where the output is exact (each equals the reference
    # above), else within the sum of their two bounds (they walk different tilings and add their fp32 partials in another order)
    lf, lt = ls.cpu().sum() / N, outs["train"][2].cpu().sum() / N
    assert abs(float(lf - lt)) <= 2 * float(ref_t["b_loss"]), "forward and train disagree on the loss"
    for k in ("dW4", "dW6", "db6", "db4", "db2"):
        gap = (outs["backward"][1][k] - outs["train"][1][k]).abs()
        assert not (gap > ref_b["b_" + k] + ref_t["b_" + k]).any(), f"backward and train disagree on {k}"
    # the ops wrappers hand out the same launches
    g2o, parto, wslo, lso = ops.dec_tail_train(g["d2"], g["w4"], g["b4"], g["w6"], g["b6"], g["x"], g["mask"], g["var"], g["gs"])
    so = tail_sums(parto, wslo, NIN)
    assert torch.equal(g2o, outs["train"][0]) and torch.equal(lso.cpu().sum(), outs["train"][2].cpu().sum())
    assert all(torch.equal(so[k], outs["train"][1][k]) for k in so)


def test_dec_tail_null_b6_is_zero_bias(lib):
    """include/dynamorph_hip.h: b6 = NULL means a zero bias (forward and training form)."""
    case = T.tail_cases()[0]
    a = T.tail_inputs(case)
    g = {k: dev(v) for k, v in a.items() if k != "gscale"}
    g["gs"] = torch.tensor([a["gscale"]], device=DEV)
    zero = dict(g, b6=torch.zeros_like(g["b6"]))
    null = dict(g, b6=None)
    assert all(torch.equal(p, q) for p, q in zip(raw_tail(lib, zero, "forward"), raw_tail(lib, null, "forward")))
    assert all(torch.equal(p, q) for p, q in zip(raw_tail(lib, zero, "train"), raw_tail(lib, null, "train")))


def test_null_gscale_is_refused_and_head_nulls_mean_what_the_header_says(lib):
    """include/dynamorph_hip.h: gscale_dev is required by dm_dec_tail_backward / _train (refused, nothing launched: the
    outputs keep their fill); the head's b6 = NULL is a zero bias, x = NULL writes zeros to loss_slabs where given, and
    dm_head_backward needs gscale_dev or gdec_ext."""
    a = T.tail_inputs(T.tail_cases()[0])
    g = {k: dev(v) for k, v in a.items() if k != "gscale"}
    B, _, H2, W2 = g["d2"].shape
    NIN = g["w6"].shape[0]
    nb = lib.dm_dec_tail_num_blocks(B, H2, W2)
    mc = 0 if g["mask"] is None else g["mask"].shape[1]
    _, g2 = guarded(B, 4, H2, W2)
    _, part = guarded(nb, NIN * 4 + NIN + 8, 2, dtype=torch.float64)
    _, wsl = guarded(nb, 256)
    _, ls = guarded(nb, dtype=torch.float64)
    dec = torch.zeros(B, NIN, 2 * H2, 2 * W2, device=DEV)
    assert lib.dm_dec_tail_backward(ptr(g["d2"]), ptr(g["w4"]), ptr(g["b4"]), ptr(g["w6"]), ptr(dec), ptr(g["x"]), ptr(g["mask"]), mc,
                                    ptr(g["var"]), None, ptr(g2), ptr(part), ptr(wsl), B, 4, NIN, H2, W2, stream()) != 0
    assert lib.dm_dec_tail_train(ptr(g["d2"]), ptr(g["w4"]), ptr(g["b4"]), ptr(g["w6"]), ptr(g["b6"]), ptr(g["x"]), ptr(g["mask"]), mc,
                                 ptr(g["var"]), None, ptr(g2), ptr(part), ptr(wsl), ptr(ls), B, 4, NIN, H2, W2, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(g2).all()) and bool(torch.isnan(part).all()) and bool(torch.isnan(wsl).all())

    case = [c for c in T.head_cases() if c["form"] == "g"][0]
    h = T.head_inputs(case)
    hd = {k: dev(v) for k, v in h.items() if torch.is_tensor(v)}
    B, C4, H, W = hd["d4"].shape
    NIN = hd["w6"].shape[0]
    nb = lib.dm_head_num_blocks(B, H, W)
    mc = 0 if hd.get("mask") is None else hd["mask"].shape[1]

    def fwd(b6, x):
        _, dec = guarded(B, NIN, H, W)
        _, sl = guarded(nb, dtype=torch.float64, fill=T.SENTINEL)
        assert lib.dm_head_forward(ptr(hd["d4"]), ptr(hd["w6"]), ptr(b6), ptr(x), ptr(hd.get("mask")) if x is not None else None,
                                   mc if x is not None else 0, ptr(hd["var"]), ptr(dec), ptr(sl), B, C4, NIN, H, W, stream()) == 0
        return dec, sl
    full = fwd(hd["b6"], hd["x"])
    zero, null = fwd(torch.zeros_like(hd["b6"]), hd["x"]), fwd(None, hd["x"])
    assert torch.equal(zero[0], null[0]) and torch.equal(zero[1], null[1])
    only = fwd(hd["b6"], None)
    assert torch.equal(only[0], full[0]) and bool((only[1] == 0).all())
    _, g4 = guarded(B, C4, H, W)
    _, part = guarded(nb, NIN * C4 + NIN + C4, 2, dtype=torch.float64)
    assert lib.dm_head_backward(ptr(full[0]), ptr(hd["x"]), ptr(hd.get("mask")), mc, ptr(hd["var"]), ptr(hd["d4"]), ptr(hd["w6"]), None,
                                None, ptr(g4), ptr(part), B, C4, NIN, H, W, stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(g4).all())


# =============================================================================================================== head
@pytest.mark.parametrize("case", T.head_cases(), ids=lambda c: c["name"])
def test_head_against_float64(lib, ops, case):
    a = T.head_inputs(case)
    ref = T.head_ref(**a)
    ex, name = case["exact"], "head " + case["name"]
    B, C4, H, W = a["d4"].shape
    NIN, N = a["w6"].shape[0], a["x"].numel()
    g = {k: dev(v) for k, v in a.items() if k != "gscale"}
    gs = None if a["gscale"] is None else torch.tensor([a["gscale"]], device=DEV)
    mc = 0 if a["mask"] is None else a["mask"].shape[1]
    nb = lib.dm_head_num_blocks(B, H, W)
    assert nb == T.head_blocks(B, H, W)
    dbuf, dec = guarded(B, NIN, H, W)
    lbuf, ls = guarded(nb, dtype=torch.float64, fill=T.SENTINEL)
    assert lib.dm_head_forward(ptr(g["d4"]), ptr(g["w6"]), ptr(g["b6"]), ptr(g["x"]), ptr(g["mask"]), mc, ptr(g["var"]), ptr(dec),
                               ptr(ls), B, C4, NIN, H, W, stream()) == 0
    guard_ok(dbuf, "decoded"), guard_ok(lbuf, "loss slabs")
    check("decoded", dec, ref, ex, name)
    check("loss", ls.cpu().sum() / N, ref, ex, name)
    gbuf, g4 = guarded(B, C4, H, W)
    pbuf, part = guarded(nb, NIN * C4 + NIN + C4, 2, dtype=torch.float64, fill=T.SENTINEL)
    assert lib.dm_head_backward(ptr(dec), ptr(g["x"]), ptr(g["mask"]), mc, ptr(g["var"]), ptr(g["d4"]), ptr(g["w6"]), ptr(gs),
                                ptr(g["gdec_ext"]), ptr(g4), ptr(part), B, C4, NIN, H, W, stream()) == 0
    guard_ok(gbuf, "g4"), guard_ok(pbuf, "part slabs")
    check("g4", g4, ref, ex, name)
    flat = part.cpu()[:, :, 0].sum(0)
    check("dW6", flat[:NIN * C4].reshape(NIN, C4), ref, ex, name)
    check("db6", flat[NIN * C4:NIN * C4 + NIN], ref, ex, name)
    check("db4", flat[NIN * C4 + NIN:], ref, ex, name)
    if gs is not None:
        g4o, parto = ops.head_backward(dec, g["x"], g["mask"], g["var"], g["d4"], g["w6"], gs, g["gdec_ext"])
        assert torch.equal(g4o, g4) and torch.equal(parto, part), "head_backward: not bitwise reproducible"


# ======================================================================================================== latent tail
# (ids as they were while a second entry form, from enc.4's output, existed: "-False" is the (a3, coef3) form)
@pytest.mark.parametrize("B,nres", T.lt_cases(), ids=["%d-%d-False" % c for c in T.lt_cases()])
def test_latent_tail_every_patch_against_float64(lib, B, nres):
    """Every patch of every batch -- the second and third pass of the 512-workgroup grid included -- against the float64
    reference: z and every per-patch statistics slab, guard rows behind each output, the call repeated bit for bit."""
    from dynamorph_amd import _lib as L
    import ctypes
    a = T.lt_inputs(B, nres)
    ref = T.latent_tail_ref(**a)
    keep = []

    def P(t):
        t = dev(t)
        keep.append(t)
        return t.data_ptr()

    def run():
        args = L.LatentTailArgs()
        outs = []
        zb, z = guarded(B, 16, 16, 16)
        s4b, s4 = guarded(B, 16, 2, dtype=torch.float64)
        args.a3, args.coef3 = P(a["a3"]), P(a["coef3"])
        args.w10, args.b10, args.gamma4, args.beta4 = P(a["w10"]), P(a["b10"]), P(a["gamma4"]), P(a["beta4"])
        args.stats4, args.z, args.eps4 = s4.data_ptr(), z.data_ptr(), a["eps4"]
        args.B, args.C, args.CR, args.H, args.W, args.nres = B, 16, 32, 16, 16, nres
        outs.append(("stats4", s4b, s4))
        for i, (wa, ba, ga, bea, ea, wb, bb, gb, beb, eb) in enumerate(a["res"]):
            sab, sa = guarded(B, 32, 2, dtype=torch.float64)
            sbb, sb = guarded(B, 16, 2, dtype=torch.float64)
            r = args.res[i]
            r.wa, r.ba, r.gamma_a, r.beta_a, r.stats_a, r.eps_a = P(wa), P(ba), P(ga), P(bea), sa.data_ptr(), ea
            r.wb, r.bb, r.gamma_b, r.beta_b, r.stats_b, r.eps_b = P(wb), P(bb), P(gb), P(beb), sb.data_ptr(), eb
            outs += [(f"stats_a{i}", sab, sa), (f"stats_b{i}", sbb, sb)]
        assert lib.dm_latent_tail_forward(ctypes.byref(args), stream()) == 0
        torch.cuda.synchronize()
        return zb, z, outs

    zb, z, outs = run()
    what = f"latent tail B={B} nres={nres} a3"
    guard_ok(zb, "z")
    check("z", z, dict(z=ref["z"], b_z=ref["b_z"]), (), what)
    assert [n for n, _, _ in outs] == [n for n, _, _ in ref["stats"]]
    for (name, buf, got), (_, want, bound) in zip(outs, ref["stats"]):
        guard_ok(buf, name)
        check(name, got, {name: want, "b_" + name: bound}, (), what)
    _, z2, outs2 = run()
    assert torch.equal(z2, z) and all(torch.equal(p[2], q[2]) for p, q in zip(outs, outs2)), "not bitwise reproducible"


# ================================================================================================= enc.0 o enc.1
@pytest.mark.parametrize("kind", ["dyadic", "randn"])
@pytest.mark.parametrize("NIN,C0,C1", T.E1_SHAPES)
def test_e1_compose_border_and_chain_against_float64(ops, NIN, C0, C1, kind):
    w0, b0, w1, b1, dweff = T.e1_inputs(NIN, C0, C1, kind, (100 if kind == "dyadic" else 10) * C1 + NIN)
    ex = ("weff", "table", "dw0", "db0", "dw1") if kind == "dyadic" else ()
    weff_r, b_weff = T.e1_compose_ref(w0, b0, w1)
    table_r, b_table = T.e1_compose_border_ref(w0, b0, w1, b1)
    ch = T.e1_chain_ref(dweff, w0, b0, w1)
    ref = dict(weff=weff_r, b_weff=b_weff, table=table_r, b_table=b_table, **ch)
    w0d, b0d, w1d, b1d = dev(w0), dev(b0), dev(w1), dev(b1)
    what = f"e1 {kind} ({NIN}, {C0}, {C1})"
    weff, table = ops.e1_compose_border(w0d, b0d, w1d, b1d)
    check("weff", weff, ref, ex, what)
    check("table", table, ref, ex, what)
    assert torch.equal(ops.e1_compose(w0d, b0d, w1d), weff)
    bufs = [guarded(C0, NIN), guarded(C0), guarded(C1, C0, 4, 4)]
    ops.e1_chain(dev(dweff), w0d, b0d, w1d, bufs[0][1], bufs[1][1], bufs[2][1])
    for (buf, out), k in zip(bufs, ("dw0", "db0", "dw1")):
        guard_ok(buf, k)
        check(k, out, ref, ex, what)
