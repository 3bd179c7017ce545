"""The kernels between the convolutions -- channel statistics, BatchNorm finalisation (batch, per-sample, replay, backward),
apply, the slab reductions, the plain reconstruction loss, loss_finalize, Adam, augment and zscore_patch -- each against the
float64 reference and the derived bound of tests/helpers/glue_reference.py, at the slab counts, batch sizes, tails and NULL
pointers the one-shape tests of test_gpu_kernels.py do not reach.  Buffers the caller owns are pre-filled with NaN and
carry a guard row of a sentinel behind them that must come back untouched; raw _lib calls are used where ops allocates
the output itself or cannot express a NULL pointer.  No bound here comes from a GPU run (tests/test_glue_reference_host.py
derives and checks them on the host)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import glue_reference as G  # noqa: E402

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
    """(buffer, view): the view has `shape`, is pre-filled (NaN), and GUARD sentinel elements follow it."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), fill, dtype=dtype, device=DEV)
    buf[n:] = G.SENTINEL
    return buf, buf[:n].view(*shape)


def guard_ok(buf, what):
    assert bool((buf[-GUARD:] == G.SENTINEL).all()), f"{what}: the guard row behind the output was written"


def within(got, ref, bound, what):
    got = got.detach().cpu().double().reshape(ref.shape)
    assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} of {got.numel()} elements unwritten or NaN"
    err = (got - ref).abs()
    bad = err > bound
    worst = float(torch.nan_to_num(err / bound, nan=0.0).max())
    print(f"[glue gpu] {what}: worst error / bound {worst:.3f}")
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} beyond the bound, worst {worst:.2f} bounds (max err {err.max():.3e})"


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(t, dtype=None):
    return None if t is None else t.to(DEV, dtype).contiguous()


# =========================================================================================== channel statistics
def raw_channel_stats(lib, p, q):
    B, Cn, H, W = p.shape
    nb = lib.dm_channel_stats_num_blocks(B, Cn, H, W)
    buf, stats = guarded(nb, Cn, 2, dtype=torch.float64)
    assert lib.dm_channel_stats(ptr(p), ptr(q), ptr(stats), B, Cn, H, W, stream()) == 0
    return buf, stats


@pytest.mark.parametrize("case", G.stats_cases(), ids=lambda c: f"B{c[0]}-C{c[1]}-HW{c[2]}-{'q' if c[3] else 'sq'}-r{c[4]:g}")
def test_channel_stats(ops, lib, case):
    p, q = G.stats_inputs(case)
    pd, qd = dev(p), dev(q)
    buf, stats = raw_channel_stats(lib, pd, qd)
    assert stats.shape[0] == (case[0] + 31) // 32
    guard_ok(buf, "channel_stats")
    s1, s2, b1, b2 = G.channel_stats_ref(p, q)
    tot = stats.cpu().sum(0)                                        # float64 on the host
    within(tot[:, 0], s1, b1, "channel_stats sum p")
    within(tot[:, 1], s2, b2, "channel_stats sum p q")
    assert torch.equal(ops.channel_stats(pd, qd), stats)


# =========================================================================================== bn_finalize, batch mode
def raw_bn_finalize(lib, slabs, count, gamma, beta, rm, rv, nbt, mom, eps, per_sample=0, spg=1):
    nslabs, Cn = slabs.shape[0], slabs.shape[1]
    lead = (nslabs // spg, Cn) if per_sample else (Cn,)
    cbuf, coef = guarded(*lead, 4)
    sbuf, saved = guarded(*lead, 2)
    rc = lib.dm_bn_finalize(ptr(slabs), nslabs, spg, Cn, count, ptr(gamma), ptr(beta), ptr(rm), ptr(rv), ptr(nbt), mom, eps,
                            ptr(coef), ptr(saved), per_sample, stream())
    assert rc == 0
    guard_ok(cbuf, "bn_finalize coef")
    guard_ok(sbuf, "bn_finalize saved")
    return coef, saved


def check_coef(coef, saved, ref, what):
    within(coef[..., 0], ref["scale"], ref["b_scale"], what + " scale")
    within(coef[..., 2], ref["shift"], ref["b_shift"], what + " shift")
    assert float(coef[..., 1].abs().max()) == 0.0 and float(coef[..., 3].abs().max()) == 0.0
    within(saved[..., 0], ref["mean"], ref["b_mean"], what + " saved mean")
    within(saved[..., 1], ref["invstd"], ref["b_invstd"], what + " saved invstd")


@pytest.mark.parametrize("nslabs,Cn,count,mom,eps,form,seed", list(G.finalize_grid()))
def test_bn_finalize_on_synthetic_slabs(ops, lib, nslabs, Cn, count, mom, eps, form, seed):
    """form 0: everything given; 1: gamma / beta NULL; 2: running tensors NULL, counter given; 3: running and counter NULL.
    Channel 0 is constant (its variance clamps to exactly 0)."""
    gen = torch.Generator().manual_seed(seed)
    slabs = G.finalize_slabs(nslabs, Cn, count, seed)
    gamma, beta = torch.rand(Cn, generator=gen) + 0.5, torch.randn(Cn, generator=gen)
    rm0, rv0 = torch.randn(Cn, generator=gen), torch.rand(Cn, generator=gen) + 0.5
    if form == 1:
        gamma = beta = None
    track = form < 2
    rbuf, rm = guarded(Cn)
    vbuf, rv = guarded(Cn)
    rm.copy_(rm0)
    rv.copy_(rv0)
    nbt = torch.full((), 41, dtype=torch.int64, device=DEV)
    sd = dev(slabs)
    coef, saved = raw_bn_finalize(lib, sd, count, dev(gamma), dev(beta), rm if track else None, rv if track else None,
                                  nbt if form < 3 else None, mom, eps)
    ref = G.bn_finalize_ref(slabs.sum(0), count, gamma, beta, rm0, rv0, mom, eps)
    what = f"bn_finalize nslabs={nslabs} C={Cn} count={count}"
    check_coef(coef, saved, ref, what)
    assert float(ref["var"][0]) == 0.0                             # the constant channel: invstd = 1 / sqrt(eps)
    if track:
        within(rm, ref["rm"], ref["b_rm"], what + " running_mean")
        within(rv, ref["rv"], ref["b_rv"], what + " running_var")
    else:
        assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
    guard_ok(rbuf, "running_mean")
    guard_ok(vbuf, "running_var")
    assert int(nbt) == (42 if form < 3 else 41)                    # exactly one batch tracked
    if form == 0:
        rm2, rv2, nbt2 = dev(rm0), dev(rv0), torch.zeros((), dtype=torch.int64, device=DEV)
        c2, s2 = ops.bn_finalize(sd, count, dev(gamma), dev(beta), rm2, rv2, nbt2, mom, eps)
        assert torch.equal(c2, coef) and torch.equal(s2, saved) and torch.equal(rm2, rm) and torch.equal(rv2, rv)


# =========================================================================================== per-sample finalize, replay
@pytest.mark.parametrize("B,spg,Cn,count,mom,seed", list(G.per_sample_grid()))
def test_bn_finalize_per_sample_and_replay(ops, B, spg, Cn, count, mom, seed):
    gen = torch.Generator().manual_seed(seed)
    slabs = G.synthetic_slabs(B * spg, Cn, seed) * (count / spg)
    groups = slabs.reshape(B, spg, Cn, 2).sum(1)
    gamma, beta = torch.rand(Cn, generator=gen) + 0.5, torch.randn(Cn, generator=gen)
    rm0, rv0 = torch.randn(Cn, generator=gen), torch.rand(Cn, generator=gen) + 0.5
    sd, gd, bd = dev(slabs), dev(gamma), dev(beta)
    (rb1, rm1), (vb1, rv1), (rb2, rm2), (vb2, rv2) = guarded(Cn), guarded(Cn), guarded(Cn), guarded(Cn)
    for t, src in ((rm1, rm0), (rv1, rv0), (rm2, rm0), (rv2, rv0)):
        t.copy_(src)
    n1, n2 = torch.full((), 5, dtype=torch.int64, device=DEV), torch.full((), 5, dtype=torch.int64, device=DEV)
    coef, saved = ops.bn_finalize(sd, count, gd, bd, rm1, rv1, n1, mom, 1e-5, per_sample=True, slabs_per_group=spg)
    deferred = []
    coef2, saved2 = ops.bn_finalize(sd, count, gd, bd, rm2, rv2, n2, mom, 1e-5, per_sample=True, slabs_per_group=spg, defer=deferred)
    assert torch.equal(rm2.cpu(), rm0) and int(n2) == 5 and len(deferred) == 1       # untouched so far
    ops.bn_running_replay(deferred)
    assert not deferred
    assert torch.equal(coef, coef2) and torch.equal(saved, saved2)
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2) and int(n1) == int(n2) == 5 + B
    for b in (rb1, vb1, rb2, vb2):
        guard_ok(b, "per-sample running statistics")
    what = f"per-sample B={B} spg={spg} C={Cn} count={count}"
    check_coef(coef, saved, G.bn_finalize_ref(groups, count, gamma, beta, None, None, mom, 1e-5), what)
    rm, rv, b_rm, b_rv = G.bn_running_replay_ref(groups, count, rm0, rv0, mom)
    within(rm1, rm, b_rm, what + " replayed running_mean")
    within(rv1, rv, b_rv, what + " replayed running_var")


@pytest.mark.parametrize("nlayers", [1, 2, 16, 17])
def test_bn_running_replay_many_layers(ops, nlayers):
    """Layers of different C, B, slabs per sample and momentum in one bn_running_replay (the wrapper sends 16 per launch: 17 is
    two launches); the last layer has a counter but no running tensors."""
    deferred, want = [], []
    for k in range(nlayers):
        Cn, B, spg, mom = (3, 64, 16, 130, 1)[k % 5], (1, 9, 257, 33)[k % 4], (1, 2, 9)[k % 3], (0.1, 0.25, 0.5)[k % 3]
        slabs = G.synthetic_slabs(B * spg, Cn, 400 + k) * (64.0 / spg)
        gen = torch.Generator().manual_seed(400 + k)
        rm0, rv0 = torch.randn(Cn, generator=gen), torch.rand(Cn, generator=gen) + 0.5
        bare = k == nlayers - 1 and nlayers > 1
        rb, rm = guarded(Cn)
        vb, rv = guarded(Cn)
        rm.copy_(rm0)
        rv.copy_(rv0)
        nbt = torch.full((), k, dtype=torch.int64, device=DEV)
        deferred.append((dev(slabs), spg, 64, None if bare else rm, None if bare else rv, nbt, mom))
        want.append((slabs.reshape(B, spg, Cn, 2).sum(1), rm0, rv0, mom, rm, rv, rb, vb, nbt, k + B, bare))
    ops.bn_running_replay(deferred)
    assert not deferred
    for i, (groups, rm0, rv0, mom, rm, rv, rb, vb, nbt, nbt_want, bare) in enumerate(want):
        assert int(nbt) == nbt_want, f"layer {i}: num_batches_tracked {int(nbt)} != {nbt_want}"
        guard_ok(rb, f"layer {i} running_mean")
        guard_ok(vb, f"layer {i} running_var")
        if bare:
            assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)
            continue
        r_m, r_v, b_m, b_v = G.bn_running_replay_ref(groups, 64, rm0, rv0, mom)
        within(rm, r_m, b_m, f"replay of {nlayers} layers, layer {i} running_mean")
        within(rv, r_v, b_v, f"replay of {nlayers} layers, layer {i} running_var")


def test_bn_running_replay_refuses_bad_segment_counts(lib):
    from dynamorph_amd import _lib
    slabs = dev(G.synthetic_slabs(2, 3, 1))
    segs = (_lib.ReplaySeg * 17)()
    for i in range(17):
        segs[i] = _lib.ReplaySeg(slabs.data_ptr(), 2, 1, 3, 4, None, None, None, 0.1)
    assert lib.dm_bn_running_replay(segs, 17, stream()) < 0
    assert lib.dm_bn_running_replay(segs, 0, stream()) < 0


# =========================================================================================== bn_backward_finalize
@pytest.mark.parametrize("nslabs", G.SLAB_COUNTS)
def test_bn_backward_finalize_on_synthetic_slabs(ops, lib, nslabs):
    for k, Cn in enumerate((1, 5, 64, 130)):
        count = (0, 2, 2048 * 256, 100)[(k + nslabs) % 4]
        form = (k + nslabs) % 3                 # 0: everything given; 1: dgamma / dbeta NULL; 2: gamma NULL
        gen = torch.Generator().manual_seed(600 + nslabs + k)
        slabs = G.synthetic_slabs(nslabs, Cn, 600 + nslabs + k, mean=0.1)
        gamma = None if form == 2 else torch.rand(Cn, generator=gen) + 0.5
        saved = torch.stack([torch.randn(Cn, generator=gen), torch.rand(Cn, generator=gen) + 0.2], -1).contiguous()
        (gb, dgamma), (bb, dbeta), (cb, coef) = guarded(Cn), guarded(Cn), guarded(Cn, 4)
        sd, gd, svd = dev(slabs), dev(gamma), dev(saved)
        rc = lib.dm_bn_backward_finalize(ptr(sd), nslabs, Cn, count, ptr(gd), ptr(svd), None if form == 1 else ptr(dgamma),
                                         None if form == 1 else ptr(dbeta), ptr(coef), stream())
        assert rc == 0
        for b in (gb, bb, cb):
            guard_ok(b, "bn_backward_finalize")
        ref = G.bn_backward_ref(slabs.sum(0), count, gamma, saved)
        what = f"bn_backward_finalize nslabs={nslabs} C={Cn} count={count}"
        within(coef[:, 0], ref["A"], ref["b_A"], what + " A")
        within(coef[:, 1], ref["Bc"], ref["b_Bc"], what + " B")
        within(coef[:, 2], ref["Cc"], ref["b_Cc"], what + " C")
        assert float(coef[:, 3].abs().max()) == 0.0
        if count == 0:
            assert float(coef[:, 1].abs().max()) == 0.0 and float(coef[:, 2].abs().max()) == 0.0
        if form == 1:
            assert bool(torch.isnan(dgamma).all()) and bool(torch.isnan(dbeta).all())       # NULL: nothing written
        else:
            within(dgamma, ref["dgamma"], ref["b_dgamma"], what + " dgamma")
            within(dbeta, ref["dbeta"], ref["b_dbeta"], what + " dbeta")
        if form == 0:
            dg2, db2 = torch.empty(Cn, device=DEV), torch.empty(Cn, device=DEV)
            assert torch.equal(ops.bn_backward_finalize(sd, count, gd, svd, dg2, db2), coef)
            assert torch.equal(dg2, dgamma) and torch.equal(db2, dbeta)


# =========================================================================================== the two chains end to end
@pytest.mark.parametrize("r", [0.0, 3.0, 30.0])
@pytest.mark.parametrize("i", range(len(G.CHAIN_SHAPES)))
def test_bn_chain_batch_mode(ops, i, r):
    """channel_stats -> bn_finalize -> apply and channel_stats(dy, a) -> bn_backward_finalize -> apply(AFFINE2) against float64
    BatchNorm by autograd; r = |mean| / std of every channel (30: a post-ReLU channel with a large bias).  The bound carries
    the cancellation: C_VAR U (1 + r^2) on the variance, C_BWD U on the magnitude of the terms of B a + C."""
    B, Cn, h = G.CHAIN_SHAPES[i]
    a, dy, gamma, beta = G.chain_inputs(B, Cn, h, r, 300 + i)
    ref = G.bn_apply_chain_ref(a, dy, gamma, beta, 1e-5)
    ad, dyd, gd, bd = dev(a), dev(dy), dev(gamma), dev(beta)
    n = B * h * h
    rm, rv = torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    coef, saved = ops.bn_finalize(ops.channel_stats(ad), n, gd, bd, rm, rv, nbt, 0.1, 1e-5)
    ybuf, y = guarded(B, Cn, h, h)
    ops.apply(ops.Op(ad, 2, coef), B, Cn, h, h, out=y)
    guard_ok(ybuf, "apply")
    what = f"chain B={B} C={Cn} {h}x{h} r={r:g}"
    within(y, ref["y"], ref["b_y"], what + " y")
    (gb, dgamma), (bb, dbeta) = guarded(Cn), guarded(Cn)
    cb = ops.bn_backward_finalize(ops.channel_stats(dyd, ad), n, gd, saved, dgamma, dbeta)
    dbuf, da = guarded(B, Cn, h, h)
    ops.apply(ops.Op(dyd, 4, cb, p1=ad), B, Cn, h, h, out=da)
    for b in (gb, bb, dbuf):
        guard_ok(b, "chain backward")
    within(da, ref["da"], ref["b_da"], what + " da")
    within(dgamma, ref["dgamma"], ref["b_dgamma"], what + " dgamma")
    within(dbeta, ref["dbeta"], ref["b_dbeta"], what + " dbeta")


@pytest.mark.parametrize("r", [0.0, 3.0, 30.0])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_bn_chain_per_sample_forward(ops, i, r):
    B, Cn, h = G.CHAIN_SHAPES[i]
    a, dy, gamma, beta = G.chain_inputs(B, Cn, h, r, 350 + i)
    ref = G.bn_apply_chain_ref(a, dy, gamma, beta, 1e-5, per_sample=True)
    ad = dev(a)
    stats = torch.cat([ops.channel_stats(ad[b:b + 1]) for b in range(B)], 0)       # one slab per sample
    coef, _ = ops.bn_finalize(stats, h * h, dev(gamma), dev(beta), None, None, None, 0.1, 1e-5, per_sample=True, slabs_per_group=1)
    ybuf, y = guarded(B, Cn, h, h)
    ops.apply(ops.Op(ad, 2, coef, per_sample=True), B, Cn, h, h, out=y)
    guard_ok(ybuf, "apply")
    within(y, ref["y"], ref["b_y"], f"per-sample chain B={B} C={Cn} {h}x{h} r={r:g} y")


def test_apply_affine2_resid_per_sample_grid_stride(ops):
    """What the operand-contract table does not hold: resid together with AFFINE2 and per-sample coefficients at more than
    2048 x 256 float4, so that apply_kernel's grid-stride loop runs."""
    B, Cn, h = 9, 16, 128
    assert B * Cn * h * h // 4 > 2048 * 256
    gen = torch.Generator().manual_seed(77)
    p0, p1, res = (torch.randn(B, Cn, h, h, generator=gen) for _ in range(3))
    coef = torch.randn(B, Cn, 4, generator=gen)
    obuf, out = guarded(B, Cn, h, h)
    ops.apply(ops.Op(dev(p0), 4, dev(coef), p1=dev(p1), per_sample=True), B, Cn, h, h, resid=dev(res), out=out)
    guard_ok(obuf, "apply")
    c = coef.double().reshape(B, Cn, 4, 1, 1)
    t0, t1 = c[:, :, 0] * p0.double(), c[:, :, 1] * p1.double()
    ref = t0 + t1 + c[:, :, 2] + res.double()
    # two products, three adds, each on partial sums no larger than the sum of the terms' magnitudes
    within(out, ref, 5 * G.U * (t0.abs() + t1.abs() + c[:, :, 2].abs() + res.double().abs()), "apply AFFINE2 + resid, per-sample")


# =========================================================================================== sum_slabs, scatter
@pytest.mark.parametrize("nslabs", [1, 255, 257])
def test_sum_slabs_and_scatter(ops, nslabs):
    N = 37
    # (random doubles: sum_slabs_scatter promises sum_slabs' own order, so the bit-equality below is a statement about order)
    slabs = torch.randn(nslabs, N, 2, generator=torch.Generator().manual_seed(700 + nslabs), dtype=torch.float64)
    sd = dev(slabs)
    for scale in (1.0, 0.5, 1.0 / 3):
        dbuf, dst = guarded(N)
        ops.sum_slabs(sd, dst, scale=scale, n=N)
        guard_ok(dbuf, "sum_slabs")
        ref, bound = G.sum_slabs_ref(slabs, scale)
        within(dst, ref, bound + G.U * ref.abs(), f"sum_slabs nslabs={nslabs} scale={scale:.3f}")       # + the product's rounding
        for lens in ((N,), (1, N - 1), (1, 2, 3, 4, 5, 6, 7, 9)):
            outs = [guarded(ln) for ln in lens]
            ops.sum_slabs_scatter(sd, [v for _, v in outs], scale=scale)
            for b, _ in outs:
                guard_ok(b, "sum_slabs_scatter")
            assert torch.equal(torch.cat([v for _, v in outs]), dst), f"scatter to {len(lens)} destinations differs from sum_slabs"
    with pytest.raises(ValueError):
        ops.sum_slabs_scatter(sd, [torch.empty(N - 1, device=DEV)])
    with pytest.raises(ValueError):
        ops.sum_slabs(sd, torch.empty(N - 1, device=DEV))          # a destination shorter than the slab rows
    with pytest.raises(ValueError):
        ops.sum_slabs(sd, torch.empty(N, device=DEV), n=N - 1)


# =========================================================================================== reduce_slabs, reduce_slabs_multi
@pytest.mark.parametrize("E", [1, 63, 64, 65])
def test_reduce_slabs_orders(ops, E):
    for n in (1, 15, 16, 17, 63, 64, 65, 512):
        s = torch.randn(n, E, generator=torch.Generator().manual_seed(n * 100 + E))
        exact, bound, order = G.reduce_slabs_ref(s)
        sd = dev(s)
        (b1, d1), (b2, d2) = guarded(E), guarded(E)
        ops.reduce_slabs(sd, d1)
        pending = [(sd, d2)]
        ops.reduce_slabs_multi(pending)
        assert not pending
        guard_ok(b1, "reduce_slabs")
        guard_ok(b2, "reduce_slabs_multi")
        assert torch.equal(d1.cpu(), order), f"reduce_slabs n={n} E={E}: not the promised order"
        assert torch.equal(d2.cpu(), order), f"reduce_slabs_multi n={n} E={E}: not the promised order"
        within(d1, exact, bound, f"reduce_slabs n={n} E={E}")


@pytest.mark.parametrize("entries", [1, 32, 33, 70])
def test_reduce_slabs_multi_mixed_pending_list(ops, entries):
    """Float slabs mixed with pend_stats runs (several destinations per statistics tensor: first column non-zero, stride != E);
    the wrapper cuts the list into launches of 32."""
    pending, checks = [], []
    k = 0
    while len(pending) < entries:
        n, E = (1, 15, 16, 17, 63, 64, 65, 512)[k % 8], (1, 63, 64, 65, 200)[k % 5]
        if k % 3 == 2 and entries - len(pending) >= 3:
            # random doubles, NOT the exact grid of synthetic_slabs: this kernel adds sixteen groups with two accumulators,
            # sum_slabs 256 threads and a block sum -- both "in double", so both are held to the float64 bound, not to each other
            stats = torch.randn(n, 1 + E + 7, 2, generator=torch.Generator().manual_seed(900 + k), dtype=torch.float64)
            sd = dev(stats)
            outs = [guarded(1), guarded(E), guarded(7)]
            ops.pend_stats(pending, sd, [v for _, v in outs])
            want = torch.empty(1 + E + 7, device=DEV)
            ops.sum_slabs(sd, want)
            checks.append(("dbl", outs, want, G.sum_slabs_ref(stats)))
        else:
            s = torch.randn(n, E, generator=torch.Generator().manual_seed(900 + k))
            buf, dst = guarded(E)
            pending.append((dev(s), dst))
            checks.append(("f32", [(buf, dst)], None, G.reduce_slabs_ref(s)))
        k += 1
    assert len(pending) == entries
    ops.reduce_slabs_multi(pending)
    assert not pending
    for kind, outs, want, ref in checks:
        for b, _ in outs:
            guard_ok(b, "reduce_slabs_multi")
        got = torch.cat([v for _, v in outs])
        if kind == "dbl":
            within(got, ref[0], ref[1], "reduce_slabs_multi statistics run")
            within(want, ref[0], ref[1], "sum_slabs on the same statistics")
        else:
            assert torch.equal(got.cpu(), ref[2]), "float segment: not the promised order"
            within(got, ref[0], ref[1], "reduce_slabs_multi float segment")
    with pytest.raises(ValueError):
        ops.pend_stats([], dev(G.synthetic_slabs(2, 5, 1)), [torch.empty(4, device=DEV)])


# =========================================================================================== reconstruction loss
@pytest.mark.parametrize("i", range(len(G.RECON_CASES)))
def test_recon_loss_and_backward(ops, lib, i):
    B, NIN, h, mc = G.RECON_CASES[i]
    dec, x, mask, var = G.recon_inputs(B, NIN, h, mc, 500 + i)
    ref = G.recon_loss_ref(dec, x, mask, var, 1.3)
    dd, xd, md, vd = dev(dec), dev(x), dev(mask), dev(var)
    nb = lib.dm_recon_loss_num_blocks(B, NIN, h, h)
    assert nb == G.recon_blocks(B, NIN)          # (above 1024 planes with 1024 % NIN != 0 a block crosses channels)
    lbuf, lslabs = guarded(nb, dtype=torch.float64)
    assert lib.dm_recon_loss(ptr(dd), ptr(xd), ptr(md), mc or 0, ptr(vd), ptr(lslabs), B, NIN, h, h, stream()) == 0
    guard_ok(lbuf, "recon_loss slabs")
    assert torch.equal(ops.recon_loss(dd, xd, md, vd), lslabs)
    what = f"recon B={B} NIN={NIN} {h}x{h} mask={mc}"
    vq = torch.tensor([0.37, 11.0], device=DEV)
    out = ops.loss_finalize(lslabs, dec.numel(), vq, 0.7, 0.3)
    within(out[0], ref["loss"], ref["b_loss"], what + " loss")
    gs = torch.tensor([1.3], device=DEV)
    gbuf, g = guarded(B, NIN, h, h)
    bbuf, bias_slabs = guarded(nb, NIN, 2, dtype=torch.float64)
    assert lib.dm_recon_loss_backward(ptr(dd), ptr(xd), ptr(md), mc or 0, ptr(vd), ptr(gs), ptr(g), ptr(bias_slabs), B, NIN, h, h,
                                      stream()) == 0
    guard_ok(gbuf, "recon_loss_backward g")
    guard_ok(bbuf, "recon_loss_backward bias slabs")
    g2, part2 = ops.recon_loss_backward(dd, xd, md, vd, gs)
    assert torch.equal(g2, g) and torch.equal(part2, bias_slabs)
    within(g, ref["g"], ref["b_g"], what + " g_decoded")
    sbuf, bias = guarded(NIN)
    ops.sum_slabs(bias_slabs, bias)
    guard_ok(sbuf, "bias sums")
    within(bias, ref["bias"], ref["b_bias"], what + " per-channel sums")


@pytest.mark.parametrize("nslabs", [1, 255, 257, 1024])
def test_loss_finalize_on_synthetic_slabs(ops, nslabs):
    slabs = G.synthetic_slabs(nslabs, 1, 800 + nslabs, mean=2.0)[:, 0, 1].contiguous()
    count = 3 * 70 * 64 * 64
    vq = torch.tensor([0.37, 11.0])
    wr, wc = 0.7, 0.3
    out = ops.loss_finalize(dev(slabs), count, dev(vq), wr, wc).cpu().double()
    recon = float(slabs.sum()) / count
    commit = float(vq[0])
    total = G.f32(wr) * recon + G.f32(wc) * commit
    assert abs(float(out[0]) - recon) <= G.U * recon
    assert float(out[1]) == commit and float(out[3]) == 11.0
    assert abs(float(out[2]) - total) <= 4 * G.U * total           # recon's store, two products, one sum (all positive)


# =========================================================================================== Adam
def adam_buffers(p, g, m, v, off):
    """The four vectors as views at float offset `off` into flat NaN buffers (how the trainer calls the kernel)."""
    n = p.numel()
    flats, views = [], []
    for t in (p, g, m, v):
        flat = torch.full((n + off + 5,), NAN, device=DEV)
        flat[off:off + n] = t.to(DEV)
        flats.append(flat)
        views.append(flat[off:off + n])
    return flats, views


def outside_untouched(flats, off, n):
    return all(bool(torch.isnan(f[:off]).all()) and bool(torch.isnan(f[off + n:]).all()) for f in flats)


def adam_cases():
    k = 0
    for n in (1, 255, 256, 257, 5000, 262144, 262145, 1_000_003):
        reps = 6 if n <= 5000 else 2
        for _ in range(reps):
            yield n, G.ADAM_STEPS[k % 6], G.ADAM_GSCALES[(k // 2 + k) % 6], k % 2, (0, 1, 3)[k % 3], k
            k += 1
    for t in G.ADAM_STEPS:                      # the whole step x gradient-scale x hyper-parameter product at n = 5000
        for gi in range(6):
            for h in (0, 1):
                yield 5000, t, G.ADAM_GSCALES[gi], h, (0, 1, 3)[(gi + h) % 3], k
                k += 1


@pytest.mark.parametrize("n,t,gsc,hyper,off,seed", list(adam_cases()))
def test_adam_against_float64(ops, n, t, gsc, hyper, off, seed):
    lr, b1, b2, eps = G.ADAM_HYPER[hyper]
    p, g, m, v = G.adam_state(n, t, gsc, seed)
    ref = G.adam_ref(p, g, m, v, t, lr, b1, b2, eps)
    flats, (pv, gv, mv, vv) = adam_buffers(p, g, m, v, off)
    step = torch.tensor([float(t)], device=DEV)
    ops.adam(pv, gv, mv, vv, lr, b1, b2, eps, step)
    assert outside_untouched(flats, off, n), "Adam wrote outside its views"
    assert torch.equal(gv.cpu(), g) and float(step) == float(t)
    what = f"adam n={n} t={t} gscale={gsc:g} hyper={hyper} offset={off}"
    within(mv, ref["m"], ref["b_m"], what + " m")
    within(vv, ref["v"], ref["b_v"], what + " v")
    within(pv, ref["p"], ref["b_p"], what + " p")


def test_adam_counted_ping_pong_equals_adam(ops):
    n = 262145
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(2))
    pa, pb = dev(p0), dev(p0)
    ma, va, mb, vb = (torch.zeros(n, device=DEV) for _ in range(4))
    step, cnt = torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
    for s in range(10):
        g = dev(torch.randn(n, generator=torch.Generator().manual_seed(20 + s)) * 0.1)
        step += 1
        ops.adam(pa, g, ma, va, 1e-3, 0.9, 0.999, 1e-8, step)
        a, b = s % 2, 1 - s % 2
        ops.adam_counted(pb, g, mb, vb, 1e-3, 0.9, 0.999, 1e-8, cnt[a:a + 1], cnt[b:b + 1])
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert float(cnt[0]) == 10.0 and float(cnt[1]) == 9.0
    with pytest.raises(ValueError):
        ops.adam_counted(pb, g, mb, vb, 1e-3, 0.9, 0.999, 1e-8, cnt[0:1], cnt[0:1])
    with pytest.raises(ValueError):
        ops.adam_counted(pb, g, mb, vb, 1e-3, 0.9, 0.999, 1e-8, cnt[0:1], cnt[0:1], grad_scale=0.5)


@pytest.mark.parametrize("scale", [0.5, 0.25, 1.0 / 3])
def test_adam_counted_grad_scale(ops, scale):
    n, t = 262145, 10
    lr, b1, b2, eps = G.ADAM_HYPER[0]
    p, g, m, v = G.adam_state(n, t, 1.0, 31)
    ref = G.adam_ref(p, g, m, v, t, lr, b1, b2, eps, scale)
    fa, (pa, ga, ma, va) = adam_buffers(p, g, m, v, 1)
    fb, (pb, gb, mb, vb) = adam_buffers(p, g, m, v, 3)
    cnt = torch.tensor([t - 1.0, 0.0], device=DEV)
    ops.adam_counted(pa, ga, ma, va, lr, b1, b2, eps, cnt[0:1], cnt[1:2], grad_scale=scale)
    assert float(cnt[1]) == float(t) and outside_untouched(fa, 1, n)
    gs = gb * torch.tensor(scale, dtype=torch.float32, device=DEV)              # g * float32(scale), in fp32 on the device
    ops.adam(pb, gs, mb, vb, lr, b1, b2, eps, torch.tensor([float(t)], device=DEV))
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    what = f"adam_counted grad_scale={scale:.3f}"
    within(ma, ref["m"], ref["b_m"], what + " m")
    within(va, ref["v"], ref["b_v"], what + " v")
    within(pa, ref["p"], ref["b_p"], what + " p")


def test_adam_matches_torch_adam_at_step_1000(ops):
    """One comparison with torch.optim.Adam (fp32, CPU) at the tolerance of test_gpu_kernels.py::test_adam_matches_torch."""
    n, t = 262145, 1000
    p, g, m, v = G.adam_state(n, t, 1.0, 47)
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-4, betas=(.9, .999))
    pr.grad = g.clone()
    opt.step()                                                     # creates the state; then overwrite it
    with torch.no_grad():
        pr.copy_(p)
    st = opt.state[pr]
    st["step"] = torch.tensor(float(t - 1))
    st["exp_avg"].copy_(m)
    st["exp_avg_sq"].copy_(v)
    opt.step()
    pd, md, vd = dev(p), dev(m), dev(v)
    ops.adam(pd, dev(g), md, vd, 1e-4, 0.9, 0.999, 1e-8, torch.tensor([float(t)], device=DEV))
    err = (pd.cpu().double() - pr.detach().double()).abs()
    assert bool((err <= 1e-7 + 1e-6 * pr.detach().double().abs()).all()), f"max err {err.max():.3e}"


# =========================================================================================== augment, zscore_patch
@pytest.mark.parametrize("Cn,h", [(1, 4), (2, 16), (4, 128), (1, 128), (4, 4)])
def test_augment_all_pairs(ops, Cn, h):
    B = 37
    x = torch.randn(B, Cn, h, h, generator=torch.Generator().manual_seed(h + Cn))
    flips = torch.tensor([(b % 12) // 4 for b in range(B)], dtype=torch.int32)     # all 12 (flip, rot) pairs, three times
    rots = torch.tensor([b % 4 for b in range(B)], dtype=torch.int32)
    rots[12:16] += 4                                                # 4..7 and ...
    rots[24:28] -= 4                                                # ... -4..-1 behave as rot & 3 (include/dynamorph_hip.h)
    rots[36] = 5
    ref = []
    for i in range(B):
        img = x[i]
        if flips[i] != 0:
            img = torch.flip(img, dims=(int(flips[i]),))
        ref.append(torch.rot90(img, k=int(rots[i]) & 3, dims=[1, 2]))
    out = ops.augment(dev(x), dev(flips), dev(rots))
    assert torch.equal(out.cpu(), torch.stack(ref))
    assert {(int(f), int(r) & 3) for f, r in zip(flips, rots)} == {(f, r) for f in range(3) for r in range(4)}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("shape", [(3, 2, 2, 2), (2, 3, 10, 10), (5, 1, 15, 17), (2, 2, 1, 257), (2, 2, 128, 128)])
def test_zscore_patch_plane_sizes(ops, dtype, shape):
    g = torch.Generator().manual_seed(shape[2] * shape[3])
    x = (torch.rand(*shape, generator=g, dtype=torch.float64) * 3000 + 100).to(dtype)
    x[0, 0] = 7.0                                                   # a constant plane: 0 / eps
    xn = x.numpy().astype(np.float64)
    ref = ((xn - xn.mean((2, 3), keepdims=True)) / (xn.std((2, 3), keepdims=True) + np.finfo(float).eps)).astype(np.float32)
    out = ops.zscore_patch(x.to(DEV)).cpu()
    assert out.dtype == torch.float32 and not torch.isnan(out).any()
    assert torch.equal(out[0, 0], torch.zeros(shape[2], shape[3]))
    r = torch.from_numpy(ref).double()
    err = (out.double() - r).abs()
    # numpy adds pairwise, the kernel thread by thread: the float64 results differ in their last bits, so the float32 values
    # are equal except where that crosses a rounding boundary (one ulp = 2 U); the existing test's 2e-7 holds a fortiori
    assert bool((err <= 2 * G.U * r.abs() + 1e-30).all()), f"max err {err.max():.3e}"
    assert float((out != torch.from_numpy(ref)).double().mean()) <= 1e-3
