"""GPU: the per-patch scoring kernels (dm_vq_patch_scalars, dm_dec_tail_score, dm_recon_loss_per_sample, dm_score_finalize)
against float64 references evaluated on the host, patch by patch, and the identities that make a value "per patch": the
same to the bit whatever the batch, the patch's position and its neighbours.

The decoder tail's yardstick is tests/helpers/tail_reference.py::dec_tail_ref on each single-patch slice (its `loss` is the
patch's recon_loss, `b_loss` its counted bound); the per-channel bound restates the same expression for one channel.  The
scoring form runs the forward kernel's own fp32 chain per lane and tile (the term 3 roundings, the pair sum 1, the chain over
5 NIN <= 20 row terms: the 24 of C_TAIL_LOSS) and credits each step's increment, taken exactly in double, to the step's
channel; everything after that is summed in double.  The constant therefore covers the patch's recon_loss as it covers the
forward kernel's loss.  For ONE channel the expression is restated as it stands, with this caveat: a step's rounding is
relative to the lane's running sum over all channels of the tile, so a channel whose terms are far smaller than its
neighbours' carries roundings its own terms do not count (measured: at most 0.10 of the bound, in the four-channel case
whose channel variances span a factor of 31; 0.002 - 0.007 elsewhere)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tail_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64
SENT = T.SENTINEL


@pytest.fixture(scope="module")
def lib():
    from dynamorph_amd import _lib
    return _lib.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(*shape, dtype=torch.float32):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENT, dtype=dtype, device=DEV)
    return buf, buf[:n].view(*shape)


def guard_ok(buf, what):
    assert bool((buf[-GUARD:] == torch.tensor(SENT).to(buf.dtype)).all()), f"{what}: the guard row behind the output was written"


def ptr(t):
    return None if t is None else t.data_ptr()


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


# ====================================================================================== dm_vq_patch_scalars
def vq_call(lib, z, idx, cb, cc, want_counts):
    B, D, H, W = z.shape
    K = cb.shape[0]
    sbuf, sc = guarded(B, 3)
    cbuf, cnt = guarded(B, K, dtype=torch.int32) if want_counts else (None, None)
    assert lib.dm_vq_patch_scalars(ptr(z), ptr(idx), ptr(cb), cc, ptr(sc), ptr(cnt), B, D, K, H, W, stream()) == 0
    torch.cuda.synchronize()
    guard_ok(sbuf, "scalars")
    if want_counts:
        guard_ok(cbuf, "counts")
    return sc, cnt


def vq_hold(lib, z, idx, cb, cc, what):
    B, D, H, W = z.shape
    K = cb.shape[0]
    sc, cnt = vq_call(lib, dev(z), dev(idx), dev(cb), cc, True)
    sc0, _ = vq_call(lib, dev(z), dev(idx), dev(cb), cc, False)
    assert torch.equal(bits(sc), bits(sc0)), f"{what}: counts = NULL changes the scalars"
    sc = sc.cpu().double().numpy()
    q = cb.double()[idx].permute(0, 3, 1, 2)
    mse = ((q - z.double()) ** 2).mean((1, 2, 3)).numpy()
    want_cnt = np.stack([np.bincount(idx[i].reshape(-1).numpy(), minlength=K) for i in range(B)])
    assert np.array_equal(cnt.cpu().numpy(), want_cnt), f"{what}: counts"
    p = want_cnt / float(H * W)
    perp = np.exp(-(p * np.log(p + 1e-10)).sum(1))
    e_mse = np.abs(sc[:, 2] - mse) / mse
    e_loss = np.abs(sc[:, 0] - (1 + cc) * mse) / mse
    e_perp = np.abs(sc[:, 1] - perp) / perp
    print(f"[score gpu] {what}: mse {e_mse.max():.2e}, loss {e_loss.max():.2e}, perplexity {e_perp.max():.2e} (relative)")
    assert e_mse.max() <= 2e-6 and e_loss.max() <= 2e-6 and e_perp.max() <= 1e-4, (what, e_mse, e_loss, e_perp)


@pytest.mark.parametrize("B,D,K,H,W", [(3, 16, 64, 16, 16), (2, 64, 512, 8, 8), (2, 8, 5, 5, 7), (2, 16, 4096, 8, 8),
                                       (2, 4, 5000, 6, 6)])     # (the last: beyond one window of counters)
def test_vq_patch_scalars_against_float64(lib, B, D, K, H, W):
    gen = torch.Generator().manual_seed(B * 1000 + K)
    z = torch.randn(B, D, H, W, generator=gen)
    cb = torch.randn(K, D, generator=gen)
    idx = torch.randint(0, K, (B, H, W), generator=gen)
    vq_hold(lib, z, idx, cb, 0.25, f"B{B} D{D} K{K} {H}x{W}")


def test_vq_patch_scalars_single_code_and_uniform_patches(lib):
    """One patch uses a single code (perplexity 1), its neighbour every code equally (perplexity K), a third is random: a
    histogram shared by the batch would give all three the same value."""
    gen = torch.Generator().manual_seed(5)
    K, D, H, W = 64, 16, 16, 16
    z = torch.randn(3, D, H, W, generator=gen)
    cb = torch.randn(K, D, generator=gen)
    idx = torch.stack([torch.full((H, W), 17), (torch.arange(H * W) % K).reshape(H, W), torch.randint(0, K, (H, W), generator=gen)])
    vq_hold(lib, z, idx, cb, 0.4, "single / uniform / random")
    sc, _ = vq_call(lib, dev(z), dev(idx), dev(cb), 0.4, False)
    perp = sc[:, 1].cpu().double().numpy()
    assert abs(perp[0] - 1.0) <= 1e-4 and abs(perp[1] - K) <= 1e-4 * K
    # position in the batch and the neighbours do not matter: reversed order, and patch 1 alone
    scr, _ = vq_call(lib, dev(z.flip(0)), dev(idx.flip(0)), dev(cb), 0.4, False)
    assert torch.equal(bits(scr.flip(0)), bits(sc))
    sc1, _ = vq_call(lib, dev(z[1:2]), dev(idx[1:2]), dev(cb), 0.4, False)
    assert torch.equal(bits(sc1), bits(sc[1:2]))


# ========================================================================================= dm_dec_tail_score
TAIL_CASES = [(3, 2, 16, 64, None, True), (2, 1, 8, 100, 1, True), (2, 4, 8, 4, "nin", False), (1, 3, 16, 128, None, True),
              (100, 2, 64, 64, 1, True)]          # (B, NIN, H2, W2, mask channels, b6 given)
TAIL_IDS = ["B3-n2-16x64", "B2-n1-8x100-m1", "B2-n4-8x4-mnin-nob6", "B1-n3-16x128", "B100-n2-64x64-m1"]


def tail_score(lib, g, want_decoded):
    d2 = g["d2"]
    B, _, H2, W2 = d2.shape
    NIN = g["w6"].shape[0]
    mc = 0 if g["mask"] is None else g["mask"].shape[1]
    wsb = lib.dm_dec_tail_score_workspace_bytes(B, NIN, H2, W2)
    wbuf, ws = guarded(wsb // 8, dtype=torch.float64)
    pbuf, ps = guarded(B, NIN, dtype=torch.float64)
    dbuf, dec = guarded(B, NIN, 2 * H2, 2 * W2) if want_decoded else (None, None)
    rc = lib.dm_dec_tail_score(ptr(d2), ptr(g["w4"]), ptr(g["b4"]), ptr(g["w6"]), ptr(g["b6"]), ptr(g["x"]), ptr(g["mask"]), mc,
                               ptr(g["var"]), ptr(dec), ptr(ps), ptr(ws), wsb, B, 4, NIN, H2, W2, stream())
    assert rc == 0
    torch.cuda.synchronize()
    guard_ok(wbuf, "workspace"), guard_ok(pbuf, "patch sums")
    if want_decoded:
        guard_ok(dbuf, "decoded")
    return ps, dec


def take(g, sel):
    """The device operands of the patches `sel` (an index tensor or slice)."""
    out = dict(g)
    for k in ("d2", "x", "mask"):
        out[k] = None if g[k] is None else g[k][sel].contiguous()
    return out


@functools.lru_cache(maxsize=None)
def tail_case(i):
    """Inputs, device operands, the kernel's sums (decoded = NULL) and the float64 reference per single-patch slice: once per
    case, shared by the tests below and left unchanged."""
    from dynamorph_amd import _lib
    lib = _lib.load()
    B, NIN, H2, W2, mk, has_b6 = TAIL_CASES[i]
    a = T.tail_inputs(T._case("randn", B, NIN, H2, W2, mk, 7100 + i))
    if not has_b6:
        a["b6"] = None
    g = {k: dev(v) for k, v in a.items() if k != "gscale"}
    sums, _ = tail_score(lib, g, False)
    OH, OW = 2 * H2, 2 * W2
    U = T.U
    recon, b_recon, chan, b_chan = [], [], [], []
    for b in range(B):
        m = None if a["mask"] is None else a["mask"][b:b + 1]
        r = T.dec_tail_ref(a["d2"][b:b + 1], a["w4"], a["b4"], a["w6"], a["b6"], a["x"][b:b + 1], m, a["var"], 1.0)
        recon.append(float(r["loss"])), b_recon.append(float(r["b_loss"]))
        # dec_tail_ref's loss and b_loss, restated for one channel at a time (mean over the channel's 2H2 x 2W2 pixels)
        dec, b_dec = r["decoded"], r["b_decoded"]
        X = a["x"][b:b + 1].double()
        M = torch.ones_like(dec) if m is None else m.double().expand_as(dec)
        V = a["var"].double().reshape(1, -1, 1, 1)
        t = dec * M - X * M
        dt = M.abs() * b_dec + 2 * U * ((dec * M).abs() + (X * M).abs())
        chan.append((t * t / V).sum((0, 2, 3)) / (OH * OW))
        b_chan.append(((2 * t.abs() * dt + dt * dt) / V + T.C_TAIL_LOSS * U * t * t / V).sum((0, 2, 3)) / (OH * OW))
    ref = dict(recon=torch.tensor(recon, dtype=torch.float64), b_recon=torch.tensor(b_recon, dtype=torch.float64),
               chan=torch.stack(chan), b_chan=torch.stack(b_chan))
    return a, g, sums, ref


@pytest.mark.parametrize("i", range(len(TAIL_CASES)), ids=TAIL_IDS)
def test_dec_tail_score_against_float64_per_patch(lib, i):
    a, g, sums, ref = tail_case(i)
    B, NIN, H2, W2 = TAIL_CASES[i][:4]
    hw = 4.0 * H2 * W2
    s = sums.cpu()
    assert not torch.isnan(s).any() and not (s == SENT).any()
    chan, recon = s / hw, s.sum(1) / (NIN * hw)
    e_c, e_r = (chan - ref["chan"]).abs(), (recon - ref["recon"]).abs()
    print(f"[score gpu] {TAIL_IDS[i]}: worst error / bound: recon {float((e_r / ref['b_recon']).max()):.3f}, "
          f"per channel {float((e_c / ref['b_chan']).max()):.3f}")
    assert not (e_r > ref["b_recon"]).any(), (e_r / ref["b_recon"]).max()
    assert not (e_c > ref["b_chan"]).any(), (e_c / ref["b_chan"]).max()


def forward_tail(lib, g):
    """dm_dec_tail_forward on the same operands: (decoded, loss slabs)."""
    B, _, H2, W2 = g["d2"].shape
    NIN = g["w6"].shape[0]
    mc = 0 if g["mask"] is None else g["mask"].shape[1]
    fbuf, fdec = guarded(B, NIN, 2 * H2, 2 * W2)
    lbuf, ls = guarded(lib.dm_dec_tail_num_blocks(B, H2, W2), dtype=torch.float64)
    assert lib.dm_dec_tail_forward(ptr(g["d2"]), ptr(g["w4"]), ptr(g["b4"]), ptr(g["w6"]), ptr(g["b6"]), ptr(g["x"]), ptr(g["mask"]),
                                   mc, ptr(g["var"]), ptr(fdec), ptr(ls), B, 4, NIN, H2, W2, stream()) == 0
    torch.cuda.synchronize()
    return fdec, ls


@pytest.mark.parametrize("i", range(len(TAIL_CASES)), ids=TAIL_IDS)
def test_dec_tail_score_decoded_and_forward_kernel(lib, i):
    """decoded = NULL or not: bit-equal sums; decoded bit-equal to dm_dec_tail_forward's."""
    a, g, sums, ref = tail_case(i)
    sums_d, dec = tail_score(lib, g, True)
    assert torch.equal(bits(sums_d), bits(sums))
    fdec, _ = forward_tail(lib, g)
    assert torch.equal(bits(dec), bits(fdec))


@pytest.mark.parametrize("i", range(len(TAIL_CASES)), ids=TAIL_IDS)
def test_dec_tail_score_total_equals_the_forward_slabs_total(lib, i):
    """The sum of all patch sums against the sum of dm_dec_tail_forward's slabs, to 1e-12 relative: the channels of a lane add
    up to the forward kernel's own fp32 chain for that lane and tile (each step's increment is credited to its channel in
    double, where the difference is exact), so the two totals differ by the order of their double additions only
    (measured on the MI355X: 0 in four cases, 1.8e-16 with 100 patches)."""
    a, g, sums, ref = tail_case(i)
    _, ls = forward_tail(lib, g)
    tot_s, tot_f = float(sums.cpu().sum()), float(ls.cpu().sum())
    rel = abs(tot_s - tot_f) / abs(tot_f)
    print(f"[score gpu] {TAIL_IDS[i]}: sum of patch sums {tot_s!r}, sum of forward slabs {tot_f!r}, relative difference {rel:.3e}")
    assert rel <= 1e-12, rel


@pytest.mark.parametrize("i", range(len(TAIL_CASES)), ids=TAIL_IDS)
def test_dec_tail_score_is_per_patch(lib, i):
    """Permuting the patches permutes the rows bit for bit; a patch alone reproduces its row; one pixel of x changes one row."""
    a, g, sums, ref = tail_case(i)
    B, NIN, H2, W2 = TAIL_CASES[i][:4]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(i))
    sums_p, _ = tail_score(lib, take(g, perm.to(DEV)), False)
    assert torch.equal(bits(sums_p), bits(sums[perm.to(DEV)]))
    for b in sorted({0, B // 2, B - 1}):
        one, _ = tail_score(lib, take(g, slice(b, b + 1)), False)
        assert torch.equal(bits(one), bits(sums[b:b + 1])), b
    b = B - 1
    g2 = dict(g)
    g2["x"] = g["x"].clone()
    g2["x"][b, NIN - 1, 2 * H2 - 1, 2 * W2 - 1] += 3.0
    if g["mask"] is not None:
        g2["mask"] = g["mask"].clone()
        g2["mask"][b, :, 2 * H2 - 1, 2 * W2 - 1] = 1.0
        base, _ = tail_score(lib, dict(g, mask=g2["mask"]), False)
    else:
        base = sums
    moved, _ = tail_score(lib, g2, False)
    diff = bits(moved) != bits(base)
    assert bool(diff[b, NIN - 1]) and int(diff.sum()) == 1


def test_dec_tail_score_argument_errors(lib):
    d = torch.zeros(8, device=DEV)
    p = d.data_ptr()
    assert lib.dm_dec_tail_score(p, p, p, p, p, None, None, 0, p, None, p, p, 1 << 20, 1, 4, 2, 8, 64, None) == -1      # x required
    assert lib.dm_dec_tail_score(p, p, p, p, p, p, None, 0, p, None, p, p, 8, 1, 4, 2, 8, 64, None) == -1               # workspace too small
    assert b"workspace" in lib.dm_last_error()
    assert lib.dm_dec_tail_score(p, p, p, p, p, p, None, 0, p, None, p, p, 1 << 20, 1, 8, 2, 8, 64, None) == -1         # C2 not built
    assert lib.dm_dec_tail_score_workspace_bytes(1024, 2, 64, 64) == 1024 * 8 * 4 * 2 * 8


# ==================================================================================== dm_recon_loss_per_sample
RL_CASES = [(3, 2, 128, 128, 1), (2, 3, 50, 34, "nin"), (5, 1, 8, 8, None), (2, 2, 7, 9, 1)]     # (the last: H*W odd)


def recon_call(lib, dec, x, mask, var):
    B, NIN, H, W = dec.shape
    mc = 0 if mask is None else mask.shape[1]
    pbuf, ps = guarded(B, NIN, dtype=torch.float64)
    assert lib.dm_recon_loss_per_sample(ptr(dec), ptr(x), ptr(mask), mc, ptr(var), ptr(ps), B, NIN, H, W, stream()) == 0
    torch.cuda.synchronize()
    guard_ok(pbuf, "patch sums")
    return ps


@pytest.mark.parametrize("B,NIN,H,W,mk", RL_CASES)
def test_recon_loss_per_sample_against_float64(lib, B, NIN, H, W, mk):
    """dec_tail_ref's loss expression with b_dec = 0 (decoded is an input here), per patch and per channel."""
    gen = torch.Generator().manual_seed(B * 100 + H)
    dec, x = torch.randn(B, NIN, H, W, generator=gen), torch.randn(B, NIN, H, W, generator=gen)
    mask = T._mask(gen, B, NIN if mk == "nin" else mk, H, W)
    var = torch.logspace(-1.0, 0.5, NIN) if NIN > 1 else torch.tensor([0.3])
    g = [dev(dec), dev(x), dev(mask), dev(var)]
    sums = recon_call(lib, *g)
    D, X, V, U = dec.double(), x.double(), var.double().reshape(1, -1, 1, 1), T.U
    M = torch.ones_like(D) if mask is None else mask.double().expand_as(D)
    t = D * M - X * M
    dt = 2 * U * ((D * M).abs() + (X * M).abs())
    chan = (t * t / V).sum((2, 3)) / (H * W)
    b_chan = ((2 * t.abs() * dt + dt * dt) / V + T.C_TAIL_LOSS * U * t * t / V).sum((2, 3)) / (H * W)
    got = sums.cpu() / (H * W)
    e_c, e_r = (got - chan).abs(), (got.mean(1) - chan.mean(1)).abs()
    print(f"[score gpu] recon per sample {(B, NIN, H, W, mk)}: worst error / bound per channel {float((e_c / b_chan).max()):.3f}, "
          f"recon {float((e_r / b_chan.mean(1)).max()):.3f}")
    assert not (e_c > b_chan).any() and not (e_r > b_chan.mean(1)).any()
    # per patch: a permutation permutes the rows, a patch alone reproduces its row, bit for bit
    perm = torch.randperm(B, generator=gen).to(DEV)
    sums_p = recon_call(lib, g[0][perm].contiguous(), g[1][perm].contiguous(), None if mask is None else g[2][perm].contiguous(), g[3])
    assert torch.equal(bits(sums_p), bits(sums[perm]))
    b = B - 1
    one = recon_call(lib, g[0][b:b + 1].contiguous(), g[1][b:b + 1].contiguous(), None if mask is None else g[2][b:b + 1].contiguous(), g[3])
    assert torch.equal(bits(one), bits(sums[b:b + 1]))


# ============================================================================================ dm_score_finalize
def test_score_finalize_arithmetic(lib):
    from dynamorph_amd import ops
    gen = torch.Generator().manual_seed(3)
    B, NIN, chw = 5, 3, 3 * 50 * 34
    sums = (torch.rand(B, NIN, generator=gen, dtype=torch.float64) * 1e4).to(DEV)
    vqs = torch.rand(B, 3, generator=gen).to(DEV)
    out = ops.score_finalize(sums, vqs, 0.7, 1.3, chw).cpu()
    s = sums.cpu()
    recon = (s.sum(1) / chw).float()
    assert torch.equal(out[:, 0], recon) and torch.equal(out[:, 4:], (s / (chw // NIN)).float())
    assert torch.equal(out[:, 1], vqs.cpu()[:, 0]) and torch.equal(out[:, 3], vqs.cpu()[:, 1])
    want = 0.7 * recon.double() + 1.3 * vqs.cpu()[:, 0].double()
    assert ((out[:, 2].double() - want).abs() <= 2.0 ** -23 * want.abs()).all()
