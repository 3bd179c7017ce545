"""GPU: the kernels, the modules and FusedTrainer away from the reference's default scalars.

Every other numerical test runs commitment_cost 0.25, unit loss weights and (w_a, w_t, w_n, margin) = (1.1, 0.1, -0.5, 0.5).
Here each kernel is held against a plain float64 expression of the same operation -- never against another HIP kernel --
over grids of those scalars, and the models against g12_hparams.npz, captured from the reference
(tests/golden/make_golden_hparams.py): VQ_VAE_z32 at the example configuration (config_example.yml:156-167, weight_matching
100), VQ_VAE / VQ_VAE_z16 with every loss weight away from 1, the quantiser at three commitment costs.
"""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from conftest import codes_gate, grad_gate, loss_gate, oracle_truth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from hparams import (A_KW, B_KW, B_Z16_KW, C_CCS, TM_IDS, TM_PARAMS, check_initial_state, example_batch,  # noqa: E402
                     example_relations, oracle_model, sample, stat, tm_reference, unpack_mask)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

Z32_BN_FED_BIASES = ("enc.0.bias", "enc.3.bias", "dec.1.bias") + tuple(
    f"{blk}.layers.{i}.{j}.bias" for blk in ("enc.5", "dec.0") for i in (0, 1) for j in (1, 4))
BN_FED_BIASES = ("enc.1.bias", "enc.4.bias", "enc.7.bias", "enc.10.bias",
                 "enc.12.layers.0.1.bias", "enc.12.layers.0.4.bias", "enc.12.layers.1.1.bias", "enc.12.layers.1.4.bias")


@pytest.fixture(scope="module")
def ops():
    from dynamorph_amd import ops as o
    return o


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def close(a, b, rtol, atol, what=""):
    a, b = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max():.3e} (ref max {b.abs().max():.3e})"


# ================================================================================ quantiser backward
# the three size classes of dm_vq_backward(_slabs): K <= 64 (the ordered one-hot product), 64 < K <= 4096 at D = 16, and
# the example quantiser K = 512 at D = 64 -- (B, K, D, H)
VQ_CLASSES = [(9, 64, 16, 16), (4, 1000, 16, 32), (3, 512, 64, 32)]
VQ_CCS = (0.0, 0.1, 1.0, 2.5)
VQ_GLOSS = (1.0, 0.7, 1.3)


@pytest.mark.parametrize("B,K,D,H", VQ_CLASSES, ids=["K64", "K1000", "K512xD64"])
@pytest.mark.parametrize("g_loss", VQ_GLOSS)
def test_vq_backward_commitment_cost_sweep(ops, B, K, D, H, g_loss):
    """dz = g_out + g_loss 2 cc (z - q) / N and dw = g_loss 2 (q - z) / N summed per code (vq_vae.py:71-72, the codebook's
    gradient carries no commitment cost) in float64, through the atomic and the slab form, at cc in {0, 0.1, 1, 2.5}.  The
    slab form's codebook gradient is bit-equal across cc; at cc = 0, dz is g_out to the bit."""
    z, cb, g = rnd(B, D, H, H, seed=K + D), rnd(K, D, seed=K + D + 1), rnd(B, D, H, H, seed=K + D + 2)
    zd, cbd, gd = z.to(DEV), cb.to(DEV), g.to(DEV)
    idx, _, _, _ = ops.vq_forward(zd, cbd, want_out=False)
    q = cb[idx.cpu()].permute(0, 3, 1, 2).double()
    N = z.numel()
    gl = torch.tensor([g_loss], device=DEV)
    dw_ref = torch.zeros(K, D, dtype=torch.float64).index_add_(
        0, idx.cpu().reshape(-1), (g_loss * 2 * (q - z.double()) / N).permute(0, 2, 3, 1).reshape(-1, D))
    tol_w = 1e-6 * float(dw_ref.abs().max())
    dw_first = None
    for cc in VQ_CCS:
        dz_ref = g.double() + g_loss * 2 * cc * (z.double() - q) / N
        dz_s, slabs = ops.vq_backward_slabs(zd, cbd, idx, gd, gl, cc)
        dw_s = ops.reduce_slabs(slabs, torch.empty_like(cbd))
        dz_a, dw_a = ops.vq_backward(zd, cbd, idx, gd, gl, cc, dw=torch.zeros(K, D, device=DEV))
        for name, dz in (("slabs", dz_s), ("atomic", dz_a)):
            close(dz, dz_ref, 1e-6, 1e-9, f"dz ({name}, cc {cc})")
            if cc == 0.0:
                assert torch.equal(dz, gd), name
        close(dw_s, dw_ref, 1e-5, tol_w, f"dw (slabs, cc {cc})")
        close(dw_a, dw_ref, 1e-5, tol_w, f"dw (atomic, cc {cc})")
        if dw_first is None:
            dw_first = dw_s
        else:
            assert torch.equal(dw_s, dw_first), f"the codebook gradient moved with the commitment cost ({cc})"


# ================================================================================ scalar launches
SCALAR_SETS = [(0.4, 0.7, 1.3, 3.0), (0.25, 1.0, 1.0, 100.0), (0.0, 0.0, 1.0, 0.0), (1.0, 2.0, 0.0, 0.005)]


@pytest.mark.parametrize("cc,wr,wc,wm", SCALAR_SETS)
def test_scalar_launches_weights_and_commitment_cost(ops, cc, wr, wc, wm):
    """vq_finalize, vq_loss_finalize, vq_loss_finalize_tm and loss_finalize: (recon, commitment, total, perplexity[, tm])
    with commitment = (1 + cc) mse, total = wr recon + wc commitment [+ wm tm], against float64 arithmetic on the same slabs
    and code counts."""
    B, D, K, H = 4, 16, 64, 16
    z, cb = rnd(B, D, H, H, seed=5).to(DEV), rnd(K, D, seed=6).to(DEV)
    P = B * H * H
    idx, _, sse, hist = ops.vq_forward(z, cb)
    _, _, sse2, ws = ops.vq_forward(z, cb, want_hist=False)
    assert torch.equal(sse, sse2)
    ls = torch.rand(8, dtype=torch.float64, generator=torch.Generator().manual_seed(7)).to(DEV) * 50
    tms = torch.rand(6, 1, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(8)).to(DEV)
    count = 3000
    mse = float(sse.double().sum()) / (P * D)
    commit = mse + cc * mse
    recon = float(ls.sum()) / count
    tml = float(tms[:, 0, 0].sum())
    p = torch.bincount(idx.cpu().reshape(-1), minlength=K).double() / P
    perp = float(torch.exp(-(p * torch.log(p + 1e-10)).sum()))
    total = wr * recon + wc * commit
    rel = 1e-6

    def near(got, want, what):
        assert abs(float(got) - want) <= rel * max(abs(want), 1e-6), (what, float(got), want)

    v3 = ops.vq_finalize(sse, hist, P, D, cc)
    near(v3[0], commit, "vq_finalize commitment")
    near(v3[1], perp, "vq_finalize perplexity")
    near(v3[2], mse, "vq_finalize mse")
    four = ops.vq_loss_finalize(sse, ws, K, D, P, cc, ls, count, wr, wc)
    five = ops.vq_loss_finalize_tm(sse, ws, K, D, P, cc, ls, count, wr, wc, tms, wm)
    lf = ops.loss_finalize(ls, count, v3, wr, wc)
    for name, out in (("vq_loss_finalize", four), ("vq_loss_finalize_tm", five), ("loss_finalize", lf)):
        near(out[0], recon, name + " recon")
        near(out[1], commit, name + " commitment")
        near(out[3], perp, name + " perplexity")
    near(four[2], total, "vq_loss_finalize total")
    near(lf[2], total, "loss_finalize total")
    near(five[4], tml, "vq_loss_finalize_tm term")
    near(five[2], total + wm * tml, "vq_loss_finalize_tm total")


# ================================================================================ time matching
TM_SHAPES = [(6, 4096, 0.7), (70, 1024, 0.7), (200, 4096, 2.0), (513, 256, 0.7)]


def _trajectory_batch(B, n, spread, seed):
    """Latents and a relation block as reorder_with_trajectories lays them out (frames of a trajectory next to each other:
    adjacent 2, others 1), related frames 40 % of the spread apart, plus relation values 0.5 and 3 and a one-way entry
    (they keep themselves as weight, vae.py:327-330)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, n, generator=g) * spread + 0.05
    tm = torch.zeros(B, B)
    if B <= 8:
        tm = torch.randint(0, 3, (B, B), generator=g).float()
    else:
        for t0 in range(0, B - 7, 11):
            for a in range(8):
                z[t0 + a] = z[t0] + 0.4 * spread * torch.randn(n, generator=g)
                for b in range(8):
                    if a != b:
                        tm[t0 + a, t0 + b] = 2.0 if abs(a - b) == 1 else 1.0
    tm[0, 1], tm[1, 0], tm[2, 1] = 0.5, 3.0, 3.0
    tm[B - 1, 0] = 1.0
    return z, tm


def _hinge_unsure(z, tm, w_n, margin, tol=1e-4):
    """Unrelated pairs whose hinge argument lies within fp32 reach of zero: the kernel may decide them the other way."""
    zd = z.double()
    sim = (zd.reshape(1, *zd.shape) - zd.reshape(zd.shape[0], 1, -1)).pow(2).mean(2)
    off = ~torch.eye(tm.shape[0], dtype=torch.bool)                 # (the diagonal's sim is exactly 0 on both sides)
    return off & (tm == 0) & ((sim * w_n + margin).abs() <= tol * (sim.abs() * abs(w_n) + abs(margin) + 1e-30))


def _check_S(S, gsim, unsure, what):
    """S (2, B, B): far + near part = d loss / d sim + its transpose."""
    want = (gsim + gsim.T)
    got = (S[0] + S[1]).cpu().double()
    keep = ~(unsure | unsure.T)
    err = ((got - want).abs() * keep).max().item()
    assert err <= 1e-6 * float(want.abs().max()) + 1e-12, (what, err, float(want.abs().max()))


@pytest.mark.parametrize("params", TM_PARAMS, ids=TM_IDS)
@pytest.mark.parametrize("B,n,spread", TM_SHAPES, ids=[f"{b}x{n}" for b, n, _ in TM_SHAPES])
def test_time_matching_weight_grid(ops, params, B, n, spread):
    """Mode 1 (vae.py:327-336) at six (w_a, w_t, w_n, margin) sets: loss, S = d loss / d sim (+ transpose) and dz against the
    reference's expression in float64, for the dense form and the stateful one (far-block map); the map covers every
    nonzero block of S's far part; the stateful gradient product equals the stateless one to the bit."""
    w_a, w_t, w_n, margin = params
    z, tm = _trajectory_batch(B, n, spread, seed=B + n)
    ref, gz, gsim = tm_reference(z, tm, 1, *params)
    unsure = _hinge_unsure(z, tm, w_n, margin)
    assert int(unsure.sum()) <= max(2, B * B // 1000)
    zd, tmd = z.to(DEV), tm.to(DEV)
    gl = torch.full((1,), 0.75, device=DEV)
    for form in ("dense", "stateful"):
        loss, S = ops.time_matching_forward(zd, tmd, 1, *params, allow_sparse=(form == "stateful"))
        assert abs(float(loss) - ref) <= 1e-5 * max(1.0, abs(ref)), (form, float(loss), ref)
        _check_S(S, gsim, unsure, form)
        dz = ops.time_matching_backward(zd, S, gl, 100.0).cpu().double()
        want = gz * 75.0
        assert (dz - want).abs().max() <= 2e-5 * want.abs().max() + 1e-9, (form, float((dz - want).abs().max()))
        if form == "stateful":
            nchunks, npanels = (B + 31) // 32, (B + 63) // 64
            fmap = S._dm_tm_state[4:].cpu().numpy().reshape(npanels, nchunks)
            far = S[0].cpu()
            for pnl in range(npanels):
                for c in range(nchunks):
                    if bool((far[64 * pnl:64 * pnl + 64, 32 * c:32 * c + 32] != 0).any()):
                        assert fmap[pnl, c] != 0, (pnl, c)
            if w_n > 0:
                assert int((fmap != 0).sum()) == npanels * nchunks          # every hinge live: the map is dense
            assert torch.equal(ops.time_matching_backward(zd, S, gl, 100.0), ops.time_matching_backward(zd, S.clone(), gl, 100.0))


@pytest.mark.parametrize("params", TM_PARAMS, ids=TM_IDS)
@pytest.mark.parametrize("B,n", [(70, 1024), (200, 4096)])
def test_time_matching_rows_weight_grid(ops, params, B, n):
    """The row-range pair (dm_time_matching_forward_rows / _backward_rows) against float64 directly: each range's share of
    the loss (sum over its rows i and all j of v_ij), its rows of S and of the whole term's dz."""
    w_a, w_t, w_n, margin = params
    z, tm = _trajectory_batch(B, n, 2.0 if B == 200 else 0.7, seed=3 * B + n)
    ref, gz, gsim = tm_reference(z, tm, 1, *params)
    unsure = _hinge_unsure(z, tm, w_n, margin)
    want_S = gsim + gsim.T
    zd, tmd = z.to(DEV), tm.to(DEV)
    partition = [(0, B // 3), (B // 3, 1), (B // 3 + 1, B - B // 3 - 1)]
    total = 0.0
    for r0, R in partition + [(0, B), (B - 1, 1)]:
        part, S = ops.time_matching_forward_rows(zd, tmd, r0, R, 1, *params)
        share, _, _ = tm_reference(z, tm, 1, *params, rows=(r0, R))
        assert abs(float(part) - share) <= 1e-5 * max(1.0, abs(ref)), (r0, R, float(part), share)
        if (r0, R) in partition:
            total += float(part)
        got = (S[0] + S[1]).cpu().double()
        keep = ~(unsure | unsure.T)[r0:r0 + R]
        err = ((got - want_S[r0:r0 + R]).abs() * keep).max().item()
        assert err <= 1e-6 * float(want_S.abs().max()) + 1e-12, (r0, R, err)
        dz = ops.time_matching_backward_rows(zd, S, None, 3.0).cpu().double()
        want = gz[r0:r0 + R] * 3.0
        assert (dz - want).abs().max() <= 2e-5 * float(gz.abs().max()) * 3.0 + 1e-9, (r0, R)
    assert abs(total - ref) <= 1e-5 * max(1.0, abs(ref))


@pytest.mark.parametrize("w_a,w_t,w_n", [(1.0, 0.5, -0.5), (1.1, 0.1, -1.3)])
@pytest.mark.parametrize("B,n", [(6, 4096), (70, 1024)])
def test_time_matching_hinge_boundary(ops, w_a, w_t, w_n, B, n):
    """margin 0 and exact duplicate latents marked unrelated: sim is exactly 0 (taken from differences), the hinge argument
    w_n sim + margin exactly 0, and torch.clamp's gradient passes at equality (vae.py:333-335).  dz cannot see this (the
    pair's z_i - z_j is 0), so S is compared on those pairs and on the diagonal, in both orientations, with float64."""
    g = torch.Generator().manual_seed(B)
    z = torch.randn(B, n, generator=g) * 0.7
    z[1] = z[0]
    z[4] = z[3]
    tm = torch.zeros(B, B)
    tm[2, 3] = tm[3, 2] = 2.0
    tm[0, 2] = 1.0
    params = (w_a, w_t, w_n, 0.0)
    ref, gz, gsim = tm_reference(z, tm, 1, *params)
    want = gsim + gsim.T
    pairs = [(0, 1), (1, 0), (3, 4), (4, 3)] + [(i, i) for i in range(B)]
    for i, j in pairs:
        assert float(want[i, j]) == pytest.approx(2 * w_n / B ** 2, rel=1e-12), (i, j)    # live at v == 0
    zd, tmd = z.to(DEV), tm.to(DEV)
    for form in ("dense", "stateful"):
        loss, S = ops.time_matching_forward(zd, tmd, 1, *params, allow_sparse=(form == "stateful"))
        assert abs(float(loss) - ref) <= 1e-5 * max(1.0, abs(ref)), (form, float(loss), ref)
        got = (S[0] + S[1]).cpu().double()
        for i, j in pairs:
            assert float(got[i, j]) == pytest.approx(float(want[i, j]), rel=1e-6), (form, i, j, float(got[i, j]))
        _check_S(S, gsim, torch.zeros(B, B, dtype=torch.bool), form)
        dz = ops.time_matching_backward(zd, S, None, 1.0).cpu().double()
        assert (dz - gz).abs().max() <= 2e-5 * gz.abs().max() + 1e-12, form
    _, Sr = ops.time_matching_forward_rows(zd, tmd, 0, 2, 1, *params)
    got = (Sr[0] + Sr[1]).cpu().double()
    for i, j in ((0, 1), (1, 0), (0, 0), (1, 1)):
        assert float(got[i, j]) == pytest.approx(float(want[i, j]), rel=1e-6), ("rows", i, j)


@pytest.mark.parametrize("B,n", [(6, 4096), (70, 1024), (129, 64)])
def test_time_matching_sum_form_non_integer_relations(ops, B, n):
    """Mode 0 (vq_vae.py:331, sum(sim * tm)) with non-integer relation values and one-way entries, at a gradient scale of
    100 (weight_matching of the example configuration), sparse and dense, against float64."""
    g = torch.Generator().manual_seed(B + 1)
    z = torch.randn(B, n, generator=g) * 0.6
    tm = (torch.rand(B, B, generator=g) * 2.5) * (torch.rand(B, B, generator=g) < 0.05)
    tm[0, 1], tm[1, 0], tm[2, 0] = 0.5, 0.0, 1.75
    tm.fill_diagonal_(0.0)
    ref, gz, gsim = tm_reference(z, tm, 0)
    zd, tmd = z.to(DEV), tm.to(DEV)
    for allow_sparse in (True, False):
        loss, S = ops.time_matching_forward(zd, tmd, 0, allow_sparse=allow_sparse)
        assert abs(float(loss) - ref) <= 1e-5 * max(1.0, abs(ref)), (allow_sparse, float(loss), ref)
        _check_S(S, gsim, torch.zeros(B, B, dtype=torch.bool), f"sparse {allow_sparse}")
        dz = ops.time_matching_backward(zd, S, None, 100.0).cpu().double()
        want = gz * 100.0
        assert (dz - want).abs().max() <= 2e-5 * want.abs().max() + 1e-9, allow_sparse


@pytest.mark.parametrize("params", TM_PARAMS + [None], ids=TM_IDS + ["sum_form"])
def test_time_matching_autograd_fallback_weight_grid(params):
    """vq_vae.time_matching_loss at a latent length the MFMA kernels do not tile (n % 32 != 0): distances from
    dm_pair_msd, weights / hinge / reduction in torch -- loss and gradient against float64."""
    from dynamorph_amd import ops as o
    from dynamorph_amd.vq_vae import time_matching_loss
    B, n = 9, 100
    assert not o.time_matching_supported(B, n)
    z, tm = _trajectory_batch(B, n, 0.7, seed=99)
    mode = 0 if params is None else 1
    ref, gz, _ = tm_reference(z, tm, mode, *(params or ()))
    za = z.to(DEV).requires_grad_(True)
    loss = time_matching_loss(za, tm.to(DEV), mode == 1, *(params or ()))
    loss.backward()
    assert abs(float(loss) - ref) <= 1e-5 * max(1.0, abs(ref)), (float(loss), ref)
    assert (za.grad.cpu().double() - gz).abs().max() <= 2e-5 * gz.abs().max() + 1e-12


# ================================================================================ models against g12_hparams.npz
def _models(g, cls, kw, part, name=None):
    """(the fp32 oracle, the HIP model) in the fixture's initial state: the oracle's seeded construction reproduces the
    reference's initialisation, held against the statistics the maker stored."""
    ref = oracle_model(part, name)
    prefix = "A/sd_stat/" if part == "A" else f"B/{name}/sd_stat/"
    check_initial_state(ref, g, prefix)
    m = cls(**kw)
    m.load_state_dict(ref.state_dict())
    return ref, m.to(DEV)


def _codes(m, ref, x):
    """The HIP path's codes against the reference's (conftest.codes_gate); returns the HIP codes where they differ."""
    with torch.no_grad():
        probe, mp = copy.deepcopy(ref), copy.deepcopy(m)
        z_r = probe.enc(x)
        idx_r = probe.vq.encode_inputs(z_r)
        idx = mp.vq.encode_inputs(mp.enc(x.to(DEV))).cpu()
    codes_gate(idx != idx_r, z_r, probe.vq.w.weight.detach())
    return idx if bool((idx != idx_r).any()) else None


def _run(m, path, x, mask, tm, lr=1e-4):
    """(losses of the first step {name: float}, losses of the second step after one Adam step, the model with p.grad set to
    the first step's gradients)."""
    from dynamorph_amd.train import FusedTrainer
    keys = ("recon_loss", "commitment_loss", "total_loss", "perplexity", "time_matching_loss")
    if path == "autograd":
        _, ld = m(x, time_matching_mat=tm, batch_mask=mask)
        ld["total_loss"].backward()
        first = {k: float(ld[k]) for k in keys}
        grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        opt = torch.optim.Adam(m.parameters(), lr=lr, betas=(.9, .999))
        opt.step()
        m.zero_grad()
        _, ld2 = m(x, time_matching_mat=tm, batch_mask=mask)
        second = {k: float(ld2[k]) for k in keys}
        for k, p in m.named_parameters():
            p.grad = grads.get(k)
        return first, second
    tr = FusedTrainer(m, lr=lr, use_graph=(path == "fused_graph"))
    first = dict(zip(keys, tr.step(x, mask, tm).tolist()))
    tr.expose_grads()
    snap = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    second = dict(zip(keys, tr.step(x, mask, tm).tolist()))
    for k, p in m.named_parameters():
        p.grad = snap.get(k)
    return first, second


def _fixture_gates(m, g, prefix, first, fed, what):
    for k in ("recon_loss", "commitment_loss", "time_matching_loss", "total_loss"):
        loss_gate(first[k], g[prefix + "loss/" + k], f"{what} {k}")
    assert abs(first["perplexity"] - float(g[prefix + "loss/perplexity"])) <= 1e-3 * float(g[prefix + "loss/perplexity"])
    n = 0
    for k, p in m.named_parameters():
        if not p.requires_grad:
            continue
        if k in fed:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k          # never written: exactly zero
            continue
        # the fixture keeps a strided sample of every gradient and statistics of the whole tensor
        st = g[prefix + "grad_stat/" + k]
        scale = max(float(st[3]), 1e-6)
        err = float(np.abs(sample(p.grad) - g[prefix + "grad/" + k]).max())
        assert err <= 4e-3 * scale + 1e-8, (what, k, err, scale)
        got = stat(p.grad)
        assert abs(got[1] - st[1]) <= 4e-3 * st[1] + 1e-8, (what, k, "sum |.|", got[1], st[1])
        assert abs(got[3] - st[3]) <= 4e-3 * scale + 1e-8, (what, k, "max |.|", got[3], st[3])
        n += 1
    assert n >= 25


PATHS = ["autograd", "fused", "fused_graph"]


@pytest.mark.parametrize("path", PATHS)
def test_example_configuration_against_reference(golden, path):
    """Part A: VQ_VAE_z32 at config_example.yml's scalars (64 / 64 / 512, weight_matching 100, margin 1, w_a 1, w_t 0.5,
    w_n -0.5) with vq_vae_supp.py's channel variances, both sides of the hinge occupied.  Losses (loss_gate), every
    gradient against the reference's and against the float64 oracle (grad_gate), the losses of the second step after one
    Adam step.  Sensitivity: on the encoder tensors the HIP error is at most 1 % of what the pairwise term contributes
    (|grad - grad_wm0|), so a mis-scaled term fails.  (The codebook's gradient is the q-latent loss alone: the term acts
    on z_after, whose gradient reaches z through the straight-through value, so there grad == grad_wm0.)"""
    import dynamorph_amd
    g = golden("g12_hparams.npz")
    assert int(g["A/hinge_live"]) > 0 and int(g["A/hinge_dead"]) > 0
    x = example_batch(golden("g2_input.npz")["x"])
    assert np.array_equal(stat(x), g["A/x_stat"])
    tm, mask = example_relations(), unpack_mask(g["A/mask_bits"], (6, 1, 128, 128))
    ref, m = _models(g, dynamorph_amd.VQ_VAE_z32, A_KW, "A")
    flips = _codes(m, ref, x)
    if flips is not None:
        ref.vq.force_idx = flips.clone()
    first, second = _run(m, path, x.to(DEV), mask.to(DEV), tm.to(DEV))
    _fixture_gates(m, g, "A/", first, Z32_BN_FED_BIASES, f"example z32 {path}")
    for k in ("recon_loss", "commitment_loss", "time_matching_loss", "total_loss"):
        loss_gate(second[k], g["A/step2/" + k], f"example z32 {path} step 2 {k}", tol=5e-5)
    assert np.array_equal(g["A/grad/vq.w.weight"], g["A/grad_wm0/vq.w.weight"])
    assert np.array_equal(g["A/grad_stat/vq.w.weight"], g["A/grad_wm0_stat/vq.w.weight"])
    for k in ("enc.0.weight", "enc.3.weight", "enc.5.layers.0.1.weight"):
        term = float(np.abs(g["A/grad/" + k] - g["A/grad_wm0/" + k]).max())
        err = float(np.abs(sample(dict(m.named_parameters())[k].grad) - g["A/grad/" + k]).max())
        print(f"{path} {k}: hip error {err:.3e}, pairwise term's share {term:.3e}")
        assert term > 0.02 * float(g["A/grad_stat/" + k][3]), k
        assert err <= 0.01 * term, (k, err, term)
    _, g32, g64 = oracle_truth(ref, x, time_matching_mat=tm, batch_mask=mask)
    grad_gate(m, g32, g64, skip=Z32_BN_FED_BIASES, floor=4e-3, what=f"example z32 {path}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["vqvae", "z16"])
def test_weighted_losses_against_reference(golden, name, path):
    """Part B: VQ_VAE (sum form) and VQ_VAE_z16 (weighted hinge, w_a 0.8, w_t 0.3, w_n -0.2, margin 0.7) with
    commitment_cost 0.4, weight_recon 0.7, weight_commitment 1.3, channel_var [0.5, 1.5], weight_matching 3: the weights are
    gradient seeds on FusedTrainer's path (w_recon / w_commit) and autograd's factors on the module path."""
    import dynamorph_amd
    g = golden("g12_hparams.npz")
    x = torch.from_numpy(golden("g2_input.npz")["x"])
    tm, mask = torch.from_numpy(g[f"B/{name}/tm"]), unpack_mask(g["B/mask_bits"], (4, 1, 128, 128))
    kw = dict(B_KW, **B_Z16_KW) if name == "z16" else dict(B_KW)
    cls = dynamorph_amd.VQ_VAE_z16 if name == "z16" else dynamorph_amd.VQ_VAE
    ref, m = _models(g, cls, kw, "B", name)
    flips = _codes(m, ref, x)
    if flips is not None:
        ref.vq.force_idx = flips.clone()
    first, _ = _run(m, path, x.to(DEV), mask.to(DEV), tm.to(DEV))
    _fixture_gates(m, g, f"B/{name}/", first, BN_FED_BIASES, f"{name} {path}")
    _, g32, g64 = oracle_truth(ref, x, time_matching_mat=tm, batch_mask=mask)
    grad_gate(m, g32, g64, skip=BN_FED_BIASES, floor=4e-3, what=f"{name} {path}")


@pytest.mark.parametrize("cc", C_CCS)
def test_vector_quantizer_commitment_cost_against_reference(golden, cc):
    """Part C: dynamorph_amd.VectorQuantizer forward and backward at commitment_cost 0, 0.1, 1 against the reference's."""
    import dynamorph_amd
    g = golden("g12_hparams.npz")
    vq = dynamorph_amd.VectorQuantizer(16, 64, commitment_cost=cc).to(DEV)
    with torch.no_grad():
        vq.w.weight.copy_(torch.from_numpy(g["C/w"]))
    z = torch.from_numpy(g["C/z"]).to(DEV).requires_grad_(True)
    out, loss, perp = vq(z)
    ((out * torch.from_numpy(g["C/g_out"]).to(DEV)).sum() + float(g["C/g_loss"]) * loss).backward()
    p = f"C/cc{cc:g}/"
    assert torch.equal(out.detach().cpu(), torch.from_numpy(g[p + "out"]))
    loss_gate(loss, g[p + "loss"], f"quantiser cc {cc:g} loss")
    assert abs(float(perp) - float(g[p + "perplexity"])) <= 1e-5 * float(g[p + "perplexity"])
    close(z.grad, torch.from_numpy(g[p + "dz"]), 1e-5, 1e-7, f"dz cc {cc:g}")
    close(vq.w.weight.grad, torch.from_numpy(g[p + "dw"]), 1e-5, 1e-6 * float(np.abs(g[p + "dw"]).max()), f"dw cc {cc:g}")
    if cc == 0.0:
        assert torch.equal(z.grad.cpu(), torch.from_numpy(g["C/g_out"]))
