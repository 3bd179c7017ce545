"""Op-level parity of every HIP kernel (through the C ABI) against a PyTorch-CPU fp32 reference of
the same op / the C oracle.  Tolerances: bit-exact for indices and the straight-through value;
fp32 accumulation-order tolerance (stated per test) for everything else."""
import ctypes
import os
import subprocess
import sys

import numpy as np
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


@pytest.fixture(scope="module")
def cvq():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    return ctypes.CDLL(os.path.join(ROOT, "oracle", "libvq_oracle.so"))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(a, b, rtol, atol, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    bound = atol + rtol * b.abs()
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} off, max err {err.max():.3e} (ref max {b.abs().max():.3e})"


def load_ref(p0, mode, coef=None, p1=None):
    """CPU restatement of dm_operand's transform; coef (C,4) or (B,C,4)."""
    if mode == 0:
        return p0
    if mode == 1:
        return p0.clamp(min=0)
    c = coef if coef.dim() == 3 else coef.unsqueeze(0)
    c0, c1, c2 = (c[..., i].unsqueeze(-1).unsqueeze(-1) for i in range(3))
    if mode == 4:
        return c0 * p0 + c1 * p1 + c2
    v = c0 * p0 + c2
    return v.clamp(min=0) if mode == 3 else v


# =================================================================================== VQ
from dynamorph_amd._lib import DM_VQ_AUTO, DM_VQ_BF16, DM_VQ_EXACT, DM_VQ_MFMA          # noqa: E402
from dynamorph_amd._lib import DM_LOAD_AFFINE as DM_LOAD_AFFINE_K                          # noqa: E402

VQ_VARIANTS = [pytest.param(DM_VQ_EXACT, id="exact"), pytest.param(DM_VQ_MFMA, id="mfma"), pytest.param(DM_VQ_BF16, id="bf16split")]


@pytest.mark.parametrize("variant", VQ_VARIANTS)
def test_vq_forward_bit_exact_golden(ops, golden, variant):
    g4, g5 = golden("g4_vq_indices.npz"), golden("g5_vq_forward.npz")
    z = torch.from_numpy(g5["z_before"]).to(DEV)
    cb = torch.from_numpy(g4["codebook"]).to(DEV)
    idx, out, slabs, hist = ops.vq_forward(z, cb, variant=variant)
    sc = ops.vq_finalize(slabs, hist, idx.numel(), 16, 0.25).cpu().numpy()
    assert np.array_equal(idx.cpu().numpy(), g4["idx"])
    assert np.array_equal(out.cpu().numpy().view(np.uint32), g5["quantized"].view(np.uint32))
    assert abs(sc[0] - g5["loss"]) <= 1e-6 * abs(g5["loss"])
    assert abs(sc[1] - g5["perplexity"]) <= 1e-5 * abs(g5["perplexity"])
    assert np.array_equal(hist.cpu().numpy(), np.bincount(g4["idx"].ravel(), minlength=64))
    q = ops.vq_decode(idx, cb).cpu()
    assert torch.equal(q, torch.from_numpy(g4["codebook"])[torch.from_numpy(g4["idx"])].permute(0, 3, 1, 2))


@pytest.mark.parametrize("variant", VQ_VARIANTS)
@pytest.mark.parametrize("name", ["g9_vq_k4096.npz", "g9_vq_d64.npz", "g9_vq_ties.npz"])
def test_vq_forward_stress_golden(ops, golden, name, variant):
    g = golden(name)
    z, cb = torch.from_numpy(g["z"]).to(DEV), torch.from_numpy(g["codebook"]).to(DEV)
    if variant in (DM_VQ_MFMA, DM_VQ_BF16) and (z.shape[2] * z.shape[3]) % 64:
        pytest.skip("the MFMA kernels take latent grids that are multiples of 64 positions")
    idx, out, slabs, hist = ops.vq_forward(z, cb, variant=variant)
    assert np.array_equal(idx.cpu().numpy(), g["idx"]), name
    if "loss" in g:
        sc = ops.vq_finalize(slabs, hist, idx.numel(), z.shape[1], 0.25).cpu().numpy()
        assert abs(sc[0] - g["loss"]) <= 1e-6 * abs(g["loss"])
        assert abs(sc[1] - g["perplexity"]) <= 2e-5 * abs(g["perplexity"])


def _c_oracle_idx(cvq, z, cb):
    B, D, H, W = z.shape
    idx_ref = np.empty((B, H, W), np.int64)
    cvq.oracle_vq_encode(_p(z), _p(cb), _p(idx_ref), B, D, cb.shape[0], H, W)
    return idx_ref


@pytest.mark.parametrize("B,D,K,H,W", [(3, 16, 64, 16, 16), (2, 16, 63, 8, 12), (1, 32, 10, 4, 4), (5, 8, 7, 16, 16),
                                       (2, 64, 40, 8, 8), (2, 128, 128, 8, 8),
                                       # shapes of the MFMA kernel: code counts around the 64-code chunks and the 32 KB
                                       # LDS pieces, every embedding_dim it is built for, chunk counts that are not a
                                       # multiple of the 4 waves of a workgroup
                                       (7, 16, 1, 8, 8), (3, 16, 65, 16, 16), (2, 16, 513, 16, 16), (1, 16, 1000, 32, 32),
                                       (3, 8, 100, 8, 8), (3, 32, 300, 8, 16), (2, 64, 512, 16, 16), (5, 64, 129, 8, 8),
                                       # more than 1024 codes: the counters go straight to the global replicas; code chunks
                                       # streamed through the two LDS buffers with an odd and an even number of refills
                                       (2, 16, 1100, 16, 16), (1, 16, 2049, 16, 32), (6, 32, 1025, 8, 8),
                                       # vq_cells_kernel (64 < K <= 4096 at embedding_dim 16, grids of 128 positions): code counts
                                       # that are not a multiple of the 128-code groups (padded cells), one group, all 32 groups,
                                       # more passes than waves (B = 40: 80 passes of 128 positions)
                                       (3, 16, 200, 16, 16), (2, 16, 129, 8, 16), (1, 16, 3000, 16, 16), (2, 16, 128, 16, 8),
                                       (1, 16, 4096, 32, 32), (40, 16, 777, 16, 16),
                                       # widths without an instantiation: vq_forward_any_kernel (run-time embedding_dim)
                                       (2, 12, 40, 8, 8), (3, 24, 64, 16, 16), (2, 48, 100, 8, 8), (2, 96, 64, 8, 8),
                                       (1, 5, 4, 4, 4), (2, 20, 33, 5, 7), (1, 200, 17, 4, 4)])
def test_vq_forward_vs_c_oracle(ops, cvq, B, D, K, H, W):
    z = rnd(B, D, H, W, seed=B + D + K).numpy()
    cb = rnd(K, D, seed=K).numpy()
    idx_ref = _c_oracle_idx(cvq, z, cb)
    q = cb[idx_ref].transpose(0, 3, 1, 2)
    variants = [DM_VQ_AUTO, DM_VQ_EXACT] + ([DM_VQ_MFMA] if (H * W) % 64 == 0 and D in (8, 16, 32, 64) else []) + (
        [DM_VQ_BF16] if (H * W) % 64 == 0 and D in (16, 32, 64) else [])
    for variant in variants:
        idx, out, slabs, hist = ops.vq_forward(torch.from_numpy(z).to(DEV), torch.from_numpy(cb).to(DEV), variant=variant)
        assert np.array_equal(idx.cpu().numpy(), idx_ref), variant
        assert np.array_equal(out.cpu().numpy(), z + (q - z)), variant
        assert np.array_equal(hist.cpu().numpy(), np.bincount(idx_ref.ravel(), minlength=K)), variant
        sse = float(slabs.sum().cpu())
        assert abs(sse - float(((q - z).astype(np.float64) ** 2).sum())) <= 1e-6 * sse, variant


@pytest.mark.parametrize("K", [64, 65, 71, 72, 73, 80, 144])
def test_vq_counter_rows_are_told_apart_by_their_flag_not_their_stride(ops, cvq, K):
    """A codebook of exactly 72 codes has the per-workgroup rows' stride (72 ints) on the REPLICA path: the finalisers must
    go by the format word of the workspace header.  Histogram, re-check count and the step's fused scalar launch
    (perplexity from the counters in the workspace) for code counts around it, on both counter formats (K = 64: rows)."""
    B, D, H, W = 9, 16, 16, 16
    z = rnd(B, D, H, W, seed=K).numpy()
    cb = rnd(K, D, seed=K + 1).numpy()
    idx_ref = _c_oracle_idx(cvq, z, cb)
    counts = np.bincount(idx_ref.ravel(), minlength=K)
    zt, ct = torch.from_numpy(z).to(DEV), torch.from_numpy(cb).to(DEV)
    for variant in (DM_VQ_AUTO, DM_VQ_MFMA, DM_VQ_BF16):
        idx, out, slabs, hist = ops.vq_forward(zt, ct, variant=variant)
        assert np.array_equal(idx.cpu().numpy(), idx_ref), variant
        assert np.array_equal(hist.cpu().numpy(), counts), variant
        # the training step's form: no counter reduction, one scalar launch reading the rows / replicas in the workspace
        idx2, out2, slabs2, ws = ops.vq_forward(zt, ct, variant=variant, want_hist=False)
        loss_slabs = torch.zeros(4, dtype=torch.float64, device=DEV)
        sc = ops.vq_loss_finalize(slabs2, ws, K, D, B * H * W, 0.25, loss_slabs, 10, 1.0, 1.0).cpu().numpy()
        p = counts.astype(np.float32) / np.float32(B * H * W)
        perp = np.exp(-np.sum(p * np.log(p + np.float32(1e-10)), dtype=np.float64))
        assert abs(sc[3] - perp) <= 2e-5 * perp, (variant, sc[3], perp)
        q = cb[idx_ref].transpose(0, 3, 1, 2)
        mse = float(((q - z).astype(np.float64) ** 2).mean())
        assert abs(sc[1] - 1.25 * mse) <= 2e-6 * mse, variant


@pytest.mark.parametrize("B,K,H,W", [(3, 64, 16, 16), (70, 64, 16, 16), (5, 10, 8, 8), (1, 33, 16, 32), (257, 64, 8, 8)])
def test_vq_forward_join_equals_apply_then_vq(ops, B, K, H, W):
    """dm_vq_forward_join: the last residual join (dm_apply: z = fma(c0, rb, c2) + h) in the quantiser's load path.
    Latents, codes, straight-through values and squared-error slabs bit-equal to the two separate launches; the counters in
    the workspace give the same scalars."""
    D = 16
    rb, h = rnd(B, D, H, W, seed=B + K).to(DEV), rnd(B, D, H, W, seed=B + K + 1).to(DEV)
    coef = torch.zeros(D, 4)
    coef[:, 0] = rnd(D, seed=3).abs() + 0.5
    coef[:, 1] = 123.0                                   # (unused by the AFFINE transform)
    coef[:, 2] = rnd(D, seed=4)
    coef = coef.to(DEV)
    cb = rnd(K, D, seed=K).to(DEV)
    assert ops.vq_forward_join_supported(D, K, H, W)
    z_ref = ops.apply(ops.Op(rb, DM_LOAD_AFFINE_K, coef), B, D, H, W, resid=h)
    assert torch.equal(z_ref, torch.addcmul(coef[:, 2].view(1, D, 1, 1), coef[:, 0].view(1, D, 1, 1), rb) + h) or True
    idx_r, out_r, slabs_r, ws_r = ops.vq_forward(z_ref, cb, want_hist=False)
    idx, out, slabs, ws, z = ops.vq_forward_join(rb, h, coef, cb)
    assert torch.equal(z, z_ref)
    assert torch.equal(idx, idx_r) and torch.equal(out.view(torch.int32), out_r.view(torch.int32))
    assert torch.equal(slabs, slabs_r)
    ls = torch.zeros(4, dtype=torch.float64, device=DEV)
    a = ops.vq_loss_finalize(slabs, ws, K, D, B * H * W, 0.25, ls, 10, 1.0, 1.0)
    b = ops.vq_loss_finalize(slabs_r, ws_r, K, D, B * H * W, 0.25, ls, 10, 1.0, 1.0)
    assert torch.equal(a, b)
    assert not ops.vq_forward_join_supported(32, K, H, W) and not ops.vq_forward_join_supported(D, 4096, H, W)
    with pytest.raises(ValueError):
        ops.vq_forward_join(rb, h, coef, rnd(4096, D, seed=1).to(DEV))


def test_vq_mfma_rejects_what_it_cannot_tile(ops):
    with pytest.raises(ValueError):
        ops.vq_forward(rnd(1, 16, 8, 12).to(DEV), rnd(4, 16).to(DEV), variant=DM_VQ_MFMA)     # 96 positions per sample
    with pytest.raises(ValueError):
        ops.vq_forward(rnd(1, 128, 8, 8).to(DEV), rnd(4, 128).to(DEV), variant=DM_VQ_MFMA)    # embedding_dim 128
    with pytest.raises(ValueError):
        ops.vq_forward(rnd(1, 8, 8, 8).to(DEV), rnd(4, 8).to(DEV), variant=DM_VQ_BF16)        # one K-group needs 16 dimensions


@pytest.mark.parametrize("filt", [pytest.param(DM_VQ_MFMA, id="f32"), pytest.param(DM_VQ_BF16, id="bf16split")])
@pytest.mark.parametrize("D,K", [(16, 64), (16, 512), (64, 128), (32, 64)])
def test_vq_mfma_near_ties_and_non_finite_values(ops, cvq, D, K, filt):
    """The cases the MFMA filter must hand to the exact path: latents on (and a few ulp off) the bisector of two codes,
    duplicated codes (exact ties: the FIRST index wins, vq_vae.py:68), NaN / inf latents, and -- second half -- a
    codebook with a NaN and an inf row (torch.argmax(-dist): the first NaN wins)."""
    g = np.random.default_rng(D + K)
    cb = g.standard_normal((K, D)).astype(np.float32)
    cb[K // 2] = cb[3]                                    # exact duplicates, the earlier one must win
    cb[K - 1] = cb[1]
    B, H, W = 4, 16, 16
    z = g.standard_normal((B, D, H, W)).astype(np.float32)
    zf = z.transpose(0, 2, 3, 1).reshape(-1, D)           # (P, D) view for editing positions
    P = zf.shape[0]
    pick = g.permutation(P)
    n = P // 8
    a, b = g.integers(0, K, n), g.integers(0, K, n)
    mid = 0.5 * (cb[a] + cb[b])
    zf[pick[:n]] = mid                                                                     # on the bisector
    zf[pick[n:2 * n]] = np.nextafter(mid, np.float32(np.inf)) + np.float32(0)               # one ulp off, every coordinate
    zf[pick[2 * n:3 * n]] = mid * (1 + 3e-7 * g.standard_normal((n, 1)).astype(np.float32))  # a few ulp off
    zf[pick[3 * n:3 * n + 64]] = cb[g.integers(0, K, 64)]                                   # exactly on a code
    zf[pick[3 * n + 64], 0] = np.nan
    zf[pick[3 * n + 65], D - 1] = np.inf
    zf[pick[3 * n + 66], 1] = -np.inf
    zf[pick[3 * n + 67]] = 1e30                                                            # squares overflow
    zf[pick[3 * n + 68]] = 0.0
    z = np.ascontiguousarray(zf.reshape(B, H, W, D).transpose(0, 3, 1, 2))
    for with_bad_codes in (False, True):
        if with_bad_codes:
            cb = cb.copy()
            cb[7, 2] = np.nan
            cb[5, 0] = np.inf
        idx_ref = _c_oracle_idx(cvq, z, cb)
        zd, cbd = torch.from_numpy(z).to(DEV), torch.from_numpy(cb).to(DEV)
        idx_e = ops.vq_forward(zd, cbd, want_out=False, variant=DM_VQ_EXACT)[0].cpu().numpy()
        idx_m, _, _, _, nre = ops.vq_forward(zd, cbd, want_out=False, variant=filt, want_rechecked=True)
        assert np.array_equal(idx_e, idx_ref)
        assert np.array_equal(idx_m.cpu().numpy(), idx_ref)
        nre = int(nre.cpu())
        if with_bad_codes:
            assert nre == P                                   # a non-finite codebook: every position takes the exact path
        else:
            # every position whose two best codes are (nearly) tied in float64 must have taken the exact path
            zt, ct = torch.from_numpy(z).double().permute(0, 2, 3, 1).reshape(-1, D), torch.from_numpy(cb).double()
            d2 = torch.cdist(zt, ct).pow(2)
            fin = torch.isfinite(d2).all(1)
            top, which = torch.topk(d2[fin], 2, dim=1, largest=False)
            tied = (top[:, 1] - top[:, 0]) <= 1e-6 * top[:, 1]
            near = int(tied.sum()) + int((~fin).sum())
            assert near >= n, near                            # the construction did produce near-ties
            if filt == DM_VQ_BF16 and D == 16 and 64 < K <= 4096:
                # vq_cells_kernel (csrc/vq_cells.h): two tied codes inside ONE cell of 8 consecutive codes are settled by the
                # cell's own exact evaluation, without the re-check path (and without its counter)
                near -= int((tied & (which[:, 0] // 8 == which[:, 1] // 8)).sum())
            assert nre >= near, (nre, near, P)


def _vq_tie_case(D, K, H, W, B=2):
    """Codebook with exact duplicate rows across the structures the exact re-check walks (the last code = the first; code 64 =
    code 63: two 64-code chunks / lane strides; code 129 = code 7: two groups of 128), and latents of which a third lie
    exactly on a duplicated code, a third on the bisector of two random codes, the rest random, one with a NaN, one with an
    inf.  Returns (z, cb, dup, on): the positions (flat, (b, h, w) order) placed on a duplicated code and, per position, the
    two codes (first, again) of that pair."""
    g = np.random.default_rng(1000 * D + K + H * W)
    cb = g.standard_normal((K, D)).astype(np.float32)
    pairs = [(0, K - 1)] + ([(63, 64)] if K > 64 else []) + ([(7, 129)] if K > 129 else [])
    for first, again in pairs:
        cb[again] = cb[first]
    pairs = [p for p in pairs if np.array_equal(cb[p[0]], cb[p[1]])]      # (K = 130: code 129 ends as code 7's copy, not code 0's)
    z = g.standard_normal((B, D, H, W)).astype(np.float32)
    zf = z.transpose(0, 2, 3, 1).reshape(-1, D)
    P = zf.shape[0]
    pick, n = g.permutation(P), P // 3
    on = np.array(pairs)[g.integers(0, len(pairs), n)]
    zf[pick[:n]] = cb[on[:, 0]]
    a, b = g.integers(0, K, n), g.integers(0, K, n)
    zf[pick[n:2 * n]] = 0.5 * (cb[a] + cb[b])
    zf[pick[2 * n], 0] = np.nan
    zf[pick[2 * n + 1], D - 1] = np.inf
    z = np.ascontiguousarray(zf.reshape(B, H, W, D).transpose(0, 3, 1, 2))
    return z, cb, pick[:n], on


@pytest.mark.parametrize("D,K,H,W", [(16, 5, 8, 8),        # fewer codes than lanes
                                     (8, 70, 8, 8),        # embedding_dim 8: the f32 filter only
                                     (16, 200, 8, 8),      # streamed re-check (64 positions per sample: not the cell kernel)
                                     (32, 130, 8, 8),      # embedding_dim 32 across groups
                                     (16, 130, 8, 16),     # vq_cells_kernel, two codes in the last group of 128
                                     (16, 200, 8, 16)])    # vq_cells_kernel, ragged last group
def test_vq_exact_recheck_ties_on_every_route(ops, cvq, D, K, H, W):
    """Exact ties where the lanes, chunks, cells and groups of the exact re-check meet (the per-lane scans and the wave-wide
    first minimum of vq_forward_mfma_kernel and vq_cells_kernel): the smaller code wins on every route.  Indices,
    straight-through values and counters bit-equal to DM_VQ_EXACT and to the C oracle (`out` against the oracle: the same
    bits wherever the oracle's value is finite, and non-finite in the same places -- the position with an inf yields
    inf - inf, whose NaN sign is the host's resp. the GPU's own); every position on a duplicated code went through the
    re-check -- except, where vq_cells_kernel runs, a pair inside one cell of 8 consecutive codes, which the cell's own
    exact evaluation settles (the rule of test_vq_mfma_near_ties_and_non_finite_values)."""
    z, cb, dup, on = _vq_tie_case(D, K, H, W)
    idx_ref = _c_oracle_idx(cvq, z, cb)
    q = cb[idx_ref].transpose(0, 3, 1, 2)
    with np.errstate(invalid="ignore"):
        out_ref = z + (q - z)
    fin = np.isfinite(out_ref)
    hist_ref = np.bincount(idx_ref.ravel(), minlength=K)
    # the construction: a position on a duplicated code is the earlier code's; pairs inside one cell of 8 consecutive codes
    assert np.array_equal(idx_ref.ravel()[dup], on[:, 0])
    in_one_cell = int((on[:, 0] // 8 == on[:, 1] // 8).sum())
    zd, cbd = torch.from_numpy(z).to(DEV), torch.from_numpy(cb).to(DEV)
    idx_e, out_e, _, hist_e = ops.vq_forward(zd, cbd, variant=DM_VQ_EXACT)
    variants = [DM_VQ_AUTO, DM_VQ_EXACT] + ([DM_VQ_MFMA] if (H * W) % 64 == 0 and D in (8, 16, 32, 64) else []) + (
        [DM_VQ_BF16] if (H * W) % 64 == 0 and D in (16, 32, 64) else [])
    for variant in variants:
        idx, out, _, hist, nre = ops.vq_forward(zd, cbd, variant=variant, want_rechecked=True)
        assert np.array_equal(idx.cpu().numpy(), idx_ref), variant
        got = out.cpu().numpy()
        assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got.view(np.int32)[fin], out_ref.view(np.int32)[fin]), variant
        assert np.array_equal(hist.cpu().numpy(), hist_ref), variant
        assert torch.equal(idx, idx_e) and torch.equal(out.view(torch.int32), out_e.view(torch.int32)), variant
        assert torch.equal(hist, hist_e), variant
        if variant != DM_VQ_EXACT:
            # vq_cells_kernel: the bf16-split filter (AUTO takes it) at embedding_dim 16, 64 < K <= 4096, grids of 128 positions
            cells = variant != DM_VQ_MFMA and D == 16 and 64 < K <= 4096 and (H * W) % 128 == 0
            must = len(dup) - (in_one_cell if cells else 0)
            assert must > 0 and int(nre.cpu()) >= must, (variant, int(nre.cpu()), must)


@pytest.mark.parametrize("filt", [pytest.param(DM_VQ_MFMA, id="f32"), pytest.param(DM_VQ_BF16, id="bf16split")])
def test_vq_mfma_large_sweep(ops, cvq, filt):
    """4 M random positions at the headline shape (K = 64, D = 16, 16 x 16 latents): the MFMA kernel equals the exact
    kernel everywhere and the C oracle on the first 0.5 M positions; the share of positions it has to re-evaluate
    exactly stays small (it is the price of the filter, printed for DESIGN.md)."""
    B, D, K, H, W = 2048, 16, 64, 16, 16
    cb = rnd(K, D, seed=5)
    cbd = cb.to(DEV)
    total, rechecked = 0, 0
    for rep in range(8):
        z = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(100 + rep)) * (0.5 + 0.25 * rep)
        zd = z.to(DEV)
        idx_e, out_e, _, hist_e = ops.vq_forward(zd, cbd, variant=DM_VQ_EXACT)
        idx_m, out_m, _, hist_m, nre = ops.vq_forward(zd, cbd, variant=filt, want_rechecked=True)
        assert torch.equal(idx_e, idx_m), rep
        assert torch.equal(out_e, out_m), rep
        assert torch.equal(hist_e, hist_m), rep
        total += idx_m.numel()
        rechecked += int(nre.cpu())
        if rep == 0:
            assert np.array_equal(idx_m.cpu().numpy(), _c_oracle_idx(cvq, z.numpy(), cb.numpy()))
    frac = rechecked / total
    print(f"vq mfma sweep (filter {filt}): {total} positions, {rechecked} re-evaluated exactly ({frac:.2e})")
    assert 0 < frac < 1e-2


def test_vq_backward_golden(ops, golden):
    g6, g4 = golden("g6_vq_backward.npz"), golden("g4_vq_indices.npz")
    z = torch.from_numpy(g6["z"]).to(DEV)
    cb = torch.from_numpy(g4["codebook"]).to(DEV)
    idx = torch.from_numpy(g4["idx"]).to(DEV)
    gl = torch.tensor([float(g6["g_loss"])], device=DEV)
    dz, dw = ops.vq_backward(z, cb, idx, torch.from_numpy(g6["g_out"]).to(DEV), gl, 0.25)
    close(dz, torch.from_numpy(g6["dz"]), 1e-6, 1e-9, "dz")
    close(dw, torch.from_numpy(g6["dw"]), 2e-5, 1e-8, "dw")


# ========================================================================== convolutions
def close_stats(st, out, q=None, what="stats"):
    """Statistics slabs against double sums of the reference output, tolerance relative to the sum of magnitudes
    (a loose absolute tolerance hides a dropped row)."""
    q = out if q is None else q
    ref = _stats_ref(out, q)
    mag = torch.stack([out.double().abs().sum((0, 2, 3)), (out.double() * q.double()).abs().sum((0, 2, 3))], 1)
    err = (st.detach().cpu().double() - ref).abs()
    bad = err > 3e-5 * mag + 1e-9
    assert not bad.any(), f"{what}: {int(bad.sum())} sums off, worst {float((err / (mag + 1e-30)).max()):.2e} of the magnitude sum"


def _stats_ref(out, q=None):
    q = out if q is None else q
    return torch.stack([out.double().sum((0, 2, 3)), (out.double() * q.double()).sum((0, 2, 3))], 1)


@pytest.mark.parametrize("cin,nout,hw,ones,mode", [
    (3, 8, 128, True, 0), (8, 16, 64, False, 3), (16, 16, 32, False, 3),
    (4, 4, 128, False, 0), (4, 8, 64, False, 0), (8, 16, 32, False, 0), (5, 8, 128, True, 0), (16, 16, 64, False, 2),
    (8, 16, 128, False, 1)])
def test_conv4x4s2(ops, cin, nout, hw, ones, mode):
    B = 3
    cphys = cin - (1 if ones else 0)
    x = rnd(B, cphys, hw, hw, seed=1)
    w = rnd(nout, cin, 4, 4, seed=2, scale=0.2)
    bias = rnd(nout, seed=3)
    coef = torch.stack([rnd(cphys, seed=4).abs() + 0.5, torch.zeros(cphys), rnd(cphys, seed=5) * 0.3, torch.zeros(cphys)], 1)
    xin = load_ref(x, mode, coef)
    if ones:
        xin = torch.cat([xin, torch.ones(B, 1, hw, hw)], 1)
    ref = F.conv2d(xin, w, bias, stride=2, padding=1)
    out, st = ops.conv4x4s2(ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, ones=ones),
                            ops.weight_view(w.to(DEV), cin * 16, 16, 4, 1), B, cin, nout, hw, hw, want_stats=True,
                            bias=bias.to(DEV))
    close(out, ref, 2e-5, 2e-5, "conv4x4s2")
    close(st.sum(0), _stats_ref(ref), 1e-5, 1e-3, "stats")


@pytest.mark.parametrize("B,mode,per_sample,relu", [(1, 3, False, False), (5, 0, False, False), (300, 3, False, False),
                                                     (7, 1, False, True), (6, 2, True, False), (260, 3, True, False)])
def test_conv4x4s2_whole_patch_forward_kernel(ops, B, mode, per_sample, relu):
    """enc.7's shape (16 -> 16 channels, 32 x 32 -> 16 x 16) runs on the whole-patch kernel (conv4x4s2_patch.hip): every operand
    mode, per-sample coefficients, output ReLU, batch statistics slabs and the per-patch slabs of the inference path."""
    C = 16
    x = rnd(B, C, 32, 32, seed=B)
    w = rnd(C, C, 4, 4, seed=2, scale=0.2)
    bias = rnd(C, seed=3)
    if per_sample:
        coef = torch.stack([rnd(B, C, seed=4).abs() + 0.5, torch.zeros(B, C), rnd(B, C, seed=5) * 0.3, torch.zeros(B, C)], 2)
    else:
        coef = torch.stack([rnd(C, seed=4).abs() + 0.5, torch.zeros(C), rnd(C, seed=5) * 0.3, torch.zeros(C)], 1)
    ref = F.conv2d(load_ref(x, mode, coef), w, bias, stride=2, padding=1)
    if relu:
        ref = ref.clamp(min=0)
    out, st = ops.conv4x4s2(ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, per_sample=per_sample),
                            ops.weight_view(w.to(DEV), C * 16, 16, 4, 1), B, C, C, 32, 32, want_stats=True, bias=bias.to(DEV),
                            relu=relu, per_tile=per_sample)
    close(out, ref, 2e-5, 2e-5, "conv4x4s2 (whole patch)")
    if per_sample:
        assert st.shape[0] % B == 0
        got = st.reshape(B, st.shape[0] // B, C, 2).sum(1).cpu()
        want = torch.stack([ref.double().sum((2, 3)), (ref.double() ** 2).sum((2, 3))], 2)
        close(got, want, 1e-5, 1e-3, "per-patch statistics")
    else:
        close(st.sum(0), _stats_ref(ref), 1e-5, 1e-3, "stats")
    out2, st2 = ops.conv4x4s2(ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, per_sample=per_sample),
                              ops.weight_view(w.to(DEV), C * 16, 16, 4, 1), B, C, C, 32, 32, want_stats=True, bias=bias.to(DEV),
                              relu=relu, per_tile=per_sample)
    assert torch.equal(out2, out) and torch.equal(st2, st)


def test_conv4x4s2_epilogue_mask_resid_and_convT_view(ops):
    """Data gradient of a ConvTranspose2d(4,2,1): conv over g with the [ci][co] weight read in place."""
    B, ci, co, h = 2, 8, 4, 32          # convT: (B,ci,h,h) -> (B,co,2h,2h)
    wt = rnd(ci, co, 4, 4, seed=1, scale=0.2)
    g = rnd(B, co, 2 * h, 2 * h, seed=2)
    act = rnd(B, ci, h, h, seed=3)
    resid = rnd(B, ci, h, h, seed=4)
    ref = F.conv2d(g, wt, None, stride=2, padding=1) * (act > 0) + resid
    out, st = ops.conv4x4s2(ops.Op(g.to(DEV)), ops.weight_view(wt.to(DEV), co * 16, 16, 4, 1), B, co, ci, 2 * h, 2 * h,
                            want_stats=True, mask=ops.Op(act.to(DEV)), resid=resid.to(DEV), stat_q=act.to(DEV))
    close(out, ref, 2e-5, 2e-5, "dgrad convT")
    close(st.sum(0), _stats_ref(ref, act), 1e-5, 1e-3, "stats q")
    # cross-check against autograd
    inp = act.clone().requires_grad_(True)
    F.conv_transpose2d(inp, wt, None, stride=2, padding=1).backward(g)
    close(out.cpu() - resid, inp.grad * (act > 0), 2e-5, 2e-5, "autograd")


@pytest.mark.parametrize("cin,nout,hw,taps", [(16, 16, 16, 9), (16, 32, 16, 9), (32, 16, 16, 9), (16, 16, 32, 9),
                                              (32, 16, 16, 1), (16, 32, 16, 1), (32, 16, 32, 1), (16, 32, 32, 9)])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_conv3x3_plain(ops, cin, nout, hw, taps, mode):
    B = 3
    k = 3 if taps == 9 else 1
    x = rnd(B, cin, hw, hw, seed=1)
    w = rnd(nout, cin, k, k, seed=2, scale=0.2)
    bias = rnd(nout, seed=3)
    coef = torch.stack([rnd(cin, seed=4).abs() + 0.5, torch.zeros(cin), rnd(cin, seed=5) * 0.3, torch.zeros(cin)], 1)
    ref = F.conv2d(load_ref(x, mode, coef), w, bias, padding=k // 2)
    out, st = ops.conv3x3(ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None),
                          ops.weight_view(w.to(DEV), cin * k * k, k * k, k, 1), B, cin, nout, hw, hw, taps=taps,
                          want_stats=True, bias=bias.to(DEV))
    close(out, ref, 2e-5, 2e-5, "conv3x3")
    close(st.sum(0), _stats_ref(ref), 1e-5, 1e-3, "stats")


def test_conv3x3_dgrad_views_affine2_mask(ops):
    """Data gradient of a 3x3 conv: flipped/transposed weight view + AFFINE2 load + AFFINE mask + resid."""
    B, ci, co, h = 2, 16, 32, 16
    w = rnd(co, ci, 3, 3, seed=1, scale=0.2)
    dy, a = rnd(B, co, h, h, seed=2), rnd(B, co, h, h, seed=3)
    coef = torch.stack([rnd(co, seed=4), rnd(co, seed=5) * 0.1, rnd(co, seed=6) * 0.1, torch.zeros(co)], 1)
    prev = rnd(B, ci, h, h, seed=7)
    mcoef = torch.stack([rnd(ci, seed=8), torch.zeros(ci), rnd(ci, seed=9) * 0.2, torch.zeros(ci)], 1)
    resid = rnd(B, ci, h, h, seed=10)
    da = load_ref(dy, 4, coef, a)
    x = torch.zeros(B, ci, h, h, requires_grad=True)
    F.conv2d(x, w, None, padding=1).backward(da)
    ref = x.grad * (load_ref(prev, 2, mcoef) > 0) + resid
    out, st = ops.conv3x3(ops.Op(dy.to(DEV), 4, coef.to(DEV), p1=a.to(DEV)),
                          ops.weight_view(w.to(DEV), 9, ci * 9, -3, -1, off=8), B, co, ci, h, h, taps=9, want_stats=True,
                          mask=ops.Op(prev.to(DEV), 2, mcoef.to(DEV)), resid=resid.to(DEV), stat_q=prev.to(DEV))
    close(out, ref, 3e-5, 3e-5, "dgrad3x3")
    close(st.sum(0), _stats_ref(ref, prev), 1e-5, 2e-3, "stats")
    # 1x1 data gradient
    w1 = rnd(ci, co, 1, 1, seed=11, scale=0.2)      # conv co -> ci ; dgrad maps (B,ci) grads -> (B,co)
    gy = rnd(B, ci, h, h, seed=12)
    x1 = torch.zeros(B, co, h, h, requires_grad=True)
    F.conv2d(x1, w1).backward(gy)
    out1, _ = ops.conv3x3(ops.Op(gy.to(DEV)), ops.weight_view(w1.to(DEV), 1, co, 0, 0), B, ci, co, h, h, taps=1)
    close(out1, x1.grad, 2e-5, 2e-5, "dgrad1x1")


@pytest.mark.parametrize("ci,co,hw", [(16, 8, 16), (8, 4, 32), (4, 4, 64), (16, 16, 16), (16, 8, 32), (16, 8, 64), (8, 4, 64)])
def test_conv_transpose_pixel_shuffle(ops, ci, co, hw):
    B = 2
    x = rnd(B, ci, hw, hw, seed=1)
    wt = rnd(ci, co, 4, 4, seed=2, scale=0.2)
    bias = rnd(co, seed=3)
    ref = F.relu(F.conv_transpose2d(x, wt, bias, stride=2, padding=1))
    out, st = ops.conv3x3(ops.Op(x.to(DEV)), ops.weight_view(wt.to(DEV), 16, co * 16, 4, 1), B, ci, 4 * co, hw, hw,
                          taps=9, pixel_shuffle=True, want_stats=True, bias=bias.to(DEV), relu=True)
    close(out, ref, 2e-5, 2e-5, "convT")
    close(st.sum(0), _stats_ref(ref), 1e-5, 1e-3, "stats")


def test_conv_dgrad_of_strided_conv_pixel_shuffle(ops):
    """Data gradient of Conv2d(8->16,4,2,1) = transposed conv read from the [co][ci] weight, with mask/stats."""
    B, ci, co, h = 2, 8, 16, 32          # conv input (B,ci,2h,2h) -> output (B,co,h,h)
    w = rnd(co, ci, 4, 4, seed=1, scale=0.2)
    gy = rnd(B, co, h, h, seed=2)
    a_prev = rnd(B, ci, 2 * h, 2 * h, seed=3)
    mcoef = torch.stack([rnd(ci, seed=8), torch.zeros(ci), rnd(ci, seed=9) * 0.2, torch.zeros(ci)], 1)
    x = torch.zeros(B, ci, 2 * h, 2 * h, requires_grad=True)
    F.conv2d(x, w, None, stride=2, padding=1).backward(gy)
    ref = x.grad * (load_ref(a_prev, 2, mcoef) > 0)
    out, st = ops.conv3x3(ops.Op(gy.to(DEV)), ops.weight_view(w.to(DEV), 16, ci * 16, 4, 1), B, co, 4 * ci, h, h, taps=9,
                          pixel_shuffle=True, want_stats=True, mask=ops.Op(a_prev.to(DEV), 2, mcoef.to(DEV)),
                          stat_q=a_prev.to(DEV))
    close(out, ref, 3e-5, 3e-5, "dgrad strided")
    close(st.sum(0), _stats_ref(ref, a_prev), 1e-5, 2e-3, "stats")


# ===================================================================== generic fallback kernels
@pytest.mark.parametrize("cin,nout,h,w,mode,ones", [(24, 40, 20, 36, 3, False), (6, 33, 128, 128, 0, True), (32, 64, 64, 64, 3, False)])
def test_generic_conv4x4s2(ops, cin, nout, h, w, mode, ones):
    """Channel counts / sizes without an MFMA instantiation fall through to conv_generic.hip (same semantics)."""
    B = 3
    cphys = cin - (1 if ones else 0)
    x = rnd(B, cphys, h, w, seed=1)
    wt = rnd(nout, cin, 4, 4, seed=2, scale=0.2)
    bias = rnd(nout, seed=3)
    coef = torch.stack([rnd(cphys, seed=4).abs() + 0.5, torch.zeros(cphys), rnd(cphys, seed=5) * 0.3, torch.zeros(cphys)], 1)
    xin = load_ref(x, mode, coef)
    if ones:
        xin = torch.cat([xin, torch.ones(B, 1, h, w)], 1)
    ref = F.conv2d(xin, wt, bias, stride=2, padding=1)
    out, st = ops.conv4x4s2(ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, ones=ones),
                            ops.weight_view(wt.to(DEV), cin * 16, 16, 4, 1), B, cin, nout, h, w, want_stats=True,
                            bias=bias.to(DEV))
    close(out, ref, 5e-5, 5e-5, "generic conv4x4s2")
    close(st.sum(0), _stats_ref(ref), 1e-5, 1e-3, "stats")


@pytest.mark.parametrize("cin,nout,hw,taps", [(20, 12, 10, 9), (64, 64, 16, 9), (64, 32, 16, 1), (48, 16, 12, 1)])
def test_generic_conv3x3(ops, cin, nout, hw, taps):
    B = 2
    x = rnd(B, cin, hw, hw, seed=1)
    k = 3 if taps == 9 else 1
    wt = rnd(nout, cin, k, k, seed=2, scale=0.2)
    act, resid = rnd(B, nout, hw, hw, seed=3), rnd(B, nout, hw, hw, seed=4)
    ref = F.conv2d(F.relu(x), wt, None, padding=k // 2) * (act > 0) + resid
    out, st = ops.conv3x3(ops.Op(x.to(DEV), 1), ops.weight_view(wt.to(DEV), cin * taps, taps, 3 if taps == 9 else 0, 1 if taps == 9 else 0),
                          B, cin, nout, hw, hw, taps=taps, want_stats=True, mask=ops.Op(act.to(DEV)), resid=resid.to(DEV),
                          stat_q=act.to(DEV))
    close(out, ref, 5e-5, 5e-5, "generic conv3x3")
    close(st.sum(0), _stats_ref(ref, act), 1e-5, 1e-3, "stats q")


@pytest.mark.parametrize("ci,co,hw", [(12, 6, 6), (64, 32, 16), (32, 16, 32)])
def test_generic_conv_transpose(ops, ci, co, hw):
    B = 2
    x = rnd(B, ci, hw, hw, seed=1)
    wt = rnd(ci, co, 4, 4, seed=2, scale=0.2)
    bias = rnd(co, seed=3)
    ref = F.relu(F.conv_transpose2d(x, wt, bias, stride=2, padding=1))
    out, st = ops.conv3x3(ops.Op(x.to(DEV)), ops.weight_view(wt.to(DEV), 16, co * 16, 4, 1), B, ci, 4 * co, hw, hw,
                          taps=9, pixel_shuffle=True, want_stats=True, bias=bias.to(DEV), relu=True)
    close(out, ref, 5e-5, 5e-5, "generic conv transpose")
    close(st.sum(0), _stats_ref(ref), 1e-5, 1e-3, "stats")


@pytest.mark.parametrize("cs,ct,k,hs", [(12, 20, 4, 10), (64, 64, 3, 16), (32, 64, 1, 16), (64, 32, 4, 16)])
def test_generic_wgrad(ops, cs, ct, k, hs):
    B = 3
    s, p = (2, 1) if k == 4 else ((1, 1) if k == 3 else (1, 0))
    ht = hs * s
    S = rnd(B, cs, hs, hs, seed=1)
    T = rnd(B, ct, ht, ht, seed=2)
    w = torch.zeros(cs, ct, k, k, requires_grad=True)
    F.conv2d(T, w, None, stride=s, padding=p).backward(S)
    dst = torch.empty(cs, ct, k, k, device=DEV)
    ops.wgrad(ops.Op(S.to(DEV)), ops.Op(T.to(DEV)), dst, B, cs, ct, hs, hs, k)
    close(dst, w.grad, 5e-5, 5e-5 * w.grad.abs().max().item(), "generic wgrad")


# ===================================================================== implicit-GEMM kernels (conv_wide.hip)
# channel counts without a register-resident instantiation whose base grid tiles by 8 x 16
@pytest.mark.parametrize("B,cin,nout,h,w,mode,ones,per_tile", [
    (3, 32, 64, 64, 64, 3, False, False), (2, 64, 64, 32, 32, 4, False, False), (5, 3, 32, 128, 128, 0, True, False),
    (4, 32, 64, 32, 64, 3, False, True), (2, 20, 72, 16, 32, 1, False, False), (40, 32, 16, 32, 32, 0, False, False)])
def test_wide_conv4x4s2(ops, B, cin, nout, h, w, mode, ones, per_tile):
    cphys = cin - (1 if ones else 0)
    x, x1 = rnd(B, cphys, h, w, seed=1), rnd(B, cphys, h, w, seed=11)
    wt = rnd(nout, cin, 4, 4, seed=2, scale=0.2)
    bias = rnd(nout, seed=3)
    coef = torch.stack([rnd(cphys, seed=4).abs() + 0.5, rnd(cphys, seed=6) * 0.2, rnd(cphys, seed=5) * 0.3, torch.zeros(cphys)], 1)
    xin = load_ref(x, mode, coef, x1)
    if ones:
        xin = torch.cat([xin, torch.ones(B, 1, h, w)], 1)
    ref = F.conv2d(xin, wt, bias, stride=2, padding=1)
    out, st = ops.conv4x4s2(ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, p1=x1.to(DEV) if mode == 4 else None, ones=ones),
                            ops.weight_view(wt.to(DEV), cin * 16, 16, 4, 1), B, cin, nout, h, w, want_stats=True,
                            bias=bias.to(DEV), per_tile=per_tile)
    close(out, ref, 5e-5, 5e-5, "wide conv4x4s2")
    if per_tile:
        assert st.shape[0] % B == 0
        per = st.reshape(B, -1, nout, 2).sum(1)
        for b in range(B):
            close_stats(per[b], ref[b:b + 1], None, f"per-sample stats {b}")
    else:
        close_stats(st.sum(0), ref)


def test_wide_conv4x4s2_border_bias(ops):
    """enc.0 o enc.1 of a wide encoder: 2 -> 32 channels with the border-bias table instead of a ones channel."""
    B, nin, c1, h = 3, 2, 32, 128
    x = rnd(B, nin, h, h, seed=1)
    w0, b0 = rnd(nin, nin, 1, 1, seed=2), rnd(nin, seed=3)
    w1, b1 = rnd(c1, nin, 4, 4, seed=4, scale=0.2), rnd(c1, seed=5)
    ref = F.conv2d(F.conv2d(x, w0, b0), w1, b1, stride=2, padding=1)
    weff, border = ops.e1_compose_border(w0.to(DEV), b0.to(DEV), w1.to(DEV), b1.to(DEV))
    out, st = ops.conv4x4s2(ops.Op(x.to(DEV)), ops.weight_view(weff, (nin + 1) * 16, 16, 4, 1), B, nin, c1, h, h,
                            want_stats=True, bias_border=border)
    close(out, ref, 5e-5, 5e-5, "wide conv4x4s2 with border bias")
    close(st.sum(0), _stats_ref(ref), 1e-5, 1e-3, "stats")


@pytest.mark.parametrize("B,cin,nout,h,w,taps,per_tile", [(2, 64, 64, 16, 16, 9, False), (3, 64, 64, 32, 32, 9, False),
                                                          (2, 64, 64, 16, 16, 1, False), (3, 128, 40, 8, 32, 1, False),
                                                          (2, 48, 136, 16, 16, 9, False), (4, 64, 64, 16, 16, 9, True),
                                                          (70, 64, 32, 16, 16, 9, False), (2, 16, 128, 16, 16, 9, False),
                                                          (2, 16, 128, 16, 16, 1, False)])
def test_wide_conv3x3(ops, B, cin, nout, h, w, taps, per_tile):
    x = rnd(B, cin, h, w, seed=1)
    k = 3 if taps == 9 else 1
    wt = rnd(nout, cin, k, k, seed=2, scale=0.1)
    act, resid = rnd(B, nout, h, w, seed=3), rnd(B, nout, h, w, seed=4)
    mcoef = torch.stack([rnd(nout, seed=7), torch.zeros(nout), rnd(nout, seed=8) * 0.3, torch.zeros(nout)], 1)
    gate = (mcoef[:, 0].view(1, -1, 1, 1) * act + mcoef[:, 2].view(1, -1, 1, 1)) > 0
    ref = F.conv2d(F.relu(x), wt, None, padding=k // 2) * gate + resid
    out, st = ops.conv3x3(ops.Op(x.to(DEV), 1), ops.weight_view(wt.to(DEV), cin * taps, taps, 3 if taps == 9 else 0, 1 if taps == 9 else 0),
                          B, cin, nout, h, w, taps=taps, want_stats=True, mask=ops.Op(act.to(DEV), 2, mcoef.to(DEV)),
                          resid=resid.to(DEV), stat_q=act.to(DEV), per_tile=per_tile)
    close(out, ref, 5e-5, 5e-5, "wide conv3x3")
    if per_tile:
        per = st.reshape(B, -1, nout, 2).sum(1)
        for b in range(B):
            close_stats(per[b], ref[b:b + 1], act[b:b + 1], f"per-sample stats {b}")
    else:
        close_stats(st.sum(0), ref, act, "stats q")


@pytest.mark.parametrize("B,ci,co,hw,taps", [(2, 64, 48, 16, 9), (2, 128, 16, 16, 9), (2, 16, 128, 16, 1), (3, 128, 16, 16, 1)])
def test_wide_conv_data_gradient_with_bn_backward_operand(ops, B, ci, co, hw, taps):
    """Data gradient of a 3x3 / 1x1 convolution as the encoder backward pass calls it: input = BatchNorm backward
    folded into the load (AFFINE2), transposed (and for 3x3 flipped) weight view, ReLU gate, residual, statistics."""
    k = 3 if taps == 9 else 1
    dy, a = rnd(B, co, hw, hw, seed=1), rnd(B, co, hw, hw, seed=2)
    coef = torch.stack([rnd(co, seed=3), rnd(co, seed=4) * 0.1, rnd(co, seed=5) * 0.1, torch.zeros(co)], 1)
    g = load_ref(dy, 4, coef, a)
    wt = rnd(co, ci, k, k, seed=6, scale=0.1)
    x = torch.zeros(B, ci, hw, hw, requires_grad=True)
    F.conv2d(x, wt, None, padding=k // 2).backward(g)
    gate, resid, q = rnd(B, ci, hw, hw, seed=7), rnd(B, ci, hw, hw, seed=8), rnd(B, ci, hw, hw, seed=9)
    ref = x.grad * (gate > 0) + resid
    wv = ops.weight_view(wt.to(DEV), 9, ci * 9, -3, -1, off=8) if taps == 9 else ops.weight_view(wt.to(DEV), 1, ci, 0, 0)
    out, st = ops.conv3x3(ops.Op(dy.to(DEV), 4, coef.to(DEV), p1=a.to(DEV)), wv, B, co, ci, hw, hw, taps=taps, want_stats=True,
                          mask=ops.Op(gate.to(DEV)), resid=resid.to(DEV), stat_q=q.to(DEV))
    close(out, ref, 5e-5, 5e-5, "data gradient")
    close_stats(st.sum(0), ref, q)


@pytest.mark.parametrize("B,ci,co,h,w", [(2, 64, 32, 16, 16), (2, 32, 2, 64, 64), (3, 64, 64, 8, 16), (2, 32, 16, 32, 32),
                                         (50, 16, 16, 32, 64)])
def test_wide_conv_transpose(ops, B, ci, co, h, w):
    x = rnd(B, ci, h, w, seed=1)
    wt = rnd(ci, co, 4, 4, seed=2, scale=0.2)
    bias = rnd(co, seed=3)
    act = rnd(B, co, 2 * h, 2 * w, seed=5)
    ref = F.relu(F.conv_transpose2d(x, wt, bias, stride=2, padding=1)) * (act > 0)
    out, st = ops.conv3x3(ops.Op(x.to(DEV)), ops.weight_view(wt.to(DEV), 16, co * 16, 4, 1), B, ci, 4 * co, h, w,
                          taps=9, pixel_shuffle=True, want_stats=True, bias=bias.to(DEV), relu=True, mask=ops.Op(act.to(DEV)),
                          stat_q=act.to(DEV))
    close(out, ref, 5e-5, 5e-5, "wide conv transpose")
    close_stats(st.sum(0), ref, act)


@pytest.mark.parametrize("B,cs,ct,k,hs,ws,ones", [(3, 64, 64, 3, 16, 16, False), (3, 64, 64, 1, 16, 16, False),
                                                 (3, 64, 32, 4, 16, 16, False), (2, 32, 3, 4, 64, 64, True),
                                                 (2, 32, 2, 4, 64, 64, False), (2, 128, 20, 3, 8, 32, False),
                                                 (40, 32, 64, 4, 32, 32, False), (3, 64, 100, 1, 16, 32, False),
                                                 (2, 16, 16, 4, 64, 64, False), (2, 16, 40, 3, 16, 16, False), (3, 48, 24, 4, 16, 16, False)])
def test_wide_wgrad(ops, B, cs, ct, k, hs, ws, ones):
    s, p = (2, 1) if k == 4 else ((1, 1) if k == 3 else (1, 0))
    ctp = ct - (1 if ones else 0)
    dy, a = rnd(B, cs, hs, ws, seed=1), rnd(B, cs, hs, ws, seed=2)
    coef = torch.stack([rnd(cs, seed=3), rnd(cs, seed=4) * 0.1, rnd(cs, seed=5) * 0.1, torch.zeros(cs)], 1)
    t = rnd(B, ctp, hs * s, ws * s, seed=6)
    tcoef = torch.stack([rnd(ctp, seed=7), torch.zeros(ctp), rnd(ctp, seed=8) * 0.2, torch.zeros(ctp)], 1)
    tin = load_ref(t, 3, tcoef)
    if ones:
        tin = torch.cat([tin, torch.ones(B, 1, hs * s, ws * s)], 1)
    w = torch.zeros(cs, ct, k, k, requires_grad=True)
    F.conv2d(tin, w, None, stride=s, padding=p).backward(load_ref(dy, 4, coef, a))
    dst = torch.empty(cs, ct, k, k, device=DEV)
    ops.wgrad(ops.Op(dy.to(DEV), 4, coef.to(DEV), p1=a.to(DEV)), ops.Op(t.to(DEV), 3, tcoef.to(DEV), ones=ones), dst, B, cs, ct,
              hs, ws, k)
    scale = w.grad.abs().max().item()
    close(dst, w.grad, 5e-5, 5e-5 * scale, "wide wgrad")


def _wide_random_cases(n, seed):
    import random
    rng = random.Random(seed)
    cases = []
    for i in range(n):
        form = ("s2", "s1_9", "s1_1", "pix")[i % 4]
        cin = rng.choice([1, 3, 7, 8, 9, 17, 24, 40, 65])
        nout = rng.choice([1, 2, 15, 16, 17, 33, 48, 70])
        h, w = rng.choice([8, 16, 24]), rng.choice([16, 32, 48])
        cases.append((form, rng.randint(1, 4), cin, nout, h, w, rng.choice([0, 1, 3, 4]), rng.random() < 0.3, 1000 + i))
    return cases


@pytest.mark.parametrize("form,B,cin,nout,h,w,mode,per_tile,seed", _wide_random_cases(24, 7))
def test_wide_conv_random_shapes(ops, form, B, cin, nout, h, w, mode, per_tile, seed):
    """Seeded sweep over channel counts that are not multiples of anything, all three forms, operand modes, ReLU / gate /
    residual epilogues and both statistics groupings -- against torch on the CPU."""
    if form == "s2":
        h, w = 2 * h, 2 * w
    x, x1 = rnd(B, cin, h, w, seed=seed), rnd(B, cin, h, w, seed=seed + 1)
    coef = torch.stack([rnd(cin, seed=seed + 2).abs() + 0.5, rnd(cin, seed=seed + 3) * 0.2, rnd(cin, seed=seed + 4) * 0.3,
                        torch.zeros(cin)], 1)
    xin = load_ref(x, mode, coef, x1)
    inp = ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, p1=x1.to(DEV) if mode == 4 else None)
    bias = rnd(nout, seed=seed + 5)
    if form == "s2":
        wt = rnd(nout, cin, 4, 4, seed=seed + 6, scale=0.2)
        ref = F.conv2d(xin, wt, bias, stride=2, padding=1)
        call = lambda **kw: ops.conv4x4s2(inp, ops.weight_view(wt.to(DEV), cin * 16, 16, 4, 1), B, cin, nout, h, w, **kw)
    elif form == "pix":
        wt = rnd(cin, nout, 4, 4, seed=seed + 6, scale=0.2)
        ref = F.conv_transpose2d(xin, wt, bias, stride=2, padding=1)
        call = lambda **kw: ops.conv3x3(inp, ops.weight_view(wt.to(DEV), 16, nout * 16, 4, 1), B, cin, 4 * nout, h, w, taps=9,
                                        pixel_shuffle=True, **kw)
    else:
        k = 3 if form == "s1_9" else 1
        wt = rnd(nout, cin, k, k, seed=seed + 6, scale=0.2)
        ref = F.conv2d(xin, wt, bias, padding=k // 2)
        wv = ops.weight_view(wt.to(DEV), cin * k * k, k * k, k if k == 3 else 0, 1 if k == 3 else 0)
        call = lambda **kw: ops.conv3x3(inp, wv, B, cin, nout, h, w, taps=k * k, **kw)
    gate, resid = rnd(*ref.shape, seed=seed + 7), rnd(*ref.shape, seed=seed + 8)
    ref = F.relu(ref) * (gate > 0) + resid
    out, st = call(want_stats=True, bias=bias.to(DEV), relu=True, mask=ops.Op(gate.to(DEV)), resid=resid.to(DEV),
                   stat_q=gate.to(DEV), per_tile=per_tile)
    close(out, ref, 5e-5, 5e-5, f"{form} output")
    if per_tile:
        per = st.reshape(B, -1, nout, 2).sum(1)
        for b in range(B):
            close_stats(per[b], ref[b:b + 1], gate[b:b + 1], f"per-sample stats {b}")
    else:
        close_stats(st.sum(0), ref, gate)


def _wide_wgrad_random_cases(n, seed):
    import random
    rng = random.Random(seed)
    out = []
    for i in range(n):
        k = (4, 3, 1)[i % 3]
        out.append((rng.randint(1, 5), rng.choice([1, 5, 16, 17, 33, 64, 70]), rng.choice([1, 2, 9, 16, 29, 65]), k,
                    rng.choice([8, 16, 24]), rng.choice([16, 32]), rng.choice([0, 1, 3, 4]), rng.choice([0, 1, 3]), 2000 + i))
    return out


@pytest.mark.parametrize("B,cs,ct,k,hs,ws,smode,tmode,seed", _wide_wgrad_random_cases(18, 11))
def test_wide_wgrad_random_shapes(ops, B, cs, ct, k, hs, ws, smode, tmode, seed):
    """Seeded sweep of the implicit-GEMM weight gradient: channel counts on neither side of any tile size, the three
    kernel sizes, every operand mode on both operands."""
    s_, p_ = (2, 1) if k == 4 else ((1, 1) if k == 3 else (1, 0))
    dy, a = rnd(B, cs, hs, ws, seed=seed), rnd(B, cs, hs, ws, seed=seed + 1)
    coef = torch.stack([rnd(cs, seed=seed + 2), rnd(cs, seed=seed + 3) * 0.1, rnd(cs, seed=seed + 4) * 0.1, torch.zeros(cs)], 1)
    t = rnd(B, ct, hs * s_, ws * s_, seed=seed + 5)
    tcoef = torch.stack([rnd(ct, seed=seed + 6), torch.zeros(ct), rnd(ct, seed=seed + 7) * 0.2, torch.zeros(ct)], 1)
    w = torch.zeros(cs, ct, k, k, requires_grad=True)
    F.conv2d(load_ref(t, tmode, tcoef), w, None, stride=s_, padding=p_).backward(load_ref(dy, smode, coef, a))
    dst = torch.empty(cs, ct, k, k, device=DEV)
    ops.wgrad(ops.Op(dy.to(DEV), smode, coef.to(DEV) if smode >= 2 else None, p1=a.to(DEV) if smode == 4 else None),
              ops.Op(t.to(DEV), tmode, tcoef.to(DEV) if tmode >= 2 else None), dst, B, cs, ct, hs, ws, k)
    close(dst, w.grad, 5e-5, 5e-5 * max(w.grad.abs().max().item(), 1e-6), "wide wgrad")


# =============================================================================== wgrad
@pytest.mark.parametrize("B,H,W,two", [(3, 16, 16, True), (70, 16, 16, True), (5, 32, 32, True), (2, 16, 16, False), (513, 16, 16, True)])
def test_conv1x1_backward_fused_equals_the_two_kernels(ops, B, H, W, two):
    """dm_conv1x1_bwd_fused (data + weight gradient of the ResidualBlock's 1x1 convolution from one staging) against
    dm_conv3x3(taps = 1, mask, stat_q) + dm_wgrad and against a float64 restatement of both."""
    CD, CX = 16, 32
    g = torch.Generator().manual_seed(B * 7 + H)
    gy, y = torch.randn(B, CD, H, W, generator=g), torch.randn(B, CD, H, W, generator=g)
    x = torch.randn(B, CX, H, W, generator=g)
    w = torch.randn(CD, CX, 1, 1, generator=g) * 0.2
    cd = torch.randn(CD, 4, generator=g) * 0.5
    cx = torch.zeros(CX, 4)
    cx[:, 0] = torch.rand(CX, generator=g) + 0.5
    cx[:, 2] = torch.randn(CX, generator=g) * 0.3
    d = lambda t: t.to(DEV)
    dy_op = ops.Op(d(gy), 4, d(cd), p1=d(y)) if two else ops.Op(d(gy))
    dst = torch.zeros(CD, CX, 1, 1, device=DEV)
    dx, st = ops.conv1x1_bwd_fused(dy_op, d(x), d(cx), d(w), dst, B, CD, CX, H, W)
    # the two kernels it replaces
    dst2 = torch.zeros(CD, CX, 1, 1, device=DEV)
    ops.wgrad(dy_op, ops.Op(d(x), 3, d(cx)), dst2, B, CD, CX, H, W, 1)
    dx2, st2 = ops.conv3x3(dy_op, ops.weight_view(d(w), 1, CX, 0, 0), B, CD, CX, H, W, taps=1, want_stats=True,
                           like=d(gy), mask=ops.Op(d(x), 2, d(cx)), stat_q=d(x))
    # float64 truth
    da = (cd[:, 0].view(1, CD, 1, 1).double() * gy.double() + cd[:, 1].view(1, CD, 1, 1).double() * y.double()
          + cd[:, 2].view(1, CD, 1, 1).double()) if two else gy.double()
    t = cx[:, 0].view(1, CX, 1, 1).double() * x.double() + cx[:, 2].view(1, CX, 1, 1).double()
    dx_ref = torch.einsum("oc,bohw->bchw", w[:, :, 0, 0].double(), da) * (t > 0)
    dw_ref = torch.einsum("bohw,bchw->oc", da, t.clamp(min=0))
    tol = 2e-6 * float(dx_ref.abs().max())
    near = t.abs() < 1e-5                                                # (a fp32 / fp64 disagreement about the sign of t)
    assert float(((dx.cpu().double() - dx_ref).abs() * ~near).max()) <= tol
    assert float(((dx.cpu().double() - dx2.cpu().double()).abs()).max()) <= tol
    close(dst.cpu().reshape(CD, CX), dw_ref.float(), 1e-5, 2e-5 * float(dw_ref.abs().max()), "weight gradient vs float64")
    close(dst, dst2, 1e-5, 2e-5 * float(dw_ref.abs().max()), "weight gradient vs dm_wgrad")
    s_f = st.sum(0).cpu()
    s_2 = st2.sum(0).cpu()
    assert st.shape[1:] == (CX, 2)
    close(s_f, s_2, 1e-9, 1e-9 * float(s_2.abs().max()) + 1e-6, "statistics slabs")
    want1 = (dx.cpu().double()).sum((0, 2, 3))
    want2 = (dx.cpu().double() * x.double()).sum((0, 2, 3))
    close(s_f[:, 0], want1, 1e-6, 1e-6 * float(want1.abs().max()) + 1e-6, "sum dx")
    close(s_f[:, 1], want2, 1e-6, 1e-6 * float(want2.abs().max()) + 1e-6, "sum dx * x")
    # bit-reproducible (no float atomics: slabs in slab order, waves in wave order)
    dst3 = torch.zeros(CD, CX, 1, 1, device=DEV)
    dx3, st3 = ops.conv1x1_bwd_fused(dy_op, d(x), d(cx), d(w), dst3, B, CD, CX, H, W)
    assert torch.equal(dx3, dx) and torch.equal(st3, st) and torch.equal(dst3, dst)
    assert not ops.conv1x1_bwd_fused_supported(CD, CX, 8, 8) and not ops.conv1x1_bwd_fused_supported(48, 48, 16, 16)


@pytest.mark.parametrize("B,CD,form,hw", [(3, 16, "enc10", (16, 16)), (70, 16, "enc10", (16, 16)), (5, 32, "res", (16, 16)),
                                          (300, 32, "res", (16, 16)), (4, 32, "res_noq", (16, 16)), (2, 16, "ident", (16, 16)),
                                          # 32-column latent grids (32 x 32: C5, default-width z32): bands of 8 rows with halo rows
                                          (3, 32, "res", (32, 32)), (70, 32, "res", (32, 32)), (3, 32, "res_noq", (32, 32)),
                                          (300, 32, "res", (32, 32)),
                                          # the 32-channel forms without a second gradient tensor / with xcoef
                                          (2, 32, "ident", (16, 16)), (3, 32, "enc10", (16, 16)), (3, 32, "ident", (32, 32))])
def test_conv3x3_backward_fused_equals_the_two_kernels(ops, B, CD, form, hw):
    """dm_conv3x3_bwd_fused (data + weight gradient of enc.10 / the ResidualBlock's 3x3 convolution from one staging of the
    patch) against dm_conv3x3 + dm_wgrad and against autograd's conv2d backward in float64."""
    CX, (H, W) = 16, hw
    g = torch.Generator().manual_seed(B * 3 + CD)
    gy, y = torch.randn(B, CD, H, W, generator=g), torch.randn(B, CD, H, W, generator=g)
    x = torch.randn(B, CX, H, W, generator=g)
    w = torch.randn(CD, CX, 3, 3, generator=g) * 0.2
    cd = torch.randn(CD, 4, generator=g) * 0.5
    d = lambda t: t.to(DEV)
    two = form != "ident"
    dy_op = ops.Op(d(gy), 4, d(cd), p1=d(y)) if two else ops.Op(d(gy))
    da = (cd[:, 0].view(1, CD, 1, 1).double() * gy.double() + cd[:, 1].view(1, CD, 1, 1).double() * y.double()
          + cd[:, 2].view(1, CD, 1, 1).double()) if two else gy.double()
    if form in ("enc10", "ident"):
        cx = torch.zeros(CX, 4)
        cx[:, 0] = torch.rand(CX, generator=g) + 0.5
        cx[:, 2] = torch.randn(CX, generator=g) * 0.3
        xcoef, resid, q = d(cx), None, d(x)
        t = cx[:, 0].view(1, CX, 1, 1).double() * x.double() + cx[:, 2].view(1, CX, 1, 1).double()
        T_op, mask_op = ops.Op(d(x), 3, d(cx)), ops.Op(d(x), 2, d(cx))
    else:
        xcoef, t = None, x.double()
        resid = d(torch.randn(B, CX, H, W, generator=g))
        q = d(torch.randn(B, CX, H, W, generator=g)) if form == "res" else None
        T_op, mask_op = ops.Op(d(x), 1), ops.Op(d(x))
    dst = torch.zeros(CD, CX, 3, 3, device=DEV)
    dx, st = ops.conv3x3_bwd_fused(dy_op, d(x), xcoef, d(w), dst, B, CD, resid=resid, q=q, want_stats=form != "res_noq")
    # float64 truth through autograd
    t_in = t.clamp(min=0).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    F.conv2d(t_in, w64, padding=1).backward(da)
    dx_ref = t_in.grad * (t > 0) + (resid.cpu().double() if resid is not None else 0.0)
    near = t.abs() < 1e-5
    scale = float(dx_ref.abs().max())
    assert float(((dx.cpu().double() - dx_ref).abs() * ~near).max()) <= 3e-6 * scale
    close(dst, w64.grad.float(), 1e-5, 3e-5 * float(w64.grad.abs().max()), "weight gradient vs float64")
    # the two kernels it replaces
    dst2 = torch.zeros(CD, CX, 3, 3, device=DEV)
    ops.wgrad(dy_op, T_op, dst2, B, CD, CX, H, W, 3)
    dx2, st2 = ops.conv3x3(dy_op, ops.weight_view(d(w), 9, CX * 9, -3, -1, off=8), B, CD, CX, H, W, taps=9,
                           want_stats=form != "res_noq", like=d(gy), mask=mask_op, resid=resid, stat_q=q)
    assert float((dx - dx2).abs().max()) <= 3e-6 * scale
    close(dst, dst2, 1e-5, 3e-5 * float(w64.grad.abs().max()), "weight gradient vs dm_wgrad")
    if form == "res_noq":
        assert st is None
    else:
        qq = q.cpu().double()
        want1, want2 = dx.cpu().double().sum((0, 2, 3)), (dx.cpu().double() * qq).sum((0, 2, 3))
        close(st.sum(0)[:, 0].cpu(), want1, 1e-6, 1e-6 * float(dx_ref.abs().sum((0, 2, 3)).max()), "sum dx")
        close(st.sum(0)[:, 1].cpu(), want2, 1e-6, 1e-6 * float((dx_ref.abs() * qq.abs()).sum((0, 2, 3)).max()), "sum dx * q")
        close(st.sum(0), st2.sum(0), 1e-9, 1e-6 * float(dx_ref.abs().sum((0, 2, 3)).max()), "statistics vs dm_conv3x3")
    # bit-reproducible
    dst3 = torch.zeros(CD, CX, 3, 3, device=DEV)
    dx3, st3 = ops.conv3x3_bwd_fused(dy_op, d(x), xcoef, d(w), dst3, B, CD, resid=resid, q=q, want_stats=form != "res_noq")
    assert torch.equal(dx3, dx) and torch.equal(dst3, dst) and (st is None or torch.equal(st3, st))
    assert ops.conv3x3_bwd_fused_supported(32, 16, 32, 32) and not ops.conv3x3_bwd_fused_supported(32, 16, 32, 64)
    assert not ops.conv3x3_bwd_fused_supported(16, 16, 32, 32)
    assert not ops.conv3x3_bwd_fused_supported(64, 64, 16, 16)


@pytest.mark.parametrize("B,two", [(3, True), (70, True), (300, True), (2, False)])
def test_conv4x4s2_backward_fused_equals_the_two_kernels(ops, B, two):
    """dm_conv4x4s2_bwd_fused (data + weight gradient of enc.7 from one staging of the patch) against dm_conv3x3 (pixel
    shuffle) + dm_wgrad and against autograd's conv2d backward in float64."""
    C, H = 16, 16
    g = torch.Generator().manual_seed(B * 5 + 1)
    gy, y = torch.randn(B, C, H, H, generator=g), torch.randn(B, C, H, H, generator=g)
    x = torch.randn(B, C, 2 * H, 2 * H, generator=g)
    w = torch.randn(C, C, 4, 4, generator=g) * 0.2
    cd = torch.randn(C, 4, generator=g) * 0.5
    cx = torch.zeros(C, 4)
    cx[:, 0] = torch.rand(C, generator=g) + 0.5
    cx[:, 2] = torch.randn(C, generator=g) * 0.3
    d = lambda t: t.to(DEV)
    dy_op = ops.Op(d(gy), 4, d(cd), p1=d(y)) if two else ops.Op(d(gy))
    da = (cd[:, 0].view(1, C, 1, 1).double() * gy.double() + cd[:, 1].view(1, C, 1, 1).double() * y.double()
          + cd[:, 2].view(1, C, 1, 1).double()) if two else gy.double()
    t = cx[:, 0].view(1, C, 1, 1).double() * x.double() + cx[:, 2].view(1, C, 1, 1).double()
    dst = torch.zeros(C, C, 4, 4, device=DEV)
    dx, st = ops.conv4x4s2_bwd_fused(dy_op, d(x), d(cx), d(w), dst, B)
    t_in = t.clamp(min=0).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    F.conv2d(t_in, w64, stride=2, padding=1).backward(da)
    dx_ref = t_in.grad * (t > 0)
    near = t.abs() < 1e-5
    scale = float(dx_ref.abs().max())
    assert float(((dx.cpu().double() - dx_ref).abs() * ~near).max()) <= 3e-6 * scale
    close(dst, w64.grad.float(), 1e-5, 3e-5 * float(w64.grad.abs().max()), "weight gradient vs float64")
    dst2 = torch.zeros(C, C, 4, 4, device=DEV)
    ops.wgrad(dy_op, ops.Op(d(x), 3, d(cx)), dst2, B, C, C, H, H, 4)
    dx2, st2 = ops.conv3x3(dy_op, ops.weight_view(d(w), 16, C * 16, 4, 1), B, C, 4 * C, H, H, taps=9, pixel_shuffle=True,
                           want_stats=True, like=d(gy), mask=ops.Op(d(x), 2, d(cx)), stat_q=d(x))
    assert float((dx - dx2).abs().max()) <= 3e-6 * scale
    close(dst, dst2, 1e-5, 3e-5 * float(w64.grad.abs().max()), "weight gradient vs dm_wgrad")
    want1, want2 = dx.cpu().double().sum((0, 2, 3)), (dx.cpu().double() * x.double()).sum((0, 2, 3))
    close(st.sum(0)[:, 0].cpu(), want1, 1e-6, 1e-6 * float(dx_ref.abs().sum((0, 2, 3)).max()), "sum dx")
    close(st.sum(0)[:, 1].cpu(), want2, 1e-6, 1e-6 * float((dx_ref.abs() * x.double().abs()).sum((0, 2, 3)).max()), "sum dx * x")
    close(st.sum(0), st2.sum(0), 1e-9, 1e-6 * float(dx_ref.abs().sum((0, 2, 3)).max()), "statistics vs dm_conv3x3")
    dst3 = torch.zeros(C, C, 4, 4, device=DEV)
    dx3, st3 = ops.conv4x4s2_bwd_fused(dy_op, d(x), d(cx), d(w), dst3, B)
    assert torch.equal(dx3, dx) and torch.equal(dst3, dst) and torch.equal(st3, st)
    assert not ops.conv4x4s2_bwd_fused_supported(16, 8, 32, 32)


@pytest.mark.parametrize("B,CI,CO,H,W,mask", [(3, 8, 4, 32, 32, True), (70, 8, 4, 32, 32, True), (2, 8, 4, 64, 64, True),
                                             (5, 16, 8, 16, 16, False), (130, 16, 8, 16, 16, False), (2, 16, 8, 32, 32, False),
                                             (2, 16, 8, 8, 48, True)])
def test_conv_transpose_backward_fused_equals_the_two_kernels(ops, B, CI, CO, H, W, mask):
    """dm_convt_bwd_fused (input + weight gradient of dec.0 / dec.2 from one staging) against dm_conv4x4s2 + dm_wgrad and
    against autograd's conv_transpose2d backward in float64."""
    g = torch.Generator().manual_seed(B + CI + H)
    S = torch.randn(B, CI, H, W, generator=g)
    if mask:
        S = S.clamp(min=0)                                   # the forward stored relu(.)
    G = torch.randn(B, CO, 2 * H, 2 * W, generator=g)
    w = torch.randn(CI, CO, 4, 4, generator=g) * 0.2
    d = lambda t: t.to(DEV)
    dst = torch.zeros(CI, CO, 4, 4, device=DEV)
    gin, st = ops.convT_bwd_fused(d(S), d(G), d(w), dst, mask_relu=mask, want_stats=True)
    # float64 truth through autograd
    S64, w64 = S.double().requires_grad_(True), w.double().requires_grad_(True)
    out = F.conv_transpose2d(S64, w64, stride=2, padding=1)
    out.backward(G.double())
    gin_ref = S64.grad * (S.double() > 0) if mask else S64.grad
    assert float((gin.cpu().double() - gin_ref).abs().max()) <= 3e-6 * float(gin_ref.abs().max())
    close(dst, w64.grad.float(), 1e-5, 3e-5 * float(w64.grad.abs().max()), "weight gradient vs float64")
    close(st.sum(0)[:, 0].cpu(), gin.cpu().double().sum((0, 2, 3)), 1e-6, 1e-6 * float(gin_ref.abs().sum((0, 2, 3)).max()), "channel sums")
    # the two kernels it replaces
    dst2 = torch.zeros(CI, CO, 4, 4, device=DEV)
    ops.wgrad(ops.Op(d(S)), ops.Op(d(G)), dst2, B, CI, CO, H, W, 4)
    gin2, st2 = ops.conv4x4s2(ops.Op(d(G)), ops.weight_view(d(w), CO * 16, 16, 4, 1), B, CO, CI, 2 * H, 2 * W, want_stats=True,
                              **({"mask": ops.Op(d(S))} if mask else {}))
    assert float((gin - gin2).abs().max()) <= 3e-6 * float(gin_ref.abs().max())
    close(dst, dst2, 1e-5, 3e-5 * float(w64.grad.abs().max()), "weight gradient vs dm_wgrad")
    close(st.sum(0)[:, 0], st2.sum(0)[:, 0], 1e-9, 1e-7 * float(gin_ref.abs().sum((0, 2, 3)).max()), "channel sums vs dm_conv4x4s2")
    # bit-reproducible
    dst3 = torch.zeros(CI, CO, 4, 4, device=DEV)
    gin3, st3 = ops.convT_bwd_fused(d(S), d(G), d(w), dst3, mask_relu=mask, want_stats=True)
    assert torch.equal(gin3, gin) and torch.equal(dst3, dst) and torch.equal(st3, st)
    gin4, st4 = ops.convT_bwd_fused(d(S), d(G), d(w), dst3, mask_relu=mask)          # without the sums
    assert st4 is None and torch.equal(gin4, gin)
    assert not ops.convT_bwd_fused_supported(8, 4, 32, 16) and not ops.convT_bwd_fused_supported(4, 4, 64, 64)


@pytest.mark.parametrize("cs,ct,k,hs,ones,B", [
    (8, 3, 4, 64, True, 3), (16, 8, 4, 32, False, 3), (16, 16, 4, 16, False, 5), (16, 16, 3, 16, False, 5),
    (32, 16, 3, 16, False, 5), (16, 32, 1, 16, False, 5), (16, 8, 4, 16, False, 5), (8, 4, 4, 32, False, 3),
    (4, 4, 4, 64, False, 3), (8, 5, 4, 64, True, 2), (16, 16, 4, 32, False, 2), (16, 8, 4, 64, False, 2), (8, 3, 4, 64, True, 70)])
def test_wgrad(ops, cs, ct, k, hs, ones, B):
    s, p = (2, 1) if k == 4 else ((1, 1) if k == 3 else (1, 0))
    ht = hs * s
    ctp = ct - (1 if ones else 0)
    S = rnd(B, cs, hs, hs, seed=1)
    T = rnd(B, ctp, ht, ht, seed=2)
    Tin = torch.cat([T, torch.ones(B, 1, ht, ht)], 1) if ones else T
    w = torch.zeros(cs, ct, k, k, requires_grad=True)
    F.conv2d(Tin, w, None, stride=s, padding=p).backward(S)
    dst = torch.empty(cs, ct, k, k, device=DEV)
    ops.wgrad(ops.Op(S.to(DEV)), ops.Op(T.to(DEV), ones=ones), dst, B, cs, ct, hs, hs, k)
    scale = w.grad.abs().max().item()
    close(dst, w.grad, 2e-5, 2e-5 * scale, "wgrad")


def test_wgrad_operand_modes_and_determinism(ops):
    B, cs, ct, h = 4, 16, 16, 16
    dy, a = rnd(B, cs, h, h, seed=1), rnd(B, cs, h, h, seed=2)
    coef = torch.stack([rnd(cs, seed=3), rnd(cs, seed=4) * 0.1, rnd(cs, seed=5) * 0.1, torch.zeros(cs)], 1)
    t = rnd(B, ct, 2 * h, 2 * h, seed=6)
    tcoef = torch.stack([rnd(ct, seed=7), torch.zeros(ct), rnd(ct, seed=8) * 0.2, torch.zeros(ct)], 1)
    w = torch.zeros(cs, ct, 4, 4, requires_grad=True)
    F.conv2d(load_ref(t, 3, tcoef), w, None, stride=2, padding=1).backward(load_ref(dy, 4, coef, a))
    outs = []
    for _ in range(2):
        dst = torch.empty(cs, ct, 4, 4, device=DEV)
        ops.wgrad(ops.Op(dy.to(DEV), 4, coef.to(DEV), p1=a.to(DEV)), ops.Op(t.to(DEV), 3, tcoef.to(DEV)), dst, B, cs, ct, h, h, 4)
        outs.append(dst.cpu())
    close(outs[0], w.grad, 3e-5, 3e-5 * w.grad.abs().max().item(), "wgrad modes")
    assert torch.equal(outs[0], outs[1]), "slab reduction must be bitwise reproducible"


# ============================================================================ BatchNorm
def test_bn_finalize_and_backward(ops):
    B, Cn, h = 4, 16, 16
    a = rnd(B, Cn, h, h, seed=1) * 2 + 0.7
    bn = torch.nn.BatchNorm2d(Cn)
    with torch.no_grad():
        bn.weight.copy_(rnd(Cn, seed=2).abs() + 0.5)
        bn.bias.copy_(rnd(Cn, seed=3))
    a_ref = a.clone().requires_grad_(True)
    y_ref = bn(a_ref)
    dy = rnd(B, Cn, h, h, seed=4)
    y_ref.backward(dy)

    stats = ops.channel_stats(a.to(DEV))
    rm, rv = torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    coef, saved = ops.bn_finalize(stats, B * h * h, bn.weight.detach().to(DEV), bn.bias.detach().to(DEV), rm, rv, nbt, 0.1, 1e-5)
    y = ops.apply(ops.Op(a.to(DEV), 2, coef), B, Cn, h, h)
    close(y, y_ref, 1e-5, 1e-5, "bn apply")
    close(rm, bn.running_mean, 1e-6, 1e-7, "running_mean")
    close(rv, bn.running_var, 1e-6, 1e-7, "running_var")
    assert int(nbt) == 1
    st2 = ops.channel_stats(dy.to(DEV), a.to(DEV))
    dgamma, dbeta = torch.empty(Cn, device=DEV), torch.empty(Cn, device=DEV)
    cb = ops.bn_backward_finalize(st2, B * h * h, bn.weight.detach().to(DEV), saved, dgamma, dbeta)
    da = ops.apply(ops.Op(dy.to(DEV), 4, cb, p1=a.to(DEV)), B, Cn, h, h)
    close(da, a_ref.grad, 1e-4, 2e-6, "bn backward dx")
    close(dgamma, bn.weight.grad, 1e-5, 1e-4, "dgamma")
    close(dbeta, bn.bias.grad, 1e-5, 1e-4, "dbeta")
    # the same outputs against float64 BatchNorm and the derived bound (tests/helpers/glue_reference.py): the hand-picked
    # tolerances above and the bound are seen to agree on this shape
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import glue_reference as G
    ref = G.bn_apply_chain_ref(a, dy, bn.weight.detach(), bn.bias.detach(), 1e-5)
    for name, got in (("y", y), ("da", da), ("dgamma", dgamma), ("dbeta", dbeta)):
        err = (got.cpu().double().reshape(ref[name].shape) - ref[name]).abs()
        print(f"bn {name}: worst error / derived bound {float((err / ref['b_' + name]).max()):.3f}")
        assert bool((err <= ref["b_" + name]).all()), f"bn {name}: {float((err / ref['b_' + name]).max()):.2f} derived bounds"


def test_bn_per_sample_statistics(ops):
    B, Cn, h = 3, 8, 16
    a = rnd(B, Cn, h, h, seed=1) + 0.3
    bn = torch.nn.BatchNorm2d(Cn)
    ys = torch.cat([bn(a[i:i + 1]) for i in range(B)], 0)
    stats = torch.cat([ops.channel_stats(a[i:i + 1].to(DEV)) for i in range(B)], 0)      # one slab per sample
    rm, rv = torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    g, b = torch.ones(Cn, device=DEV), torch.zeros(Cn, device=DEV)
    coef, saved = ops.bn_finalize(stats, h * h, g, b, rm, rv, nbt, 0.1, 1e-5, per_sample=True, slabs_per_group=1)
    y = ops.apply(ops.Op(a.to(DEV), 2, coef, per_sample=True), B, Cn, h, h)
    close(y, ys, 1e-5, 1e-5, "per-sample bn")
    close(rm, bn.running_mean, 1e-5, 1e-7, "running_mean")
    close(rv, bn.running_var, 1e-5, 1e-7, "running_var")
    assert int(nbt) == B
    # the same with the running statistics deferred: two layers brought up to date by ONE later launch, bit for bit
    rm2, rv2 = torch.zeros(Cn, device=DEV), torch.ones(Cn, device=DEV)
    rm3, rv3 = torch.full((Cn,), 0.5, device=DEV), torch.full((Cn,), 2.0, device=DEV)
    nbt2, nbt3 = torch.zeros((), dtype=torch.int64, device=DEV), torch.full((), 7, dtype=torch.int64, device=DEV)
    rm3_ref, rv3_ref, nbt3_ref = rm3.clone(), rv3.clone(), nbt3.clone()
    ops.bn_finalize(stats, h * h, g, b, rm3_ref, rv3_ref, nbt3_ref, 0.25, 1e-5, per_sample=True, slabs_per_group=1)
    deferred = []
    coef2, saved2 = ops.bn_finalize(stats, h * h, g, b, rm2, rv2, nbt2, 0.1, 1e-5, per_sample=True, slabs_per_group=1, defer=deferred)
    ops.bn_finalize(stats, h * h, g, b, rm3, rv3, nbt3, 0.25, 1e-5, per_sample=True, slabs_per_group=1, defer=deferred)
    assert torch.equal(coef2, coef) and torch.equal(saved2, saved)
    assert float(rm2.abs().sum()) == 0.0 and int(nbt2) == 0 and len(deferred) == 2         # untouched so far
    ops.bn_running_replay(deferred)
    assert torch.equal(rm2, rm) and torch.equal(rv2, rv) and int(nbt2) == B
    assert torch.equal(rm3, rm3_ref) and torch.equal(rv3, rv3_ref) and int(nbt3) == 7 + B and not deferred


# ================================================================================= head
@pytest.mark.parametrize("nin,masked", [(2, False), (2, True), (4, True), (1, False)])
def test_head_forward_backward(ops, nin, masked):
    B, c4, h = 2, 4, 64
    d4 = rnd(B, c4, h, h, seed=1).clamp(min=0)
    w6 = rnd(nin, c4, 1, 1, seed=2).requires_grad_(True)
    b6 = rnd(nin, seed=3).requires_grad_(True)
    x = rnd(B, nin, h, h, seed=4)
    mask = (torch.rand(B, 1, h, h, generator=torch.Generator().manual_seed(5)) > 0.4).float() * 0.5 + 0.5 if masked else None
    var = torch.linspace(0.5, 1.5, nin)
    d4r = d4.clone().requires_grad_(True)
    dec_ref = F.conv2d(F.relu(d4r), w6, b6)
    m = mask if masked else torch.ones_like(x)
    loss_ref = torch.mean(F.mse_loss(dec_ref * m, x * m, reduction="none") / var.reshape(1, nin, 1, 1))
    (loss_ref * 1.3).backward()

    dv = [t.detach().to(DEV) for t in (d4, w6, b6, x, var)]
    mk = mask.to(DEV) if masked else None
    dec, slabs = ops.head_forward(dv[0], dv[1], dv[2], dv[3], mk, dv[4])
    recon = ops.loss_finalize(slabs, x.numel(), torch.zeros(2, device=DEV), 1.0, 0.0)[0]
    close(dec, dec_ref, 1e-5, 1e-5, "decoded")
    assert abs(float(recon) - float(loss_ref)) <= 2e-6 * abs(float(loss_ref))
    g4, part = ops.head_backward(dec, dv[3], mk, dv[4], dv[0], dv[1], torch.tensor([1.3], device=DEV))
    flat = torch.empty(part.shape[1], device=DEV)
    ops.sum_slabs(part, flat)
    close(g4, d4r.grad, 1e-4, 1e-9, "g4")
    close(flat[:nin * c4].reshape(nin, c4), w6.grad.reshape(nin, c4), 1e-4, 1e-7, "dW6")
    close(flat[nin * c4:nin * c4 + nin], b6.grad, 1e-4, 1e-7, "db6")
    close(flat[nin * c4 + nin:], d4r.grad.sum((0, 2, 3)), 1e-4, 1e-7, "sum g4")


# ============================================================== composition / Adam / misc
def test_e1_compose_and_chain(ops):
    nin, c0, c1, B, h = 2, 8, 8, 2, 32
    w0 = rnd(c0, nin, 1, 1, seed=1).requires_grad_(True)
    b0 = rnd(c0, seed=2).requires_grad_(True)
    w1 = rnd(c1, c0, 4, 4, seed=3, scale=0.2).requires_grad_(True)
    x = rnd(B, nin, h, h, seed=4)
    ref = F.conv2d(F.conv2d(x, w0, b0), w1, None, stride=2, padding=1)
    weff = ops.e1_compose(w0.detach().to(DEV), b0.detach().to(DEV), w1.detach().to(DEV))
    xin = torch.cat([x, torch.ones(B, 1, h, h)], 1)
    close(F.conv2d(xin, weff.cpu(), None, stride=2, padding=1), ref, 1e-5, 1e-5, "composite conv")
    g = rnd(*ref.shape, seed=5)
    ref.backward(g)
    wz = torch.zeros(c1, nin + 1, 4, 4, requires_grad=True)
    F.conv2d(xin, wz, None, stride=2, padding=1).backward(g)
    dw0, db0, dw1 = torch.empty(c0, nin, 1, 1, device=DEV), torch.empty(c0, device=DEV), torch.empty(c1, c0, 4, 4, device=DEV)
    ops.e1_chain(wz.grad.to(DEV), w0.detach().to(DEV), b0.detach().to(DEV), w1.detach().to(DEV), dw0, db0, dw1)
    close(dw0, w0.grad, 1e-4, 1e-4, "dw0")
    close(db0, b0.grad, 1e-4, 1e-4, "db0")
    close(dw1, w1.grad, 1e-4, 1e-4, "dw1")


def test_adam_matches_torch(ops):
    n = 5000
    p0 = rnd(n, seed=1)
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=1e-4, betas=(.9, .999))
    p = p0.clone().to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step = torch.zeros(1, device=DEV)
    for s in range(3):
        g = rnd(n, seed=10 + s) * (10.0 ** (s - 3))
        p_ref.grad = g.clone()
        opt.step()
        step += 1
        ops.adam(p, g.to(DEV), m, v, 1e-4, 0.9, 0.999, 1e-8, step)
    close(p, p_ref, 1e-6, 1e-7, "adam")


def test_adam_counted_keeps_its_own_step(ops):
    """dm_adam_counted: same update as dm_adam, the step count lives in two ping-ponged device words."""
    n = 3000
    p0 = rnd(n, seed=2)
    pa, pb = p0.clone().to(DEV), p0.clone().to(DEV)
    ma, va = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    mb, vb = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step = torch.zeros(1, device=DEV)
    cnt = torch.zeros(2, device=DEV)
    for s in range(4):
        g = (rnd(n, seed=20 + s) * 0.1).to(DEV)
        step += 1
        ops.adam(pa, g, ma, va, 1e-3, 0.9, 0.999, 1e-8, step)
        a, b = s % 2, 1 - s % 2
        ops.adam_counted(pb, g, mb, vb, 1e-3, 0.9, 0.999, 1e-8, cnt[a:a + 1], cnt[b:b + 1])
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert float(cnt[0]) == 4.0                            # four completed steps, last written to word 0


def test_vq_backward_slabs_equal_the_atomic_form(ops):
    """The codebook gradient as per-workgroup slabs (no global float atomics, nothing to zero) sums to the atomic
    result (inside a workgroup the LDS adds still come in arrival order, so bits may differ run to run)."""
    B, D, K, H = 70, 16, 64, 16
    z = rnd(B, D, H, H, seed=31).to(DEV)
    cb = rnd(K, D, seed=32).to(DEV)
    g = rnd(B, D, H, H, seed=33).to(DEV)
    idx, _, _, _ = ops.vq_forward(z, cb, want_out=False)
    gl = torch.tensor([0.7], device=DEV)
    dz_a, dw_a = ops.vq_backward(z, cb, idx, g, gl, 0.25, dw=torch.zeros(K, D, device=DEV))
    dz_s, slabs = ops.vq_backward_slabs(z, cb, idx, g, gl, 0.25)
    dw_s = torch.empty(K * D, device=DEV)
    ops.reduce_slabs(slabs, dw_s)
    assert torch.equal(dz_a, dz_s)
    close(dw_s.reshape(K, D), dw_a, 1e-5, 1e-7 * float(dw_a.abs().max()) + 1e-9, "codebook gradient (slabs)")


@pytest.mark.parametrize("B,K,D,H", [(70, 64, 16, 16), (9, 64, 32, 8), (5, 64, 64, 16), (3, 10, 16, 8), (37, 33, 32, 16),
                                     (2048, 64, 16, 16)])
def test_vq_backward_one_hot_product_is_ordered(ops, B, K, D, H):
    """Codebooks of at most 64 codes: the slab form accumulates the codebook gradient on the matrix cores in a fixed
    order (no float atomics, LDS or global), so two runs agree to the bit; values against embedding_dense_backward /
    mse_loss_backward restated with index_add in double."""
    z = rnd(B, D, H, H, seed=61)
    cb = rnd(K, D, seed=62)
    g = rnd(B, D, H, H, seed=63)
    zd, cbd, gd = z.to(DEV), cb.to(DEV), g.to(DEV)
    idx, _, _, _ = ops.vq_forward(zd, cbd, want_out=False)
    gl = torch.tensor([1.3], device=DEV)
    q = cb[idx.cpu()].permute(0, 3, 1, 2)
    N = z.numel()
    dz_ref = g + 1.3 * 2 * 0.25 * (z - q) / N
    dw_ref = torch.zeros(K, D, dtype=torch.float64).index_add_(
        0, idx.cpu().reshape(-1), (1.3 * 2 * (q.double() - z.double()) / N).permute(0, 2, 3, 1).reshape(-1, D))
    dz_1, slabs_1 = ops.vq_backward_slabs(zd, cbd, idx, gd, gl, 0.25)
    dz_2, slabs_2 = ops.vq_backward_slabs(zd, cbd, idx, gd, gl, 0.25)
    assert torch.equal(slabs_1, slabs_2) and torch.equal(dz_1, dz_2)
    dw = ops.reduce_slabs(slabs_1, torch.empty_like(cbd))
    close(dz_1, dz_ref, 1e-6, 1e-9, "dz")
    close(dw, dw_ref.float(), 1e-5, 1e-6 * float(dw_ref.abs().max()), "codebook gradient (one-hot product)")
    dz_a, dw_a = ops.vq_backward(zd, cbd, idx, gd, gl, 0.25, dw=torch.zeros(K, D, device=DEV))
    assert torch.equal(dz_a, dz_1)                             # same expression as the windowed kernel
    # no upstream gradient / no dz wanted
    dz_0, slabs_0 = ops.vq_backward_slabs(zd, cbd, idx, None, gl, 0.25)
    close(dz_0, 1.3 * 2 * 0.25 * (z - q) / N, 1e-5, 1e-12, "dz without g_out")
    none, slabs_n = ops.vq_backward_slabs(zd, cbd, idx, gd, None, 0.25, want_dz=False)
    assert none is None
    close(ops.reduce_slabs(slabs_n, torch.empty_like(cbd)), (dw_ref / 1.3).float(), 1e-5, 1e-6 * float(dw_ref.abs().max()), "dw, g_loss 1")


@pytest.mark.parametrize("K,D,H", [(512, 64, 32), (4096, 16, 32), (300, 128, 8),
                                   # widths without an instantiation: vq_backward_any_kernel (run-time embedding_dim)
                                   (64, 12, 8), (100, 24, 16), (64, 48, 8), (40, 96, 8), (7, 5, 4)])
def test_vq_backward_large_codebooks(ops, K, D, H):
    """Codebooks above the LDS window (config_example.yml: 512 x 64; the stress case: 4096 x 16) go through windows
    of codes; both forms against embedding_dense_backward / mse_loss_backward restated with index_add."""
    B = 5
    z = rnd(B, D, H, H, seed=51)
    cb = rnd(K, D, seed=52)
    g = rnd(B, D, H, H, seed=53)
    zd, cbd = z.to(DEV), cb.to(DEV)
    idx, _, _, _ = ops.vq_forward(zd, cbd, want_out=False)
    gl = torch.tensor([1.3], device=DEV)
    q = cb[idx.cpu()].permute(0, 3, 1, 2)
    N = z.numel()
    dz_ref = g + 1.3 * 2 * 0.25 * (z - q) / N
    dw_ref = torch.zeros(K, D).index_add_(0, idx.cpu().reshape(-1), (1.3 * 2 * (q - z) / N).permute(0, 2, 3, 1).reshape(-1, D))
    dz_a, dw_a = ops.vq_backward(zd, cbd, idx, g.to(DEV), gl, 0.25, dw=torch.zeros(K, D, device=DEV))
    dz_s, dw_s = ops.vq_backward(zd, cbd, idx, g.to(DEV), gl, 0.25)
    close(dz_a, dz_ref, 1e-6, 1e-9, "dz")
    assert torch.equal(dz_a, dz_s)
    tol = 1e-6 * float(dw_ref.abs().max())
    for name, got in (("atomics", dw_a), ("slabs", dw_s)):
        err = (got.cpu().double() - dw_ref.double()).abs()
        off = (err > tol + 1e-5 * dw_ref.double().abs()).reshape(-1).nonzero().reshape(-1)
        if off.numel():
            # (round 4: this check failed ONCE in a full-suite run -- 1008 elements of the atomic form, never again in 400
            # repetitions of the two calls on their own, tools/exp/vq_bwd_flake.py -- so a failure says where and how much)
            rows = torch.unique(off // D)
            print(f"{name}: {off.numel()} elements off in {rows.numel()} codes (first {rows[:8].tolist()}), flat index "
                  f"{int(off.min())}..{int(off.max())}, max err {float(err.max()):.3e}; the other form's max err "
                  f"{float((dw_s if name == 'atomics' else dw_a).cpu().double().sub(dw_ref.double()).abs().max()):.3e}; "
                  f"idx still equal to its host copy: {bool(torch.equal(idx.cpu(), idx.cpu()))}")
    close(dw_a, dw_ref, 1e-5, tol, "codebook gradient (atomics)")
    close(dw_s, dw_ref, 1e-5, tol, "codebook gradient (slabs)")


def test_vq_backward_atomic_form_repeated_behind_its_neighbours(ops):
    """Round 4 saw test_vq_backward_large_codebooks[512-64-32] fail ONCE (atomic form: 1 008 of 32 768 floats -- 4 KiB minus
    64 B -- off by ~4e-5, the magnitude of the 4 KiB codebook gradients the previous test leaves in the allocator's pool).
    The pair of calls behind the calls of the tests that run before it, repeated; every workgroup's partial sum is known on
    the host, so a failure says whether a flush was lost / doubled (kernel logic: whole 64-float rows) or whether the region
    is page-shaped (stale memory under the zero fill).  Round 5: 1 000 repetitions of this in three allocation patterns
    (tools/exp/vq_bwd_flake2.py, vq_bwd_flake3.py) without a mismatch."""
    K, D, H, B = 512, 64, 32, 5
    z, cb, g = rnd(B, D, H, H, seed=51), rnd(K, D, seed=52), rnd(B, D, H, H, seed=53)
    zd, cbd, gd = z.to(DEV), cb.to(DEV), g.to(DEV)
    idx, _, _, _ = ops.vq_forward(zd, cbd, want_out=False)
    gl = torch.tensor([1.3], device=DEV)
    ih = idx.cpu().reshape(-1)
    contrib = 1.3 * 2 * (cb[ih].double() - z.permute(0, 2, 3, 1).reshape(-1, D).double()) / z.numel()
    part = torch.zeros(5, K, D, dtype=torch.float64)            # the kernel's five workgroups take 1024 positions each
    for w in range(5):
        part[w].index_add_(0, ih[w * 1024:(w + 1) * 1024], contrib[w * 1024:(w + 1) * 1024])
    ref = part.sum(0)
    tol = 1e-5 * ref.abs() + 1e-6 * float(ref.abs().max())
    # the neighbours' device-side allocation pattern: a large batch through the 64-code forms (4 KiB gradients, slabs)
    zb, cbb = rnd(2048, 16, 16, 16, seed=61).to(DEV), rnd(64, 16, seed=62).to(DEV)
    gb = rnd(2048, 16, 16, 16, seed=63).to(DEV)
    idxb, _, _, _ = ops.vq_forward(zb, cbb, want_out=False)
    for it in range(40):
        _, small = ops.vq_backward(zb, cbb, idxb, gb, gl, 0.25, dw=torch.zeros(64, 16, device=DEV))
        _, slabs = ops.vq_backward_slabs(zb, cbb, idxb, gb, gl, 0.25)
        keep = ops.reduce_slabs(slabs, torch.empty_like(cbb))
        del small, slabs, keep
        dw0 = torch.zeros(K, D, device=DEV)
        ptr = dw0.data_ptr()
        _, dw_a = ops.vq_backward(zd, cbd, idx, gd, gl, 0.25, dw=dw0)
        _, dw_s = ops.vq_backward(zd, cbd, idx, gd, gl, 0.25)
        for name, got in (("atomic", dw_a), ("slab", dw_s)):
            dd = got.cpu().double() - ref
            ww = dd.abs() > tol
            if bool(ww.any()):
                flat = ww.reshape(-1).nonzero().reshape(-1)
                who = [f"workgroup {w} {what}" for w in range(5) for sign, what in ((-1.0, "lost"), (1.0, "doubled"))
                       if float((dd - sign * part[w])[ww].abs().max()) <= 1e-9]
                raise AssertionError(
                    f"iteration {it}, {name} form: {flat.numel()} floats off, flat {int(flat.min())}..{int(flat.max())}, "
                    f"{torch.unique(flat // 16).numel()} 64-byte lines, first at byte {(ptr + 4 * int(flat.min())) % 4096} of its 4 KiB "
                    f"page, max err {float(dd.abs().max()):.3e}; explained by a workgroup's partial sum: {who or 'no'}")


@pytest.mark.parametrize("B,n", [(4, 4096), (19, 4096), (33, 100), (1, 64)])
def test_pair_msd_forward_backward(ops, B, n):
    """Pairwise mean-squared latent distance of the time-matching loss (vq_vae.py:327-329) and its gradient."""
    z = rnd(B, n, seed=41).requires_grad_(True)
    sim_ref = torch.pow(z.reshape((1, -1, n)) - z.reshape((-1, 1, n)), 2).mean(2)
    g = rnd(B, B, seed=42)
    (sim_ref * g).sum().backward()
    zd = z.detach().to(DEV)
    sim = ops.pair_msd(zd)
    close(sim, sim_ref, 2e-6, 1e-7, "sim_mat")
    dz = ops.pair_msd_backward(zd, g.to(DEV))
    close(dz, z.grad, 2e-5, 2e-6 * float(z.grad.abs().max()) + 1e-12, "d sim / d z")


@pytest.mark.parametrize("B,n,mode", [(4, 4096, 0), (4, 4096, 1), (70, 1024, 1), (129, 64, 0), (33, 16384, 1)])
def test_time_matching_fused_forward_backward(ops, B, n, mode):
    """The whole pairwise term on the MFMA (Gram form, loss epilogue, second GEMM for the gradient) against the reference's
    expressions in float64: vq_vae.py:324-332 (mode 0), vae.py:322-336 (mode 1: weights, hinge on the non-related pairs, mean)."""
    g = torch.Generator().manual_seed(B + n)
    z = torch.randn(B, n, generator=g) * 0.7 + 0.1
    tm = torch.randint(0, 3, (B, B), generator=g).float()
    w_a, w_t, w_n, margin = 1.1, 0.1, -0.5, 0.5
    zr = z.double().requires_grad_(True)
    sim = (zr.reshape(1, B, n) - zr.reshape(B, 1, n)).pow(2).mean(2)
    if mode == 0:
        ref = (sim * tm.double()).sum()
    else:
        wts = tm.double().clone()
        wts[tm == 2], wts[tm == 1], wts[tm == 0] = w_a, w_t, w_n
        val = sim * wts
        val = torch.where(tm == 0, torch.clamp(val + margin, min=0), val)
        ref = val.mean()
    ref.backward()
    zd = z.to(DEV)
    loss, S = ops.time_matching_forward(zd, tm.to(DEV), mode, w_a, w_t, w_n, margin)
    assert abs(float(loss) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), (float(loss), float(ref))
    gl = torch.full((1,), 0.75, device=DEV)
    dz = ops.time_matching_backward(zd, S, gl, 2.0).cpu().double()
    want = zr.grad * 1.5
    assert (dz - want).abs().max() <= 2e-5 * want.abs().max() + 1e-9, float((dz - want).abs().max())
    # the module-level entry takes the same path
    from dynamorph_amd.vq_vae import time_matching_loss
    za = zd.clone().requires_grad_(True)
    l2 = time_matching_loss(za, tm.to(DEV), mode == 1, w_a, w_t, w_n, margin)
    l2.backward()
    assert abs(float(l2) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    assert (za.grad.cpu().double() - zr.grad).abs().max() <= 2e-5 * zr.grad.abs().max() + 1e-9


def _tm_reference(z, tm, mode, w_a=1.1, w_t=0.1, w_n=-0.5, margin=0.5):
    """vq_vae.py:324-332 (mode 0) / vae.py:322-336 (mode 1) in float64, differences first as the reference takes them."""
    B, n = z.shape
    zr = z.double().requires_grad_(True)
    sim = (zr.reshape(1, B, n) - zr.reshape(B, 1, n)).pow(2).mean(2)
    if mode == 0:
        ref = (sim * tm.double()).sum()
    else:
        wts = tm.double().clone()
        wts[tm == 2], wts[tm == 1], wts[tm == 0] = w_a, w_t, w_n
        val = sim * wts
        val = torch.where(tm == 0, torch.clamp(val + margin, min=0), val)
        ref = val.mean()
    ref.backward()
    return float(ref), zr.grad


@pytest.mark.parametrize("B,n", [(6, 4096), (70, 1024)])
def test_time_matching_folds_into_the_step(ops, B, n):
    """The two folds of the training step: dm_time_matching_backward_add (the pairwise term's gradient summed onto another
    gradient of the latents in the kernel's store) and dm_vq_loss_finalize_tm (the term's loss and the weighted total in
    the step's one scalar launch) against the separate launches they replace."""
    g = torch.Generator().manual_seed(B)
    z = (torch.randn(B, n, generator=g) * 0.5).to(DEV)
    tm = torch.randint(0, 3, (B, B), generator=g).float().to(DEV)
    other = torch.randn(B, n, generator=g).to(DEV)
    loss, S = ops.time_matching_forward(z, tm, 1, 1.1, 0.1, -0.5, 0.5)
    slabs, S2 = ops.time_matching_forward(z, tm, 1, 1.1, 0.1, -0.5, 0.5, want_slabs=True)
    assert torch.equal(S, S2)
    sep = other + ops.time_matching_backward(z, S, None, 0.7)
    fused = ops.time_matching_backward(z, S, None, 0.7, add=other)
    close(fused, sep, 1e-6, 1e-7 * float(sep.abs().max()), "gradient sum")      # (near pairs are added in another order)
    # scalars: a VQ call's state + reconstruction slabs + the pairwise slabs
    zq = torch.randn(4, 16, 16, 16, generator=g).to(DEV)
    cb = torch.randn(64, 16, generator=g).to(DEV)
    _, _, sse, ws = ops.vq_forward(zq, cb, want_hist=False)
    ls = torch.rand(8, dtype=torch.float64, device=DEV)
    four = ops.vq_loss_finalize(sse, ws, 64, 16, 4 * 256, 0.25, ls, 1000, 0.9, 1.1)
    five = ops.vq_loss_finalize_tm(sse, ws, 64, 16, 4 * 256, 0.25, ls, 1000, 0.9, 1.1, slabs, 0.005)
    assert torch.equal(five[:2], four[:2]) and torch.equal(five[3], four[3])
    assert abs(float(five[4]) - float(loss)) <= 1e-6 * abs(float(loss)) + 1e-12
    want_total = float(four[2]) + 0.005 * float(five[4])
    assert abs(float(five[2]) - want_total) <= 2e-7 * abs(want_total)


@pytest.mark.parametrize("B,n,mode,only_near", [(24, 4096, 0, True), (24, 4096, 0, False), (40, 4096, 1, False),
                                                (70, 1024, 0, True), (12, 65536, 0, True)])
def test_time_matching_related_pairs_lie_close_together(ops, B, n, mode, only_near):
    """The regime the term exists for: related pairs (tm in {1, 2}) are adjacent frames of ONE cell,
    |a - b|^2 << |a|^2, where the Gram form |a|^2 + |b|^2 - 2ab has cancelled -- and the example configuration multiplies
    the term by weight_matching = 100 (config_example.yml:164).  Latents come in groups: a base row, a copy at 1e-3
    relative distance, an EXACT duplicate, one at 10 % distance; tm marks pairs inside a group (only_near: nothing else,
    so loss and gradient consist of near pairs alone and are gated RELATIVE to themselves).  Loss and dz against the
    reference's expression (differences first) in float64."""
    g = torch.Generator().manual_seed(7 * B + n + mode)
    groups = B // 4
    base = torch.randn(groups, n, generator=g) * 0.7 + 0.1
    z = torch.randn(B, n, generator=g) * 0.7 + 0.1
    tm = torch.zeros(B, B)
    for q in range(groups):
        r = 4 * q
        z[r] = base[q]
        z[r + 1] = base[q] + 1e-3 * torch.randn(n, generator=g)
        z[r + 2] = base[q]
        z[r + 3] = base[q] + 0.07 * torch.randn(n, generator=g)
        for a in range(4):
            for b in range(4):
                if a != b:
                    tm[r + a, r + b] = 1.0 + ((a + b) % 2)
    if not only_near:
        far = torch.randint(0, 3, (B, B), generator=g).float()
        tm = torch.where(tm > 0, tm, far)
    wm = 100.0                                             # weight_matching of the example configuration
    ref, gref = _tm_reference(z, tm, mode)
    zd = z.to(DEV)
    loss, S = ops.time_matching_forward(zd, tm.to(DEV), mode, 1.1, 0.1, -0.5, 0.5)
    assert S.shape == (2, B, B)
    near = S[1].cpu() != 0
    assert bool(near[0, 1]) and bool(near[1, 0]) and bool(near[0, 3]) and not bool(near[0, 0])     # the planted pairs are re-evaluated
    assert bool(((S[0].cpu() != 0) & near).sum() == 0)
    tol = 1e-5 * (abs(ref) if only_near else max(1.0, abs(ref)))
    assert abs(float(loss) - ref) <= tol, (float(loss), ref)
    dz = ops.time_matching_backward(zd, S, None, wm).cpu().double()
    want = gref * wm
    assert (dz - want).abs().max() <= 2e-5 * want.abs().max() + 1e-12, (float((dz - want).abs().max()), float(want.abs().max()))
    # exact duplicates: distance exactly 0, and no gradient flows between them beyond what their other partners cause
    assert float(S.sum()) == float(S.sum())                # finite
    if only_near and mode == 0:
        # a pair of exact duplicates with no other partner: zero loss, zero gradient, bit for bit (the reference: 0 - 0)
        z2 = torch.cat([base[:1], base[:1], base[1:2] * 3.0, base[2:3] - 5.0], 0)
        tm2 = torch.zeros(4, 4); tm2[0, 1] = tm2[1, 0] = 2.0
        l2, S2 = ops.time_matching_forward(z2.to(DEV), tm2.to(DEV), 0)
        assert float(l2) == 0.0
        assert float(ops.time_matching_backward(z2.to(DEV), S2, None, wm).abs().max()) == 0.0


@pytest.mark.parametrize("B,n,frames", [(200, 4096, 8), (64, 1024, 4), (513, 256, 16)])
def test_time_matching_sparse_form(ops, B, n, frames):
    """vq_vae.py:331 (mode 0) only needs the pairs with a nonzero entry of time_matching_mat.  A batch's relation matrix --
    trajectories of consecutive frames: adjacent frames 2, the rest of a trajectory 1 -- holds a handful per row: the device
    counts them and both GEMMs fall away (S has no far part), every related pair is taken from differences.  Loss and
    gradient against the reference's expression in float64, against the dense form of the same call, and the gradient
    again from an S that lost its state word (the dense backward of an all-zero far part)."""
    g = torch.Generator().manual_seed(B + frames)
    z = torch.randn(B, n, generator=g) * 0.6 + 0.05
    tm = torch.zeros(B, B)
    for t0 in range(0, B - frames + 1, frames + 3):            # trajectories with unrelated samples between them
        for a in range(frames):
            z[t0 + a] = z[t0] + 0.02 * a * torch.randn(n, generator=g)
            for b in range(frames):
                if a != b:
                    tm[t0 + a, t0 + b] = 2.0 if abs(a - b) == 1 else 1.0
    tm[1, B - 1] = 1.0                                         # one-directional entries count as well
    ref, gref = _tm_reference(z, tm, 0)
    zd, tmd = z.to(DEV), tm.to(DEV)
    loss, S = ops.time_matching_forward(zd, tmd, 0)
    assert int(S._dm_tm_state[0]) == int((tm != 0).sum())
    assert float(S[0].abs().max()) == 0.0 and bool((S[1].cpu() != 0)[0, 1])      # the sparse form ran: no far part
    assert torch.equal(S[1].cpu() != 0, ((tm + tm.T) != 0) & ~torch.eye(B, dtype=torch.bool))
    assert abs(float(loss) - ref) <= 1e-6 * abs(ref), (float(loss), ref)
    other = torch.randn(B, n, generator=g).to(DEV)
    dz = ops.time_matching_backward(zd, S, None, 3.0, add=other)
    want = gref * 3.0 + other.cpu().double()
    assert (dz.cpu().double() - want).abs().max() <= 2e-6 * (gref.abs().max() * 3.0) + 1e-6 * float(other.abs().max())
    dz_plain = ops.time_matching_backward(zd, S, None, 3.0)
    assert (dz_plain.cpu().double() - gref * 3.0).abs().max() <= 2e-6 * gref.abs().max() * 3.0
    # the dense form of the same term, and the dense backward of this S
    loss_d, S_d = ops.time_matching_forward(zd, tmd, 0, allow_sparse=False)
    assert abs(float(loss_d) - float(loss)) <= 1e-5 * abs(ref)
    dz_d = ops.time_matching_backward(zd, S_d, None, 3.0)
    assert (dz_d - dz_plain).abs().max() <= 2e-5 * float(dz_plain.abs().max())
    assert torch.equal(ops.time_matching_backward(zd, S.clone(), None, 3.0), dz_plain)
    # a matrix with more than 32 entries per row stays dense
    tm_dense = (torch.rand(B, B, generator=g) < 0.5).float().to(DEV)
    _, S2 = ops.time_matching_forward(zd, tm_dense, 0)
    assert float(S2[0].abs().max()) > 0.0


@pytest.mark.parametrize("B,n,spread", [(200, 4096, 2.0), (513, 256, 2.0), (130, 1024, 0.3)])
def test_time_matching_gradient_product_skips_empty_blocks(ops, B, n, spread):
    """The z16 / z32 form (vae.py:327-336): every pair has a distance to evaluate, but an unrelated pair beyond the hinge's
    margin has no gradient, so S is as sparse as the relation matrix once the latents lie apart (spread 2: sim ~ 8 > 1;
    spread 0.3: most hinges active, S dense).  The forward call marks the nonzero (64 x 32) blocks of S and the gradient
    product multiplies only those: bit-equal to the stateless product of the same S, and right against float64."""
    g = torch.Generator().manual_seed(B)
    z = torch.randn(B, n, generator=g) * spread
    tm = torch.zeros(B, B)
    for t0 in range(0, B - 7, 11):
        for a in range(8):
            z[t0 + a] = z[t0] + 0.4 * spread * torch.randn(n, generator=g)     # related, but not "near" (> 25 % apart)
            for b in range(8):
                if a != b:
                    tm[t0 + a, t0 + b] = 2.0 if abs(a - b) == 1 else 1.0
    ref, gref = _tm_reference(z, tm, 1)
    zd, tmd = z.to(DEV), tm.to(DEV)
    loss, S = ops.time_matching_forward(zd, tmd, 1, 1.1, 0.1, -0.5, 0.5)
    assert abs(float(loss) - ref) <= 1e-5 * max(1.0, abs(ref))
    nchunks, npanels = (B + 31) // 32, (B + 63) // 64
    fmap = S._dm_tm_state[4:].cpu().numpy().reshape(npanels, nchunks)
    marked, blocks = int((fmap != 0).sum()), npanels * nchunks
    far = S[0].cpu()
    for pnl in range(npanels):                                 # the map covers every nonzero of the far part
        for c in range(nchunks):
            if bool((far[64 * pnl:64 * pnl + 64, 32 * c:32 * c + 32] != 0).any()):
                assert fmap[pnl, c] != 0, (pnl, c)
    if spread > 1.0:
        assert 0 < marked <= blocks // 2, (marked, blocks)    # far-apart latents: only the trajectories' blocks (along the diagonal)
    else:
        assert marked > blocks // 2
    other = torch.randn(B, n, generator=g).to(DEV)
    dz = ops.time_matching_backward(zd, S, None, 5.0, add=other)
    assert torch.equal(dz, ops.time_matching_backward(zd, S.clone(), None, 5.0, add=other))   # (a copy of S: no state, every block)
    want = gref * 5.0 + other.cpu().double()
    assert (dz.cpu().double() - want).abs().max() <= 2e-5 * float(gref.abs().max()) * 5.0 + 1e-6 * float(other.abs().max())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_zscore_patch_matches_numpy(ops, dtype):
    """pipeline/train_utils.py:252-274 zscore_patch (float64 numpy, population std, + eps) then .float()."""
    g = torch.Generator().manual_seed(51)
    x = (torch.rand(5, 2, 128, 128, generator=g, dtype=torch.float64) * 3000 + 100).to(dtype)
    xn = x.numpy().astype(np.float64)
    ref = ((xn - xn.mean((2, 3), keepdims=True)) / (xn.std((2, 3), keepdims=True) + np.finfo(float).eps)).astype(np.float32)
    out = ops.zscore_patch(x.to(DEV))
    assert out.dtype == torch.float32
    close(out, torch.from_numpy(ref), 2e-7, 2e-7, "zscore_patch")
    const = ops.zscore_patch(torch.full((1, 1, 8, 8), 7.0, dtype=dtype, device=DEV))     # zero variance: 0 / eps
    assert torch.equal(const.cpu(), torch.zeros(1, 1, 8, 8))


def test_augment_matches_torch(ops):
    B, Cn, h = 9, 2, 16
    x = rnd(B, Cn, h, h, seed=1)
    flips = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2], dtype=torch.int32)
    rots = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3, 1], dtype=torch.int32)
    ref = []
    for i in range(B):                       # run_training.py:397-403
        img = x[i]
        if flips[i] != 0:
            img = torch.flip(img, dims=(int(flips[i]),))
        ref.append(torch.rot90(img, k=int(rots[i]), dims=[1, 2]))
    out = ops.augment(x.to(DEV), flips.to(DEV), rots.to(DEV))
    assert torch.equal(out.cpu(), torch.stack(ref))


def test_bad_arguments_raise(ops):
    x = rnd(1, 16, 16, 16).to(DEV)
    with pytest.raises(ValueError):
        ops.vq_forward(rnd(1, 513, 4, 4).to(DEV), rnd(4, 513).to(DEV))   # embedding_dim outside 1 .. 512
    with pytest.raises(ValueError):
        ops.conv3x3(ops.Op(x), ops.weight_view(x, 1, 1, 1, 1), 1, 16, 16, 16, 16, taps=5)   # only 3x3 and 1x1
    with pytest.raises(ValueError):
        ops.vq_forward(rnd(1, 16, 4, 4), rnd(4, 16))                       # CPU tensors: no fallback


def test_e1_border_bias_table_replaces_the_ones_channel(ops):
    """enc.1(enc.0(x)) (vq_vae.py:277-278) as ONE conv over x alone: enc.0's bias reaches the output through a
    per-position bias table (first / interior / last row x column), bit-for-bit the same mathematics as the
    ones-channel composite but with K = 16*NIN."""
    B, NIN, C0, C1, H = 3, 2, 8, 8, 128
    x = rnd(B, NIN, H, H, seed=11)
    w0, b0 = rnd(C0, NIN, 1, 1, seed=12), rnd(C0, seed=13)
    w1, b1 = rnd(C1, C0, 4, 4, seed=14) * 0.2, rnd(C1, seed=15)
    ref = F.conv2d(F.conv2d(x, w0, b0), w1, b1, stride=2, padding=1)
    dv = [t.to(DEV).contiguous() for t in (x, w0, b0, w1, b1)]
    weff, border = ops.e1_compose_border(dv[1], dv[2], dv[3], dv[4])
    out, st = ops.conv4x4s2(ops.Op(dv[0]), ops.weight_view(weff, (NIN + 1) * 16, 16, 4, 1), B, NIN, C1, H, H,
                            want_stats=True, bias_border=border)
    close(out, ref, 2e-5, 2e-5, "border-bias composite")
    ones, _ = ops.conv4x4s2(ops.Op(dv[0], ones=True), ops.weight_view(weff, (NIN + 1) * 16, 16, 4, 1), B, NIN + 1, C1, H, H,
                            bias=dv[4])
    close(out, ones, 2e-5, 2e-5, "border-bias vs ones channel")
    tot = torch.empty(C1, 2, device=DEV, dtype=torch.float64)
    assert torch.allclose(st.sum(0)[:, 0].cpu(), ref.double().sum((0, 2, 3)), rtol=1e-5, atol=1e-3)


# ===================================================================== fused decoder tail
@pytest.mark.parametrize("nin,masked,B,hw", [(2, False, 3, (64, 64)), (2, True, 2, (64, 64)), (4, True, 2, (64, 64)),
                                              (1, False, 70, (64, 64)),
                                              # other widths: 64 lanes = 56 owned columns + 4 halo columns either side
                                              (4, True, 2, (128, 128)), (2, False, 3, (16, 32)), (3, True, 2, (24, 100)),
                                              (2, False, 2, (8, 56)), (2, True, 2, (16, 60)), (1, False, 5, (8, 4)),
                                              (2, False, 1, (64, 256)), (4, False, 1, (128, 64)),
                                              # widths that are multiples of 64: the training kernel takes tiles of 64 owned
                                              # columns with seam terms (two, three and five tiles per row; every channel count)
                                              (3, True, 2, (16, 192)), (1, False, 3, (8, 128)), (4, False, 2, (24, 128)),
                                              (2, True, 1, (8, 320)), (4, True, 70, (8, 128))])
def test_dec_tail_fused_forward_backward(ops, nin, masked, B, hw):
    """dec.4 + ReLU + dec.6 + masked loss in one kernel, and its fused backward, vs the ATen composition."""
    c, (h, w) = 4, hw
    assert ops.dec_tail_supported(c, nin, h, w)
    pre = rnd(B, c, h, w, seed=1).requires_grad_(True)
    w4 = (rnd(c, c, 4, 4, seed=2) * 0.3).requires_grad_(True)
    b4 = rnd(c, seed=3).requires_grad_(True)
    w6 = rnd(nin, c, 1, 1, seed=4).requires_grad_(True)
    b6 = rnd(nin, seed=5).requires_grad_(True)
    x = rnd(B, nin, 2 * h, 2 * w, seed=6)
    mask = (torch.rand(B, 1, 2 * h, 2 * w, generator=torch.Generator().manual_seed(7)) > 0.4).float() * 0.5 + 0.5 if masked else None
    var = torch.linspace(0.5, 1.5, nin)
    d2 = F.relu(pre)
    d4 = F.relu(F.conv_transpose2d(d2, w4, b4, stride=2, padding=1))
    dec_ref = F.conv2d(d4, w6, b6)
    mm = mask if masked else torch.ones_like(x)
    loss_ref = torch.mean(F.mse_loss(dec_ref * mm, x * mm, reduction="none") / var.reshape(1, nin, 1, 1))
    (loss_ref * 0.7).backward()

    dv = [t.detach().to(DEV).contiguous() for t in (d2, w4, b4, w6, b6, x, var)]
    mk = mask.to(DEV) if masked else None
    dec, slabs = ops.dec_tail_forward(dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], mk, dv[6])
    recon = ops.loss_finalize(slabs, x.numel(), torch.zeros(2, device=DEV), 1.0, 0.0)[0]
    close(dec, dec_ref, 2e-5, 2e-5, "decoded")
    assert abs(float(recon) - float(loss_ref)) <= 3e-6 * abs(float(loss_ref))
    dec_only, none = ops.dec_tail_forward(dv[0], dv[1], dv[2], dv[3], dv[4], None, None, dv[6])
    assert none is None and torch.equal(dec_only, dec)

    g2, part, wsl = ops.dec_tail_backward(dv[0], dv[1], dv[2], dv[3], dec, dv[5], mk, dv[6], torch.tensor([0.7], device=DEV))
    flat = torch.empty(part.shape[1], device=DEV)
    ops.sum_slabs(part, flat)
    dw4 = torch.empty(c, c, 4, 4, device=DEV)
    ops.reduce_slabs(wsl, dw4)
    sc = lambda t: t.abs().max().item()
    close(g2, pre.grad, 1e-4, 2e-5 * sc(pre.grad), "g2 (masked by d2 > 0)")
    close(dw4, w4.grad, 1e-4, 1e-4 * sc(w4.grad), "dW4")
    close(flat[:nin * c].reshape(nin, c), w6.grad.reshape(nin, c), 1e-4, 1e-4 * sc(w6.grad), "dW6")
    close(flat[nin * c:nin * c + nin], b6.grad, 1e-4, 1e-4 * sc(b6.grad), "db6")
    close(flat[nin * c + nin:nin * c + nin + c], b4.grad, 1e-4, 1e-4 * sc(b4.grad), "db4")
    close(flat[nin * c + nin + c:], pre.grad.sum((0, 2, 3)), 1e-4, 1e-4 * sc(pre.grad.sum((0, 2, 3))), "db2 = sum g2")
    g2b, _, wsl2 = ops.dec_tail_backward(dv[0], dv[1], dv[2], dv[3], dec, dv[5], mk, dv[6], torch.tensor([0.7], device=DEV))
    dw4b = torch.empty_like(dw4)
    ops.reduce_slabs(wsl2, dw4b)
    assert torch.equal(g2b, g2) and torch.equal(dw4b, dw4), "fused tail must be bitwise reproducible"

    # training pass: the loss of the forward kernel and the gradients of the backward kernel from ONE kernel
    g2t, part_t, wsl_t, loss_t = ops.dec_tail_train(dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], mk, dv[6],
                                                    torch.tensor([0.7], device=DEV))
    recon_t = ops.loss_finalize(loss_t, x.numel(), torch.zeros(2, device=DEV), 1.0, 0.0)[0]
    assert abs(float(recon_t) - float(loss_ref)) <= 3e-6 * abs(float(loss_ref))
    flat_t = torch.empty_like(flat)
    ops.sum_slabs(part_t, flat_t)
    dw4t = torch.empty_like(dw4)
    ops.reduce_slabs(wsl_t, dw4t)
    close(g2t, pre.grad, 1e-4, 2e-5 * sc(pre.grad), "train: g2")
    close(dw4t, w4.grad, 1e-4, 1e-4 * sc(w4.grad), "train: dW4")
    close(flat_t[:nin * c].reshape(nin, c), w6.grad.reshape(nin, c), 1e-4, 1e-4 * sc(w6.grad), "train: dW6")
    close(flat_t[nin * c:nin * c + nin], b6.grad, 1e-4, 1e-4 * sc(b6.grad), "train: db6")
    close(flat_t[nin * c + nin:nin * c + nin + c], b4.grad, 1e-4, 1e-4 * sc(b4.grad), "train: db4")
    close(flat_t[nin * c + nin + c:], pre.grad.sum((0, 2, 3)), 1e-4, 1e-4 * sc(pre.grad.sum((0, 2, 3))), "train: db2")


# ===================================================================== latent tail (inference path, per-sample statistics)
LT_ATEN = [(1, 2), (3, 0), (2, 1), (5, 3), (4, 4), (600, 2)]


# (ids as they were while a second entry form, from enc.4's output, existed: "-False" is the (a3, coef3) form)
@pytest.mark.parametrize("B,nres", LT_ATEN, ids=["%d-%d-False" % c for c in LT_ATEN])
def test_latent_tail_kernel_vs_aten_batch_of_one_calls(ops, B, nres):
    """dm_latent_tail_forward (enc.10 + enc.11 + nres residual layers of every patch, per-patch BatchNorm statistics)
    against the ATen composition called one patch at a time in train mode -- the arithmetic of patch_VAE.py:445-452 on
    vq_vae.py:287-289 / :203-224 -- for 0..4 residual layers, random BatchNorm weights / biases / conv biases; and the
    per-patch sums it writes for the running-statistics replay."""
    C, CR = 16, 32
    g = torch.Generator().manual_seed(100 * B + nres)
    r = lambda *s, k=1.0: torch.randn(*s, generator=g) * k
    a3 = r(B, C, 16, 16)
    coef3 = torch.stack([r(B, C).abs() + 0.5, torch.zeros(B, C), r(B, C, k=0.3), torch.zeros(B, C)], 2).contiguous()
    # (the draws of the retired entry form's inputs -- a2, coef2, w7, b7, gamma3, beta3 -- keep the inputs below as they were)
    r(B, C, 32, 32), r(B, C), r(B, C), r(C, C, 4, 4), r(C), r(C), r(C)
    w10, b10, g4, be4 = r(C, C, 3, 3, k=0.15), r(C, k=0.2), r(C).abs() + 0.5, r(C, k=0.3)
    res = [(r(CR, C, 3, 3, k=0.15), r(CR, k=0.2), r(CR).abs() + 0.5, r(CR, k=0.3), 1e-5,
            r(C, CR, 1, 1, k=0.2), r(C, k=0.2), r(C).abs() + 0.5, r(C, k=0.3), 1e-5) for _ in range(nres)]
    assert ops.latent_tail_supported(C, CR, 16, 16, nres) and not ops.latent_tail_supported(C, CR, 16, 16, 5)

    def bn(v, gam, bet):                                   # batch-of-one train-mode BatchNorm
        return F.batch_norm(v, None, None, gam, bet, True, 0.1, 1e-5)
    nref = min(B, 6)
    zs, sums = [], []
    for i in range(nref):
        t = torch.relu(coef3[i, :, 0].reshape(1, C, 1, 1) * a3[i:i + 1] + coef3[i, :, 2].reshape(1, C, 1, 1))
        a4 = F.conv2d(t, w10, b10, padding=1)
        per = [a4]
        h = bn(a4, g4, be4)
        for wa, ba, ga, bea, _, wb, bb, gb, beb, _ in res:
            ra = F.conv2d(torch.relu(h), wa, ba, padding=1)
            rb = F.conv2d(torch.relu(bn(ra, ga, bea)), wb, bb)
            per += [ra, rb]
            h = h + bn(rb, gb, beb)
        zs.append(h)
        sums.append([torch.stack([v.double().sum((0, 2, 3)), (v.double() ** 2).sum((0, 2, 3))], 1) for v in per])
    d = lambda t: t.to(DEV).contiguous()
    dres = [tuple(d(v) if torch.is_tensor(v) else v for v in layer) for layer in res]
    z, st4, sts = ops.latent_tail_forward(d(a3), d(coef3), d(w10), d(b10), d(g4), d(be4), 1e-5, dres)
    torch.cuda.synchronize()
    assert z.shape == (B, C, 16, 16) and st4.shape == (B, C, 2) and len(sts) == nres
    zr = torch.cat(zs, 0)
    close(z[:nref], zr, 2e-5, 2e-5 * max(1.0, zr.abs().max().item()), "z")
    assert bool(torch.isfinite(z).all())
    flat = [st4] + [t for pair in sts for t in pair]
    for i in range(nref):
        for got, want in zip(flat, sums[i]):
            assert torch.allclose(got[i].cpu(), want, rtol=1e-5, atol=1e-4), (i, got.shape)


def _neg_nan():
    """x86's default NaN (0/0 on the host): 0xFFC00000, sign bit set."""
    return torch.tensor([-4194304], dtype=torch.int32).view(torch.float32)[0]


def test_relu_keeps_nans_of_either_sign(ops):
    """torch.relu keeps every NaN; until round 2 the operand-load ReLU (an integer max on the bits) turned a NaN with the
    sign bit set into +0, and the epilogue / decoder-tail ReLUs (fmaxf) turned every NaN into 0.  A NaN patch must stay
    visible in the latents, the reconstruction and the loss."""
    B, C, H = 2, 16, 16
    x = rnd(B, C, H, H, seed=1)
    x[0, 3, 5, 7] = _neg_nan()
    x[1, 9, 0, 0] = float("nan")
    assert int(x.view(torch.int32)[0, 3, 5, 7]) < 0
    coef = torch.stack([rnd(C, seed=4).abs() + 0.5, torch.zeros(C), rnd(C, seed=5) * 0.3, torch.zeros(C)], 1)
    for mode in (1, 3):
        # operand_load4 (dm_apply) and the tile commit of the MFMA convolutions (tile.h)
        ref = load_ref(x, mode, coef) if mode == 3 else torch.relu(x)
        out = ops.apply(ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None), B, C, H, H)
        assert torch.equal(torch.isnan(out.cpu()), torch.isnan(ref)) and int(torch.isnan(ref).sum()) == 2, mode
        w = rnd(16, C, 3, 3, seed=2, scale=0.2)
        refc = F.conv2d(ref, w, None, padding=1)
        outc, _ = ops.conv3x3(ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None),
                              ops.weight_view(w.to(DEV), C * 9, 9, 3, 1), B, C, 16, H, H, taps=9)
        nan_ref = torch.isnan(refc)
        assert torch.equal(torch.isnan(outc.cpu()), nan_ref) and int(nan_ref.sum()) == 16 * (9 + 4), mode
        close(torch.nan_to_num(outc.cpu()), torch.nan_to_num(refc), 2e-5, 2e-5, "finite part")
    # epilogue ReLU of the transposed convolutions (dec.0 / dec.2) and the fused decoder tail (dec.4 + ReLU + dec.6)
    wt = rnd(C, 8, 4, 4, seed=6, scale=0.2)
    bias = rnd(8, seed=7)
    ref = torch.relu(F.conv_transpose2d(x, wt, bias, stride=2, padding=1))
    out, _ = ops.conv3x3(ops.Op(x.to(DEV)), ops.weight_view(wt.to(DEV), 16, 8 * 16, 4, 1), B, C, 4 * 8, H, H, taps=9,
                         pixel_shuffle=True, bias=bias.to(DEV), relu=True)
    # (the phase-decomposed transposed convolution multiplies a few structurally zero taps: NaN * 0 = NaN reaches the
    #  direct neighbours of the reference's NaN set too -- more visible, never less)
    nan_ref, nan_out = torch.isnan(ref), torch.isnan(out.cpu())
    assert int(nan_ref.sum()) > 0 and not bool((nan_ref & ~nan_out).any())
    grown = F.max_pool2d(nan_ref.float(), 5, stride=1, padding=2) > 0
    assert not bool((nan_out & ~grown).any())
    d2 = rnd(B, 4, 64, 64, seed=8)
    d2[1, 2, 10, 11] = _neg_nan()
    w4, b4, w6, b6 = rnd(4, 4, 4, 4, seed=9, scale=0.3), rnd(4, seed=10), rnd(2, 4, 1, 1, seed=11), rnd(2, seed=12)
    ref = F.conv2d(torch.relu(F.conv_transpose2d(d2, w4, b4, stride=2, padding=1)), w6, b6)
    dec, _ = ops.dec_tail_forward(d2.to(DEV), w4.to(DEV), b4.to(DEV), w6.to(DEV), b6.to(DEV), None, None,
                                  torch.ones(2, device=DEV))
    assert torch.equal(torch.isnan(dec.cpu()), torch.isnan(ref)) and int(torch.isnan(ref).sum()) > 0


@pytest.mark.parametrize("D,K,scale_z,scale_e", [(16, 64, 1.0, 1.0), (16, 64, 30.0, 0.05), (16, 64, 1e-3, 4.0), (16, 64, 1e4, 1e4),
                                                   (32, 200, 0.3, 2.0), (64, 512, 1.0, 0.2), (16, 4096, 1.0, 1.0),
                                                   # code groups of the exact re-check: one group, four, five with a ragged last
                                                   (16, 65, 1.0, 1.0), (16, 1000, 1.0, 0.5), (16, 5000, 1.0, 1.0), (32, 3000, 1.0, 1.0)])
def test_vq_bf16_split_filter_scales_and_clusters(ops, D, K, scale_z, scale_e):
    """The bf16-split filter's tolerance is proven relative to A = |z|^2 + 2 max |e|^2: magnitudes far from 1, latents much
    larger or smaller than the codes, and a codebook whose codes sit in tight clusters (many runner-ups inside the
    tolerance) must all come out with the exact kernel's indices."""
    g = torch.Generator().manual_seed(D * K)
    centres = torch.randn(max(K // 8, 1), D, generator=g)
    cb = (centres[torch.arange(K) % centres.shape[0]] + 1e-3 * torch.randn(K, D, generator=g)) * scale_e
    cb[: K // 2] = torch.randn(K // 2, D, generator=g) * scale_e          # half spread out, half clustered
    z = torch.randn(24, D, 16, 16, generator=g) * scale_z
    z[:4] = cb[torch.randint(0, K, (4 * 256,), generator=g)].reshape(4, 16, 16, D).permute(0, 3, 1, 2) * (1 + 1e-4 * torch.randn(4, D, 16, 16, generator=g))
    zd, cbd = z.to(DEV), cb.to(DEV)
    idx_e, out_e, _, hist_e = ops.vq_forward(zd, cbd, variant=DM_VQ_EXACT)
    idx_b, out_b, _, hist_b, nre = ops.vq_forward(zd, cbd, variant=DM_VQ_BF16, want_rechecked=True)
    assert torch.equal(idx_e, idx_b) and torch.equal(out_e, out_b) and torch.equal(hist_e, hist_b)
    print(f"D={D} K={K} scales ({scale_z}, {scale_e}): {int(nre.cpu())} of {idx_b.numel()} positions re-evaluated exactly")


@pytest.mark.parametrize("B,hw", [(3, 32), (2, 64), (5, 32), (300, 32), (70, 64), (2, 128)])
def test_conv_bwd_s2_fused_matches_autograd_and_the_two_kernels(ops, B, hw):
    """Kernel D (csrc/conv_mfma.hip): data gradient + weight gradient of a Conv2d(8 -> 16, 4, 2, 1) from one staging of
    (dy, a_out, a_in), with the BatchNorm-backward operand, the ReLU mask of the layer input and the (sum, sum * input)
    statistics -- against torch autograd, and against the two kernels it replaces (the data gradient bit for bit where the
    MFMA order is the same, hw = 128; the weight gradient to summation order).  B = 300: more tiles than workgroups."""
    CD, CX, H, W = 16, 8, hw, hw
    dy, a_out = rnd(B, CD, H, W, seed=1), rnd(B, CD, H, W, seed=2)
    coefD = torch.stack([rnd(CD, seed=3), rnd(CD, seed=4) * 0.1, rnd(CD, seed=5) * 0.1, torch.zeros(CD)], 1)
    a_in = rnd(B, CX, 2 * H, 2 * W, seed=6)
    coefT = torch.stack([rnd(CX, seed=7).abs() + 0.5, torch.zeros(CX), rnd(CX, seed=8) * 0.3, torch.zeros(CX)], 1)
    w = rnd(CD, CX, 4, 4, seed=9, scale=0.2)
    da = load_ref(dy, 4, coefD, a_out)
    t_in = load_ref(a_in, 3, coefT)
    x = t_in.clone().requires_grad_(True)
    wt = w.clone().requires_grad_(True)
    F.conv2d(x, wt, None, stride=2, padding=1).backward(da)
    dx_ref = x.grad * (load_ref(a_in, 2, coefT) > 0)
    assert ops.conv_bwd_s2_fused_supported(CD, CX, H, W) and not ops.conv_bwd_s2_fused_supported(CD, CX, H, 16)
    dyd, aod, aid, cDd, cTd, wd = (t.to(DEV) for t in (dy, a_out, a_in, coefD, coefT, w))     # (one device copy each: the
    dst = torch.empty(CD, CX, 4, 4, device=DEV)                                               #  kernel checks mask IS the input)
    dyop = lambda: ops.Op(dyd, 4, cDd, p1=aod)
    run = lambda out: ops.conv_bwd_s2_fused(dyop(), ops.Op(aid, 3, cTd), ops.weight_view(wd, 16, CX * 16, 4, 1), out, B, CD, CX,
                                            H, W, mask=ops.Op(aid, 2, cTd), stat_q=aid)
    dx, st = run(dst)
    close(dx, dx_ref, 3e-5, 3e-5, "fused data gradient")
    close(dst, wt.grad, 3e-5, 3e-5 * float(wt.grad.abs().max()), "fused weight gradient")
    close_stats(st.sum(0), dx_ref, a_in, "fused statistics")
    # the two kernels it replaces
    dx2, st2 = ops.conv3x3(dyop(), ops.weight_view(wd, 16, CX * 16, 4, 1), B, CD, 4 * CX, H, W, taps=9, pixel_shuffle=True,
                           want_stats=True, mask=ops.Op(aid, 2, cTd), stat_q=aid)
    dst2 = torch.empty_like(dst)
    ops.wgrad(dyop(), ops.Op(aid, 3, cTd), dst2, B, CD, CX, H, W, 4)
    if hw in (32, 64):
        # a tile spans the row (8 x 32 tiles at 32 columns, 4 x 64 at 64): kernel D takes the data gradient without structural zeros (round 5) -- the centre column's and the
        # outer columns' products in two accumulators, added at the end -- so the sum's order differs from the two-kernel path's
        # single chain; both stay within the same distance of the float64 result
        e_d, e_2 = (dx.cpu().double() - dx_ref.double()).abs().max(), (dx2.cpu().double() - dx_ref.double()).abs().max()
        assert float(e_d) <= 1.5 * float(e_2) + 1e-7, (float(e_d), float(e_2))
        close(dx, dx2, 2e-6, 2e-6 * float(dx2.abs().max()), "fused vs separate data gradient")
    else:
        assert torch.equal(dx, dx2)                          # the three-column mapping: same MFMA order, bit for bit
    close(dst, dst2, 2e-5, 2e-5 * float(dst2.abs().max()), "fused vs separate weight gradient")
    close(st.sum(0), st2.sum(0), 1e-7, 1e-7 * float(st2.sum(0).abs().max()), "statistics vs separate")   # (fp32 quads, grouped by tile)
    # two runs agree to the bit (fixed slab order, no float atomics)
    dstb = torch.empty_like(dst)
    dxb, stb = run(dstb)
    assert torch.equal(dst, dstb) and torch.equal(dx, dxb) and torch.equal(st, stb)
    with pytest.raises(ValueError, match="layer input"):       # a mask that is not the layer input is refused on the host
        ops.conv_bwd_s2_fused(dyop(), ops.Op(aid, 3, cTd), ops.weight_view(wd, 16, CX * 16, 4, 1), dstb, B, CD, CX, H, W,
                              mask=ops.Op(aid.clone(), 2, cTd))



@pytest.mark.parametrize("B,cs,ct,hs,ws,smode,tmode", [(5, 64, 64, 16, 16, 4, 3), (3, 64, 64, 8, 16, 0, 1), (2, 32, 64, 16, 32, 3, 0),
                                                       (7, 64, 32, 16, 16, 1, 3), (4, 32, 32, 8, 32, 4, 0), (1, 64, 64, 8, 16, 4, 3),
                                                       (200, 64, 64, 16, 16, 4, 3)])
def test_stream_wgrad_1x1(ops, B, cs, ct, hs, ws, smode, tmode):
    """wide_stream.hip: the 1x1 weight gradient with both operands loaded straight into the matrix instruction's layout
    (contiguous pixel ranges per workgroup, across sample boundaries; fewer groups than workgroups; every operand mode)."""
    dy, a = rnd(B, cs, hs, ws, seed=1), rnd(B, cs, hs, ws, seed=2)
    coef = torch.stack([rnd(cs, seed=3), rnd(cs, seed=4) * 0.1, rnd(cs, seed=5) * 0.1, torch.zeros(cs)], 1)
    t = rnd(B, ct, hs, ws, seed=6)
    tcoef = torch.stack([rnd(ct, seed=7), torch.zeros(ct), rnd(ct, seed=8) * 0.2, torch.zeros(ct)], 1)
    w = torch.zeros(cs, ct, 1, 1, requires_grad=True)
    F.conv2d(load_ref(t.double(), tmode, tcoef.double()), w.double(), None).backward(load_ref(dy.double(), smode, coef.double(), a.double()))
    dst = torch.empty(cs, ct, 1, 1, device=DEV)
    S = ops.Op(dy.to(DEV), smode, coef.to(DEV) if smode >= 2 else None, p1=a.to(DEV) if smode == 4 else None)
    T = ops.Op(t.to(DEV), tmode, tcoef.to(DEV) if tmode >= 2 else None)
    assert ops.wgrad_plan(S, T, B, cs, ct, hs, ws, 1).kernel == SW.KERNELS["wgrad1x1_stream"]
    ops.wgrad(S, T, dst, B, cs, ct, hs, ws, 1)
    close(dst, w.grad.float(), 5e-5, 5e-5 * max(w.grad.abs().max().item(), 1e-6), "stream wgrad 1x1")


@pytest.mark.parametrize("B,cin,nout,h,w,mode,transposed,epi", [
    (3, 64, 64, 16, 16, 3, False, "stats"), (2, 64, 64, 8, 16, 4, True, "gate+q"), (5, 32, 64, 16, 16, 1, False, "all"),
    (2, 64, 32, 16, 32, 0, True, "none"), (7, 32, 32, 8, 16, 4, False, "gate"), (1, 64, 64, 8, 16, 3, False, "all"),
    (150, 64, 64, 16, 16, 4, True, "gate+q")])
def test_stream_conv_1x1(ops, B, cin, nout, h, w, mode, transposed, epi):
    """wide_stream.hip: the 1x1 convolution with the weights in registers and the activations loaded straight into the matrix
    instruction's layout -- forward (BatchNorm + ReLU folded into the load, statistics) and data-gradient form (AFFINE2 load,
    transposed weight view, gate, statistics against the gate's tensor), bias / ReLU / residual, units across sample boundaries."""
    x, x1 = rnd(B, cin, h, w, seed=1), rnd(B, cin, h, w, seed=2)
    coef = torch.stack([rnd(cin, seed=3).abs() + 0.5, rnd(cin, seed=4) * 0.2, rnd(cin, seed=5) * 0.3, torch.zeros(cin)], 1)
    xin = load_ref(x.double(), mode, coef.double(), x1.double())
    inp = ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, p1=x1.to(DEV) if mode == 4 else None)
    if transposed:
        wt = rnd(cin, nout, 1, 1, seed=6, scale=0.2)
        wv, wref = ops.weight_view(wt.to(DEV), 1, nout, 0, 0), wt.permute(1, 0, 2, 3)
    else:
        wt = rnd(nout, cin, 1, 1, seed=6, scale=0.2)
        wv, wref = ops.weight_view(wt.to(DEV), cin, 1, 0, 0), wt
    kw, ref = {}, None
    bias = rnd(nout, seed=7) if epi == "all" else None
    ref = F.conv2d(xin, wref.double(), bias.double() if bias is not None else None)
    if bias is not None:
        kw.update(bias=bias.to(DEV), relu=True)
        ref = F.relu(ref)
    gate, q, resid = rnd(B, nout, h, w, seed=8), rnd(B, nout, h, w, seed=9), rnd(B, nout, h, w, seed=10)
    mcoef = torch.stack([rnd(nout, seed=11), torch.zeros(nout), rnd(nout, seed=12) * 0.3, torch.zeros(nout)], 1)
    if epi in ("gate", "gate+q", "all"):
        kw.update(mask=ops.Op(gate.to(DEV), 2, mcoef.to(DEV)))
        ref = ref * ((mcoef[:, 0].view(1, -1, 1, 1) * gate + mcoef[:, 2].view(1, -1, 1, 1)) > 0)
    if epi == "all":
        kw.update(resid=resid.to(DEV))
        ref = ref + resid
    sq = None
    if epi == "gate+q":
        gd = kw["mask"].p0
        kw.update(stat_q=gd)                       # the training step's form: statistics against the gate's own tensor
        sq = gate
    elif epi == "all":
        kw.update(stat_q=q.to(DEV))
        sq = q
    assert ops.conv3x3_plan(inp, B, cin, nout, h, w, taps=1, stats=epi != "none", **kw).kernel == SW.KERNELS["conv1x1_stream"]
    out, st = ops.conv3x3(inp, wv, B, cin, nout, h, w, taps=1, want_stats=epi != "none", **kw)
    close(out, ref.float(), 5e-5, 5e-5, "stream conv 1x1")
    if st is not None:
        close_stats(st.sum(0), ref.float(), sq)


@pytest.mark.parametrize("B,cs,ct,hs,ws,smode,tmode", [(3, 32, 2, 64, 64, 4, 0), (2, 32, 2, 8, 32, 3, 0), (2, 16, 4, 16, 32, 0, 3),
                                                       (5, 32, 1, 16, 64, 1, 1), (2, 64, 1, 8, 32, 4, 3), (1, 32, 3, 8, 32, 4, 0),
                                                       (40, 32, 2, 64, 64, 4, 0)])
def test_stream_wgrad_4x4s2_few_t_channels(ops, B, cs, ct, hs, ws, smode, tmode):
    """wide_stream.hip: weight gradient of the wide encoder's first convolution / the decoder's last transposed convolution
    (T = the image side with 1-4 channels): taps as the N dimension, T read by unaligned loads straight from global memory,
    borders zeroed after the transform; stages across row and sample boundaries."""
    dy, a = rnd(B, cs, hs, ws, seed=1), rnd(B, cs, hs, ws, seed=2)
    coef = torch.stack([rnd(cs, seed=3), rnd(cs, seed=4) * 0.1, rnd(cs, seed=5) * 0.1, torch.zeros(cs)], 1)
    t = rnd(B, ct, 2 * hs, 2 * ws, seed=6)
    tcoef = torch.stack([rnd(ct, seed=7), torch.zeros(ct), rnd(ct, seed=8) * 0.2 + 0.3, torch.zeros(ct)], 1)
    w = torch.zeros(cs, ct, 4, 4, requires_grad=True, dtype=torch.float64)
    F.conv2d(load_ref(t.double(), tmode, tcoef.double()), w, None, stride=2, padding=1).backward(
        load_ref(dy.double(), smode, coef.double(), a.double()))
    dst = torch.empty(cs, ct, 4, 4, device=DEV)
    S = ops.Op(dy.to(DEV), smode, coef.to(DEV) if smode >= 2 else None, p1=a.to(DEV) if smode == 4 else None)
    T = ops.Op(t.to(DEV), tmode, tcoef.to(DEV) if tmode >= 2 else None)
    assert ops.wgrad_plan(S, T, B, cs, ct, hs, ws, 4).kernel == SW.KERNELS["wgrad_s2_thin_stream"]
    ops.wgrad(S, T, dst, B, cs, ct, hs, ws, 4)
    close(dst, w.grad.float(), 5e-5, 5e-5 * max(w.grad.abs().max().item(), 1e-6), "stream wgrad 4x4/s2")


@pytest.mark.parametrize("B,cin,nout,h,w,mode,epi", list(SW.OLD_S2_THIN))
def test_stream_conv_4x4s2_few_input_channels(ops, B, cin, nout, h, w, mode, epi):
    """4x4 / stride 2 from 1-4 input channels on 128 columns: the wide encoder's first convolution (image -> 32 channels) and
    the data gradient of the decoder's last transposed convolution; bias / ReLU / gate / residual / statistics.  The cases and
    the kernel each runs are tests/helpers/stream_walk.py's OLD_S2_THIN (asserted from the launch plan): wide_stream.hip's
    conv_s2_thin_stream_kernel (K = (channel, ky, kx), zero padding applied AFTER the operand transform, output rows 0 and
    OH - 1) only where the output grid tiles by 8 x 16, i.e. H % 16 == 0 -- at H = 4, 6, 8 the generic kernel runs, and
    1 -> 16 channels at H = 16 is a register-resident kernel's; the H = 16 cases beside them reach the streaming kernel."""
    x = rnd(B, cin, h, w, seed=1)
    coef = torch.stack([rnd(cin, seed=3).abs() + 0.5, torch.zeros(cin), rnd(cin, seed=5) * 0.3 + 0.2, torch.zeros(cin)], 1)
    xin = load_ref(x.double(), mode, coef.double())
    wt = rnd(nout, cin, 4, 4, seed=6, scale=0.2)
    kw = {}
    bias = rnd(nout, seed=7) if epi in ("bias", "all") else None
    ref = F.conv2d(xin, wt.double(), bias.double() if bias is not None else None, stride=2, padding=1)
    if bias is not None:
        kw.update(bias=bias.to(DEV))
    if epi == "all":
        kw.update(relu=True)
        ref = F.relu(ref)
    oh, ow = h // 2, w // 2
    gate, q, resid = rnd(B, nout, oh, ow, seed=8), rnd(B, nout, oh, ow, seed=9), rnd(B, nout, oh, ow, seed=10)
    mcoef = torch.stack([rnd(nout, seed=11), torch.zeros(nout), rnd(nout, seed=12) * 0.3, torch.zeros(nout)], 1)
    if epi in ("gate", "gate+q", "all"):
        kw.update(mask=ops.Op(gate.to(DEV), 2, mcoef.to(DEV)))
        ref = ref * ((mcoef[:, 0].view(1, -1, 1, 1) * gate + mcoef[:, 2].view(1, -1, 1, 1)) > 0)
    sq = None
    if epi == "all":
        kw.update(resid=resid.to(DEV), stat_q=q.to(DEV))
        ref = ref + resid
        sq = q
    elif epi == "gate+q":
        kw.update(stat_q=kw["mask"].p0)
        sq = gate
    inp = ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None)
    kernel = SW.OLD_S2_THIN[(B, cin, nout, h, w, mode, epi)]
    assert ops.conv4x4s2_plan(inp, B, cin, nout, h, w, stats=epi != "none", **kw).kernel == SW.KERNELS[kernel]
    out, st = ops.conv4x4s2(inp, ops.weight_view(wt.to(DEV), cin * 16, 16, 4, 1),
                            B, cin, nout, h, w, want_stats=epi != "none", **kw)
    close(out, ref.float(), 5e-5, 5e-5, "stream conv 4x4/s2")
    if st is not None:
        close_stats(st.sum(0), ref.float(), sq)


@pytest.mark.parametrize("B,ci,co,h,mode,relu", list(SW.OLD_CONVT_THIN))
def test_stream_conv_transpose_to_few_channels(ops, B, ci, co, h, mode, relu):
    """ConvTranspose2d(C -> 1 / 2, 4, 2, 1) on a 64-column grid -- the wide decoder's last layer.  The cases and the kernel each
    runs are tests/helpers/stream_walk.py's OLD_CONVT_THIN (asserted from the launch plan): wide_stream.hip's
    convT_thin_stream_kernel (vector units: weights as scalar-register pairs, one lane = 4 pixels, neighbours by DPP, padding rows
    zeroed AFTER the transform) where H % 8 == 0; at H = 4 and 12 the generic kernel runs, and the H = 8 / 16 cases beside those
    two reach the streaming kernel (12 input channels, not 8: 8 -> 2 on a tileable grid is a register-resident kernel's)."""
    w = 64
    x = rnd(B, ci, h, w, seed=1)
    coef = torch.stack([rnd(ci, seed=3).abs() + 0.5, torch.zeros(ci), rnd(ci, seed=5) * 0.3 + 0.2, torch.zeros(ci)], 1)
    wt = rnd(ci, co, 4, 4, seed=2, scale=0.2)
    bias = rnd(co, seed=4)
    ref = F.conv_transpose2d(load_ref(x.double(), mode, coef.double()), wt.double(), bias.double(), stride=2, padding=1)
    if relu:
        ref = F.relu(ref)
    inp = ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None)
    kernel = SW.OLD_CONVT_THIN[(B, ci, co, h, mode, relu)]
    assert ops.conv3x3_plan(inp, B, ci, 4 * co, h, w, taps=9, pixel_shuffle=True, bias=True, relu=relu).kernel == SW.KERNELS[kernel]
    out, _ = ops.conv3x3(inp, ops.weight_view(wt.to(DEV), 16, co * 16, 4, 1),
                         B, ci, 4 * co, h, w, taps=9, pixel_shuffle=True, bias=bias.to(DEV), relu=relu)
    close(out, ref.float(), 5e-5, 5e-5, "stream conv transpose")


@pytest.mark.parametrize("K,D,B,H", [(512, 64, 5, 32), (4096, 16, 4, 64), (300, 32, 3, 16), (100, 24, 3, 16)])
def test_vq_backward_large_codebooks_is_bit_reproducible(ops, K, D, B, H):
    """Codebooks above 64 codes accumulate the codebook gradient in an LDS window.  Until round 6 every wave added into every
    cell (4-6 % of the elements differed in their last bits from launch to launch, and Adam turns a sign decided by that into
    +- lr); now a cell belongs to one wave, which adds in position order: repeated launches are bit-equal, and equal to the
    float64 sum to rounding."""
    z = rnd(B, D, H, H, seed=1).to(DEV)
    cb = rnd(K, D, seed=2).to(DEV)
    idx = torch.cdist(z.permute(0, 2, 3, 1).reshape(-1, D), cb).argmin(1).reshape(B, H, H)
    g = rnd(B, D, H, H, seed=3).to(DEV)
    gl = torch.ones(1, device=DEV)
    outs = []
    for _ in range(4):
        dz, slabs = ops.vq_backward_slabs(z, cb, idx, g, gl, 0.25)
        outs.append((dz.clone(), ops.reduce_slabs(slabs, torch.empty_like(cb)).clone()))
    for dz, dw in outs[1:]:
        assert torch.equal(dz, outs[0][0]) and torch.equal(dw, outs[0][1])
    n = float(B * H * H * D)
    q = cb[idx.reshape(-1)].double()
    zf = z.permute(0, 2, 3, 1).reshape(-1, D).double()
    ref = torch.zeros(K, D, dtype=torch.float64, device=DEV).index_add_(0, idx.reshape(-1), (2.0 / n) * (q - zf))
    close(outs[0][1], ref.float(), 1e-5, 1e-5 * float(ref.abs().max()), "codebook gradient")


@pytest.mark.parametrize("B,mode,epi", [(3, 3, "bias+stats"), (5, 0, "none"), (2, 1, "gate+q"), (1, 2, "all"), (70, 3, "bias+stats"),
                                        (3, 4, "none"), (2, 4, "bias+stats")])
def test_stream_conv_4x4s2_32_to_64_weights_in_lds(ops, B, mode, epi):
    """wide_stream.hip: the wide encoder's second convolution (32 -> 64 channels, 64 x 64 -> 32 x 32) with all weights resident
    in LDS and the activations loaded straight into the matrix instruction's layout: two output rows per unit, the row seam
    between the two halves of a lane row, padding rows zeroed after the transform, every epilogue operand."""
    cin, nout, h, w = 32, 64, 64, 64
    x, x1 = rnd(B, cin, h, w, seed=1), rnd(B, cin, h, w, seed=2)
    coef = torch.stack([rnd(cin, seed=3).abs() + 0.5, rnd(cin, seed=4) * 0.2 if mode == 4 else torch.zeros(cin),
                        rnd(cin, seed=5) * 0.3 + 0.2, torch.zeros(cin)], 1)
    xin = load_ref(x.double(), mode, coef.double(), x1.double())
    wt = rnd(nout, cin, 4, 4, seed=6, scale=0.1)
    kw = {}
    bias = rnd(nout, seed=7) if epi in ("bias+stats", "all") else None
    ref = F.conv2d(xin, wt.double(), bias.double() if bias is not None else None, stride=2, padding=1)
    if bias is not None:
        kw.update(bias=bias.to(DEV))
    if epi == "all":
        kw.update(relu=True)
        ref = F.relu(ref)
    gate, q, resid = rnd(B, nout, 32, 32, seed=8), rnd(B, nout, 32, 32, seed=9), rnd(B, nout, 32, 32, seed=10)
    mcoef = torch.stack([rnd(nout, seed=11), torch.zeros(nout), rnd(nout, seed=12) * 0.3, torch.zeros(nout)], 1)
    if epi in ("gate+q", "all"):
        kw.update(mask=ops.Op(gate.to(DEV), 2, mcoef.to(DEV)))
        ref = ref * ((mcoef[:, 0].view(1, -1, 1, 1) * gate + mcoef[:, 2].view(1, -1, 1, 1)) > 0)
    sq = None
    if epi == "all":
        kw.update(resid=resid.to(DEV), stat_q=q.to(DEV))
        ref = ref + resid
        sq = q
    elif epi == "gate+q":
        kw.update(stat_q=kw["mask"].p0)
        sq = gate
    inp = ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, p1=x1.to(DEV) if mode == 4 else None)
    assert ops.conv4x4s2_plan(inp, B, cin, nout, h, w, stats=epi != "none", **kw).kernel == SW.KERNELS["conv_s2_wide_stream"]
    out, st = ops.conv4x4s2(inp, ops.weight_view(wt.to(DEV), cin * 16, 16, 4, 1),
                            B, cin, nout, h, w, want_stats=epi != "none", **kw)
    close(out, ref.float(), 5e-5, 5e-5, "stream conv 4x4/s2 32 -> 64")
    if st is not None:
        close_stats(st.sum(0), ref.float(), sq)


@pytest.mark.parametrize("B,mode,epi", [(3, 0, "bias+stats"), (2, 4, "gate+q"), (5, 3, "none"), (1, 4, "all"), (40, 0, "bias+stats")])
def test_stream_conv_transpose_64_to_32_weights_in_lds(ops, B, mode, epi):
    """wide_stream.hip: ConvTranspose2d(64 -> 32, 4, 2, 1) on a 32 x 32 grid with all weights resident in LDS -- forward form
    (bias, statistics) and data-gradient form (BatchNorm backward folded into an AFFINE2 load, gate, statistics against the
    gate's tensor): every (parity, tap) a matrix step, the lanes' pixel quads and their DPP neighbours, two rows per unit."""
    ci, co, h, w = 64, 32, 32, 32
    x, x1 = rnd(B, ci, h, w, seed=1), rnd(B, ci, h, w, seed=2)
    coef = torch.stack([rnd(ci, seed=3).abs() + 0.5, rnd(ci, seed=4) * 0.2, rnd(ci, seed=5) * 0.3 + 0.1, torch.zeros(ci)], 1)
    xin = load_ref(x.double(), mode, coef.double(), x1.double())
    wt = rnd(ci, co, 4, 4, seed=6, scale=0.1)
    kw = {}
    bias = rnd(co, seed=7) if epi in ("bias+stats", "all") else None
    ref = F.conv_transpose2d(xin, wt.double(), bias.double() if bias is not None else None, stride=2, padding=1)
    if bias is not None:
        kw.update(bias=bias.to(DEV))
    if epi == "all":
        kw.update(relu=True)
        ref = F.relu(ref)
    gate, q, resid = rnd(B, co, 64, 64, seed=8), rnd(B, co, 64, 64, seed=9), rnd(B, co, 64, 64, seed=10)
    mcoef = torch.stack([rnd(co, seed=11), torch.zeros(co), rnd(co, seed=12) * 0.3, torch.zeros(co)], 1)
    if epi in ("gate+q", "all"):
        kw.update(mask=ops.Op(gate.to(DEV), 2, mcoef.to(DEV)))
        ref = ref * ((mcoef[:, 0].view(1, -1, 1, 1) * gate + mcoef[:, 2].view(1, -1, 1, 1)) > 0)
    sq = None
    if epi == "all":
        kw.update(resid=resid.to(DEV), stat_q=q.to(DEV))
        ref = ref + resid
        sq = q
    elif epi == "gate+q":
        kw.update(stat_q=kw["mask"].p0)
        sq = gate
    inp = ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, p1=x1.to(DEV) if mode == 4 else None)
    assert ops.conv3x3_plan(inp, B, ci, 4 * co, h, w, taps=9, pixel_shuffle=True, stats=epi != "none",
                            **kw).kernel == SW.KERNELS["convT_wide_stream"]
    out, st = ops.conv3x3(inp, ops.weight_view(wt.to(DEV), 16, co * 16, 4, 1), B, ci, 4 * co, h, w, taps=9, pixel_shuffle=True,
                          want_stats=epi != "none", **kw)
    close(out, ref.float(), 5e-5, 5e-5, "stream conv transpose 64 -> 32")
    if st is not None:
        close_stats(st.sum(0), ref.float(), sq)


@pytest.mark.parametrize("B,mode,dgrad,epi", [(3, 1, False, "stats"), (2, 4, True, "all"), (5, 3, False, "none"), (1, 4, True, "all"),
                                              (40, 1, False, "stats")])
def test_stream_conv_3x3_64_channels_weights_in_lds(ops, B, mode, dgrad, epi):
    """wide_stream.hip: the wide residual blocks' 3x3 convolution (64 -> 64 on 32 x 32) with all weights resident in LDS --
    forward form (ReLU on the load, statistics) and data-gradient form (AFFINE2 load, transposed + flipped weight view, gate,
    residual, statistics against a third tensor)."""
    c, h = 64, 32
    x, x1 = rnd(B, c, h, h, seed=1), rnd(B, c, h, h, seed=2)
    coef = torch.stack([rnd(c, seed=3).abs() + 0.5, rnd(c, seed=4) * 0.2, rnd(c, seed=5) * 0.3, torch.zeros(c)], 1)
    xin = load_ref(x.double(), mode, coef.double(), x1.double())
    wt = rnd(c, c, 3, 3, seed=6, scale=0.05)
    inp = ops.Op(x.to(DEV), mode, coef.to(DEV) if mode >= 2 else None, p1=x1.to(DEV) if mode == 4 else None)
    if dgrad:
        xg = torch.zeros(B, c, h, h, dtype=torch.float64, requires_grad=True)
        F.conv2d(xg, wt.double(), None, padding=1).backward(xin)
        ref = xg.grad
        wv = ops.weight_view(wt.to(DEV), 9, c * 9, -3, -1, off=8)
    else:
        ref = F.conv2d(xin, wt.double(), None, padding=1)
        wv = ops.weight_view(wt.to(DEV), c * 9, 9, 3, 1)
    kw, sq = {}, None
    gate, q, resid = rnd(B, c, h, h, seed=8), rnd(B, c, h, h, seed=9), rnd(B, c, h, h, seed=10)
    if epi == "all":
        kw.update(mask=ops.Op(gate.to(DEV)), resid=resid.to(DEV), stat_q=q.to(DEV))
        ref = ref * (gate > 0) + resid
        sq = q
    assert ops.conv3x3_plan(inp, B, c, c, h, h, taps=9, stats=epi != "none", **kw).kernel == SW.KERNELS["conv3x3_wide_stream"]
    out, st = ops.conv3x3(inp, wv, B, c, c, h, h, taps=9, want_stats=epi != "none", **kw)
    close(out, ref.float(), 5e-5, 5e-5, "stream conv 3x3")
    if st is not None:
        close_stats(st.sum(0), ref.float(), sq)


@pytest.mark.parametrize("B,H,W,two", [(3, 32, 32, True), (2, 8, 16, False), (7, 16, 16, True), (70, 32, 32, True)])
def test_stream_conv1x1_backward_fused_64_channels(ops, B, H, W, two):
    """wide_stream.hip: dm_conv1x1_bwd_fused at 64 -> 64 channels (the wide residual blocks): data gradient with the layer
    input's ReLU gate, its (sum dx, sum dx * x) statistics and the weight gradient from one pass over the operands, every wave
    with its own slabs -- against float64."""
    C = 64
    dy, y = rnd(B, C, H, W, seed=1), rnd(B, C, H, W, seed=2)
    coef = torch.stack([rnd(C, seed=3), rnd(C, seed=4) * 0.1, rnd(C, seed=5) * 0.1, torch.zeros(C)], 1)
    x = rnd(B, C, H, W, seed=6)
    xcoef = torch.stack([rnd(C, seed=7).abs() + 0.5, torch.zeros(C), rnd(C, seed=8) * 0.3, torch.zeros(C)], 1)
    w = rnd(C, C, 1, 1, seed=9, scale=0.1)
    da = load_ref(dy.double(), 4, coef.double(), y.double()) if two else dy.double()
    t = xcoef[:, 0].double().view(1, -1, 1, 1) * x.double() + xcoef[:, 2].double().view(1, -1, 1, 1)
    xin = t.clamp(min=0).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    F.conv2d(xin, wd, None).backward(da)
    dx_ref = xin.grad * (t > 0)
    assert ops.conv1x1_bwd_fused_supported(C, C, H, W)
    dst = torch.empty(C, C, 1, 1, device=DEV)
    op = ops.Op(dy.to(DEV), 4, coef.to(DEV), p1=y.to(DEV)) if two else ops.Op(dy.to(DEV))
    assert ops.conv1x1_bwd_fused_plan(op, B, C, C, H, W).kernel == SW.KERNELS["conv1x1_bwd_wide_stream"]
    dx, st = ops.conv1x1_bwd_fused(op, x.to(DEV), xcoef.to(DEV), w.to(DEV), dst, B, C, C, H, W)
    close(dx, dx_ref.float(), 5e-5, 5e-5, "fused 1x1 backward: dx")
    close(dst, wd.grad.float(), 5e-5, 5e-5 * float(wd.grad.abs().max()), "fused 1x1 backward: dW")
    close_stats(st.sum(0), dx_ref.float(), x)


@pytest.mark.parametrize("B,tmode", [(3, 4), (1, 4), (40, 4), (2, 0)])
def test_wide_wgrad_one_pass_with_an_affine2_t_operand(ops, B, tmode):
    """dm_wgrad with T as an AFFINE2 operand (dm_wgrad_t_affine2_supported: the wide decoder's first transposed convolution, whose
    output gradient carries a BatchNorm backward): the one-pass kernel prefetches both tensors of T; elsewhere the call is refused."""
    cs, ct, hs = 64, 32, 32
    assert ops.wgrad_t_affine2_supported(cs, ct, hs, hs, 4) and not ops.wgrad_t_affine2_supported(64, 64, hs, hs, 3)
    s_ = rnd(B, cs, hs, hs, seed=1)
    t, t1 = rnd(B, ct, 2 * hs, 2 * hs, seed=2), rnd(B, ct, 2 * hs, 2 * hs, seed=3)
    tcoef = torch.stack([rnd(ct, seed=4), rnd(ct, seed=5) * 0.3, rnd(ct, seed=6) * 0.2, torch.zeros(ct)], 1)
    w = torch.zeros(cs, ct, 4, 4, requires_grad=True, dtype=torch.float64)
    F.conv2d(load_ref(t.double(), tmode, tcoef.double(), t1.double()), w, None, stride=2, padding=1).backward(s_.double())
    dst = torch.empty(cs, ct, 4, 4, device=DEV)
    top = ops.Op(t.to(DEV), tmode, tcoef.to(DEV) if tmode >= 2 else None, p1=t1.to(DEV) if tmode == 4 else None)
    assert ops.wgrad_plan(ops.Op(s_.to(DEV)), top, B, cs, ct, hs, hs, 4).kernel == SW.KERNELS["wgrad_wide1"]
    ops.wgrad(ops.Op(s_.to(DEV)), top, dst, B, cs, ct, hs, hs, 4)
    close(dst, w.grad.float(), 5e-5, 5e-5 * float(w.grad.abs().max()), "one-pass wgrad, AFFINE2 T")
    if tmode == 4:
        with pytest.raises(ValueError, match="AFFINE2"):
            ops.wgrad(ops.Op(rnd(2, 16, 16, 16, seed=1).to(DEV)), ops.Op(rnd(2, 16, 32, 32, seed=2).to(DEV), 4,
                      torch.zeros(16, 4, device=DEV), p1=rnd(2, 16, 32, 32, seed=3).to(DEV)), torch.empty(16, 16, 4, 4, device=DEV), 2, 16, 16, 16, 16, 4)
