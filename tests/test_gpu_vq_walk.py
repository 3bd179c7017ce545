"""The quantiser's persistent forward kernels over SEVERAL ROUNDS of their grid (cases and reasons: tests/helpers/vq_walk.py;
the cases' claims are asserted on the host by tests/test_vq_walk_host.py and again here).

Per case one call of the variant on the whole batch -- between two and three rounds -- is held to
  * the DM_VQ_EXACT kernel (no loop; held to the C oracle at these widths by test_vq_forward_vs_c_oracle) on every position,
    and the C oracle itself on the first sample, the sample workgroup 0's second round starts in, and the last;
  * z + (codebook[idx] - z) in fp32 bit for bit, bincount(idx), the float64 squared error (1e-6 relative, the gate of
    test_vq_forward_vs_c_oracle);
  * the same variant on consecutive batch slices of at most 65536 positions, ONE round each: the same bits, and re-check
    counts that ADD UP to the whole run's.  The exact re-check makes every code right even when the filter's scores are
    garbage -- the kernel only gets slower -- so a filter that breaks from the second round on passes every comparison of
    codes; whether a position takes the exact path depends on its latents and the codebook alone, so the count does not.
The share of re-checked positions is printed, not capped (HISTORY.md records it)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vq_walk as VW  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from dynamorph_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from dynamorph_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cvq():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    return ctypes.CDLL(os.path.join(ROOT, "oracle", "libvq_oracle.so"))


def _c_oracle_idx(cvq, z, cb):
    z, cb = np.ascontiguousarray(z), np.ascontiguousarray(cb)
    B, D, H, W = z.shape
    idx_ref = np.empty((B, H, W), np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    cvq.oracle_vq_encode(p(z), p(cb), p(idx_ref), B, D, cb.shape[0], H, W)
    return idx_ref


def _bits(t):
    return t.view(torch.int32)


def _planned(lib, case):
    kind, grid, ppr = VW.plan(lib, case)
    VW.conditions(case, kind, grid, ppr)
    return kind, grid, ppr


@pytest.mark.parametrize("case", [c for c in VW.CASES if c.section != "join"], ids=VW.case_id)
def test_vq_forward_over_several_rounds(ops, lib, cvq, case):
    kind, grid, ppr = _planned(lib, case)
    z, cb = VW.draw(case)
    zd, cbd = z.to(DEV), cb.to(DEV)
    P, HW, K = VW.positions(case), case.H * case.W, case.K
    idx, out, slabs, hist, nre = ops.vq_forward(zd, cbd, variant=VW.variant(case), want_rechecked=True)
    nre = int(nre.cpu())

    # codes (before anything gathers with them)
    idx_e = ops.vq_forward(zd, cbd, want_out=False, variant=VW.DM_VQ_EXACT)[0]
    bad = (idx != idx_e).flatten().nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {P} codes differ from the exact kernel's, first at position {int(bad[0])} " \
                             f"(round {int(bad[0]) // ppr}, {ppr} positions per round)"
    idx_h = idx.cpu().numpy()
    for b in VW.oracle_samples(case, ppr):
        assert np.array_equal(idx_h[b:b + 1], _c_oracle_idx(cvq, z[b:b + 1].numpy(), cb.numpy())), f"sample {b}"

    # values and counters
    assert torch.equal(_bits(out), _bits(VW.straight_through(zd, cbd, idx)))
    assert torch.equal(hist.long(), torch.bincount(idx.flatten(), minlength=K))
    sse, sse_ref = float(slabs.sum().cpu()), VW.squared_error(zd, cbd, idx)
    print(f"{VW.case_id(case)}: squared error {sse:.9e}, float64 {sse_ref:.9e}, relative {abs(sse - sse_ref) / sse_ref:.2e}")
    assert abs(sse - sse_ref) <= 1e-6 * sse_ref

    # the filter: one round per slice, the same bits, re-check counts that add up
    counts = []
    for b0, b1 in VW.slices(case.B, HW):
        k1, g1, p1 = VW.plan(lib, case, B=b1 - b0)
        assert k1 == kind and (b1 - b0) * HW <= min(p1, VW.SLICE_POSITIONS), (b0, b1, k1, g1, p1)
        idx_s, out_s, _, _, nre_s = ops.vq_forward(zd[b0:b1], cbd, variant=VW.variant(case), want_rechecked=True)
        counts.append(int(nre_s.cpu()))
        assert torch.equal(idx_s, idx[b0:b1]), (b0, b1)
        assert torch.equal(_bits(out_s), _bits(out[b0:b1])), (b0, b1)
    print(f"{VW.case_id(case)}: kernel {kind}, {grid} workgroups, {P / ppr:.2f} rounds; re-checked exactly: whole run {nre} "
          f"({nre / P:.3e} of {P}), {len(counts)} one-round slices {sum(counts)} ({sum(counts) / P:.3e})")
    assert sum(counts) == nre, (nre, counts)


def test_vq_forward_join_over_several_rounds(ops, lib):
    """dm_vq_forward_join on a grid that walks between two and three rounds, as test_vq_forward_join_equals_apply_then_vq
    holds it at one: latents, codes, straight-through values, squared-error slabs and the counter rows (code counts and,
    column 64, the re-check count of every workgroup) bit-equal to dm_apply followed by dm_vq_forward; codes equal to the
    exact kernel's on those latents."""
    from dynamorph_amd._lib import DM_LOAD_AFFINE
    case, = [c for c in VW.CASES if c.section == "join"]
    kind, grid, ppr = _planned(lib, case)
    B, D, K, H, W = case.B, case.D, case.K, case.H, case.W
    P = B * H * W
    rb, cb = VW.draw(case)
    h = torch.randn(B, D, H, W, generator=torch.Generator().manual_seed(B + K + 1))
    coef = torch.zeros(D, 4)
    coef[:, 0] = torch.randn(D, generator=torch.Generator().manual_seed(3)).abs() + 0.5
    coef[:, 1] = 123.0                                   # (unused by the AFFINE transform)
    coef[:, 2] = torch.randn(D, generator=torch.Generator().manual_seed(4))
    rb, h, coef, cb = rb.to(DEV), h.to(DEV), coef.to(DEV), cb.to(DEV)
    assert ops.vq_forward_join_supported(D, K, H, W)
    z_ref = ops.apply(ops.Op(rb, DM_LOAD_AFFINE, coef), B, D, H, W, resid=h)
    idx_r, out_r, slabs_r, ws_r = ops.vq_forward(z_ref, cb, want_hist=False)
    idx, out, slabs, ws, z = ops.vq_forward_join(rb, h, coef, cb)
    assert torch.equal(_bits(z), _bits(z_ref))
    idx_e = ops.vq_forward(z_ref, cb, want_out=False, variant=VW.DM_VQ_EXACT)[0]
    assert torch.equal(idx, idx_e) and torch.equal(idx, idx_r)
    assert torch.equal(_bits(out), _bits(out_r)) and torch.equal(_bits(out), _bits(VW.straight_through(z_ref, cb, idx)))
    assert torch.equal(slabs, slabs_r)
    sse, sse_ref = float(slabs.sum().cpu()), VW.squared_error(z_ref, cb, idx)
    assert abs(sse - sse_ref) <= 1e-6 * sse_ref
    ls = torch.zeros(4, dtype=torch.float64, device=DEV)
    a = ops.vq_loss_finalize(slabs, ws, K, D, P, 0.25, ls, 10, 1.0, 1.0)
    b = ops.vq_loss_finalize(slabs_r, ws_r, K, D, P, 0.25, ls, 10, 1.0, 1.0)
    assert torch.equal(a, b)
    # at most 64 codes: the workspace ends with 1024 counter rows of 72 ints, one per workgroup (test_cabi.py pins the layout)
    rows, rows_r = (_bits(w)[-1024 * 72:].view(1024, 72)[:grid, :65] for w in (ws, ws_r))
    assert torch.equal(rows[:, :64].sum(0), torch.bincount(idx.flatten(), minlength=64)[:64])
    assert torch.equal(rows, rows_r)
    nre = int(rows[:, 64].sum())
    # ... and the one-round slices of the latents re-check as many positions as the whole run
    counts = []
    for b0, b1 in VW.slices(B, H * W):
        k1, g1, p1 = VW.plan(lib, case, B=b1 - b0)
        assert k1 == kind and (b1 - b0) * H * W <= min(p1, VW.SLICE_POSITIONS)
        idx_s, _, _, _, nre_s = ops.vq_forward(z_ref[b0:b1], cb, want_out=False, want_rechecked=True)
        counts.append(int(nre_s.cpu()))
        assert torch.equal(idx_s, idx[b0:b1])
    print(f"{VW.case_id(case)}: kernel {kind}, {grid} workgroups, {P / ppr:.2f} rounds; re-checked exactly: whole run {nre} "
          f"({nre / P:.3e} of {P}), {len(counts)} one-round slices {sum(counts)} ({sum(counts) / P:.3e})")
    assert sum(counts) == nre, (nre, counts)
