"""`not gpu`: the cases of tests/helpers/vq_walk.py are what they claim to be -- dm_vq_forward_plan (host only; the
function the launch sizes its grid with) puts each on the named kernel with a grid that walks between two and three
rounds -- and the helper's references and slice arithmetic are right on a 2-sample stand-in.  tests/test_gpu_vq_walk.py
runs the cases."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import vq_walk as VW  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    assert (_lib.DM_VQ_AUTO, _lib.DM_VQ_MFMA) == (VW.DM_VQ_AUTO, VW.DM_VQ_MFMA)
    assert (_lib.DM_VQ_KERNEL_MFMA, _lib.DM_VQ_KERNEL_CELLS) == (VW.KERNEL_MFMA, VW.KERNEL_CELLS)
    return _lib.load()


def test_the_case_table():
    ids = [VW.case_id(c) for c in VW.CASES]
    assert len(set(ids)) == len(ids) == 37
    by = lambda **kw: [c for c in VW.CASES if all(getattr(c, k) == v for k, v in kw.items())]      # noqa: E731
    for filt in ("auto", "f32"):
        assert [c.K for c in by(section="streamed", filt=filt, D=16, H=8, W=24, B=2459)] == [40, 300, 1100, 1500]
        assert [c.K for c in by(section="streamed", filt=filt, D=32, H=8, W=24, B=1639)] == [40, 100, 600, 700]
        assert [c.K for c in by(section="streamed", filt=filt, D=64, H=8, W=24, B=819)] == [64]
        assert [c.K for c in by(section="streamed", filt=filt, D=64, H=8, W=24, B=1639)] == [128, 512, 576]
        assert len(by(section="streamed", filt=filt, D=64, K=512, H=32, W=32, B=300)) == 1
    assert [c.K for c in by(section="streamed", D=8, H=8, W=24, B=2459)] == [40, 300, 1100]
    assert not by(filt="auto", D=8)                                           # embedding_dim 8: the f32 filter only
    assert sorted(c.D for c in by(section="streamed", H=8, W=8)) == [8, 16, 32, 64]
    assert [(c.K, c.H, c.W) for c in by(section="cells")] == [(130, 8, 16), (777, 16, 24), (4096, 32, 32)]
    assert by(section="join") == [VW.Case("join", "auto", 16, 64, 16, 16, 1850)]
    # both parities of the streamed buffer count per round, per width and filter (embedding_dim 8: the odd one)
    for D in (16, 32, 64):
        for filt in ("auto", "f32"):
            n = [VW.stream_buffers(D, c.K, filt == "auto") for c in by(section="streamed", filt=filt, D=D)]
            streamed = [v for v in n if v > 2]
            assert any(v % 2 for v in streamed) and any(v % 2 == 0 for v in streamed), (D, filt, n)
    assert VW.stream_buffers(8, 1100, False) == 5 and VW.stream_buffers(16, 300, False) == 2
    assert (VW.stream_buffers(32, 600, False), VW.stream_buffers(32, 600, True)) == (5, 10)
    assert (VW.stream_buffers(32, 700, False), VW.stream_buffers(32, 700, True)) == (6, 11)


@pytest.mark.parametrize("case", VW.CASES, ids=VW.case_id)
def test_case_walks_between_two_and_three_rounds(lib, case):
    kind, grid, ppr = VW.plan(lib, case)
    VW.conditions(case, kind, grid, ppr)
    HW = case.H * case.W
    sl = VW.slices(case.B, HW)
    assert sl[0][0] == 0 and sl[-1][1] == case.B and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
    for b0, b1 in {sl[0], sl[-1]}:                        # (all but the last are the same size)
        assert 0 < (b1 - b0) * HW <= VW.SLICE_POSITIONS
        k, g, p = VW.plan(lib, case, B=b1 - b0)
        assert k == kind and (b1 - b0) * HW <= p, (VW.case_id(case), b0, b1, g, p)      # the same kernel, one round
    samples = VW.oracle_samples(case, ppr)
    assert len(samples) == 3 and samples[0] == 0 and samples[-1] == case.B - 1
    assert samples[1] * HW <= ppr < (samples[1] + 1) * HW


def test_slices():
    assert VW.slices(5, 192, 400) == [(0, 2), (2, 4), (4, 5)]
    assert VW.slices(4, 192, 384) == [(0, 2), (2, 4)]
    assert VW.slices(3, 1024, 100) == [(0, 1), (1, 2), (2, 3)]               # (a sample larger than the limit: one by one)
    assert VW.slices(2459, 192) == [(b, min(b + 341, 2459)) for b in range(0, 2459, 341)]


@pytest.mark.parametrize("case", [VW.CASES[1], VW.CASES[-2]], ids=VW.case_id)
def test_references_on_a_two_sample_stand_in(case):
    """The float64 squared error, the straight-through value and the per-slice sums, against element-wise arithmetic."""
    z, cb = VW.draw(case, B=2)
    assert z.shape == (2, case.D, case.H, case.W) and cb.shape == (case.K, case.D)
    assert torch.equal(z, VW.draw(case, B=2)[0])                                # seeded
    idx = VW.nearest_codes(z, cb)
    b, h, w = 1, case.H - 1, 3
    d = ((cb.double() - z[b, :, h, w].double()) ** 2).sum(1)
    assert int(idx[b, h, w]) == int(d.argmin()) and idx.shape == (2, case.H, case.W)
    q = VW.gather(cb, idx)
    assert torch.equal(q[b, :, h, w], cb[idx[b, h, w]])
    st = VW.straight_through(z, cb, idx)
    assert st.dtype == torch.float32 and torch.equal(st[b, :, h, w], z[b, :, h, w] + (cb[idx[b, h, w]] - z[b, :, h, w]))
    whole = VW.squared_error(z, cb, idx)
    ref = sum(float(((cb[idx[i]].double() - z[i].permute(1, 2, 0).double()) ** 2).sum()) for i in range(2))
    assert abs(whole - ref) <= 1e-12 * ref and abs(whole - float(d.min())) > 0
    sl = VW.slices(2, case.H * case.W, case.H * case.W)
    assert sl == [(0, 1), (1, 2)]
    parts = sum(VW.squared_error(z[a:e], cb, idx[a:e]) for a, e in sl)
    assert abs(parts - whole) <= 1e-12 * whole
    hist = torch.bincount(idx.flatten(), minlength=case.K)
    assert torch.equal(sum(torch.bincount(idx[a:e].flatten(), minlength=case.K) for a, e in sl), hist)
