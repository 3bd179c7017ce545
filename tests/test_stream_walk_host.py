"""`not gpu`: the cases of tests/helpers/stream_walk.py are what they claim to be.  The launch plans (host only; the decision
code the launches themselves read) put each case on the named streaming kernel with a grid whose walkers take two units or
more, unevenly, across sample boundaries and border classes; the batch slices the GPU test compares against are one-unit
launches of the same kernel; and the cases of tests/test_gpu_kernels.py that are filed under "stream" tests run the kernel the
table says.  tests/test_gpu_stream_walk.py runs the cases."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import stream_walk as SW  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib, ops as o
    for name, value in SW.KERNELS.items():
        assert getattr(_lib, "DM_KERNEL_" + name.upper()) == value, name
    assert (_lib.DM_DEAL_RANGE_STRIDED, _lib.DM_DEAL_RANGE, _lib.DM_DEAL_GRID_STRIDED) == (SW.DEAL_RANGE_STRIDED, SW.DEAL_RANGE,
                                                                                          SW.DEAL_GRID_STRIDED)
    assert tuple(getattr(_lib, "DM_LOAD_" + n) for n in ("IDENT", "RELU", "AFFINE", "AFFINE_RELU", "AFFINE2")) == tuple(range(5))
    return o


def test_the_case_table():
    ids = [SW.case_id(c) for c in SW.CASES]
    assert len(set(ids)) == len(ids) == 44
    assert len(SW.CONV_CASES) + len(SW.BWD_CASES) + len(SW.WGRAD_CASES) == len(SW.CASES)
    by = lambda k: [c for c in SW.CASES if c.kernel == k]      # noqa: E731
    # one kernel value per streaming kernel and one for wgrad_wide1, every one with cases
    assert {c.kernel for c in SW.CASES} == {k for k, v in SW.KERNELS.items() if v >= 16}
    c1 = by("conv1x1_stream")
    for pair in ((64, 64), (32, 64), (64, 32), (32, 32)):
        assert {(c.mode, c.epi) for c in c1 if (c.a, c.b) == pair} >= {(SW.AFFINE_RELU, "stats"), (SW.AFFINE2, "gate+q")}
        for ring in (SW.AFFINE2, SW.RELU):
            assert [c for c in by("wgrad1x1_stream") if (c.a, c.b, c.mode) == pair + (ring,)]
    assert {c.epi for c in c1} == {"stats", "gate+q", "bias+relu+resid"}
    assert sorted((c.a, c.b) for c in by("conv_s2_thin_stream")) == [(1, 32), (2, 32), (2, 64), (2, 64), (3, 32), (4, 32)]
    assert {c.epi for c in by("conv_s2_thin_stream")} == {"bias+stats", "gate+q"}
    assert sorted(c.b for c in by("convT_thin_stream")) == [1, 2]
    assert {c.mode for c in by("conv_s2_wide_stream")} == {SW.IDENT, SW.AFFINE_RELU, SW.AFFINE2}
    assert {c.mode for c in by("convT_wide_stream")} == {SW.IDENT, SW.AFFINE2}
    assert {(c.mode, c.epi) for c in by("conv3x3_wide_stream")} == {(SW.RELU, "stats"), (SW.AFFINE2, "all")}
    assert {c.mode for c in by("conv1x1_bwd_wide_stream")} == {SW.IDENT, SW.AFFINE2}
    assert sorted(c.b for c in by("wgrad_s2_thin_stream")) == [1, 1, 2, 3, 4]
    assert {(c.k, c.b, c.mode, c.mode2) for c in by("wgrad_wide1")} >= {(3, 64, SW.AFFINE2, SW.RELU), (4, 32, SW.AFFINE2, SW.IDENT),
                                                                        (4, 32, SW.IDENT, SW.AFFINE2)}


def test_walker_units_on_hand_made_plans():
    P = __import__("collections").namedtuple("P", "kernel workgroups waves walkers dealing ring units")
    p = P(0, 3, 4, 4, SW.DEAL_RANGE_STRIDED, 0, 20)         # ranges [0, 6), [6, 13), [13, 20)
    assert [list(SW.walker_units(p, v)) for v in range(4)] == [[0, 4], [1, 5], [2], [3]]
    assert [list(SW.walker_units(p, v)) for v in range(4, 8)] == [[6, 10], [7, 11], [8, 12], [9]]
    p = P(0, 2, 4, 4, SW.DEAL_RANGE, 0, 11)                 # walker v: [11 v / 8, 11 (v + 1) / 8)
    assert [list(SW.walker_units(p, v)) for v in range(8)] == [[0], [1], [2, 3], [4], [5], [6, 7], [8], [9, 10]]
    p = P(0, 2, 8, 1, SW.DEAL_GRID_STRIDED, 0, 5)
    assert [list(SW.walker_units(p, v)) for v in range(2)] == [[0, 2, 4], [1, 3]]
    p = P(0, 3, 4, 1, SW.DEAL_RANGE, 2, 10)                 # a workgroup that walks together: one walker each
    assert [list(SW.walker_units(p, v)) for v in range(3)] == [[0, 1, 2], [3, 4, 5], [6, 7, 8, 9]]
    assert SW.max_units_per_walker(p) == 4 and SW.walkers(p) == 3
    assert SW.slices(5, 2) == [(0, 2), (2, 4), (4, 5)] and SW.slices(4, 4) == [(0, 4)]
    assert [SW.border_class(r, 4) for r in range(4)] == ["top", "interior", "interior", "bottom"]


@pytest.mark.parametrize("case", SW.CASES, ids=SW.case_id)
def test_case_walks_several_units_per_walker(ops, case):
    p = SW.plan(ops, case)
    SW.conditions(case, p)
    # the slices of the GPU test: the same kernel, at most one unit per walker, and one sample more would be two
    per = SW.slice_batch(ops, case)
    assert 1 <= per < case.B
    sl = SW.slices(case.B, per)
    assert sl[0][0] == 0 and sl[-1][1] == case.B and all(a[1] == b[0] for a, b in zip(sl, sl[1:])) and len(sl) >= 3
    for b0, b1 in {sl[0], sl[-1]}:
        q = SW.plan(ops, case, B=b1 - b0)
        assert q.kernel == p.kernel and q.dealing == p.dealing and SW.max_units_per_walker(q) <= 1, (SW.case_id(case), q)
    assert SW.max_units_per_walker(SW.plan(ops, case, B=per + 1)) == 2
    samples = SW.reference_samples(case, p)
    assert samples[0] == 0 and samples[-1] == case.B - 1 and 3 <= len(samples) <= 4 and 0 < samples[-2] < case.B - 1


def test_plans_follow_the_operands(ops):
    """The same shape leaves the streaming kernel when an operand is one it does not take -- the plan reads the operand
    structs, not the shape alone."""
    K = SW.KERNELS
    assert ops.conv3x3_plan(SW.AFFINE_RELU, 2600, 64, 64, 8, 16, taps=1, stats=True).kernel == K["conv1x1_stream"]
    assert ops.conv3x3_plan(SW.AFFINE_RELU, 2600, 64, 64, 8, 16, taps=1, stats=True, per_sample=True).kernel == K["wide_tiled"]
    assert ops.conv3x3_plan(SW.AFFINE_RELU, 2600, 64, 64, 8, 16, taps=1, stats=True, per_tile=True).kernel == K["wide_tiled"]
    assert ops.conv3x3_plan(SW.AFFINE_RELU, 2600, 64, 64, 8, 16, taps=1, stats=True, scratch=False).kernel == K["generic"]
    assert ops.conv3x3_plan(SW.IDENT, 2600, 64, 64, 8, 16, taps=1, mask=SW.AFFINE).kernel == K["conv1x1_stream"]
    assert ops.conv3x3_plan(SW.IDENT, 2600, 64, 64, 8, 16, taps=1, mask=SW.AFFINE, per_sample=False,
                            **{}).workgroups == 512
    # statistics cap the grid at the slab count the caller allocates (here 2 tiles of 8 x 16: two workgroups)
    assert ops.conv3x3_plan(SW.IDENT, 2, 64, 64, 8, 16, taps=1, stats=True).workgroups == 1
    assert ops.conv3x3_plan(SW.IDENT, 16, 64, 64, 8, 16, taps=1, stats=True).workgroups == 8
    assert ops.conv4x4s2_plan(SW.IDENT, 800, 3, 32, 16, 128).kernel == K["conv_s2_thin_stream"]
    assert ops.conv4x4s2_plan(SW.AFFINE2, 800, 3, 32, 16, 128).kernel == K["wide_tiled"]
    assert ops.conv4x4s2_plan(SW.IDENT, 800, 3, 32, 16, 128, ones=True).kernel == K["wide_tiled"]
    assert ops.conv4x4s2_plan(SW.IDENT, 800, 3, 32, 16, 128, bias_border=True).kernel == K["wide_tiled"]
    assert ops.conv4x4s2_plan(SW.AFFINE_RELU, 8, 16, 16, 32, 32, stats=True).kernel == K["patch"]
    assert ops.conv4x4s2_plan(SW.AFFINE_RELU, 8, 16, 16, 32, 32, stats=True, mask=SW.IDENT).kernel == K["resident"]
    assert ops.conv3x3_plan(SW.IDENT, 4100, 12, 4, 8, 64, pixel_shuffle=True, bias=True).kernel == K["convT_thin_stream"]
    assert ops.conv3x3_plan(SW.IDENT, 4100, 8, 4, 8, 64, pixel_shuffle=True, bias=True).kernel == K["resident"]
    assert ops.conv3x3_plan(SW.IDENT, 4100, 12, 4, 8, 64, pixel_shuffle=True, stats=True).kernel == K["wide_tiled"]
    assert ops.conv3x3_plan(SW.RELU, 300, 64, 64, 32, 32, stats=True).kernel == K["conv3x3_wide_stream"]
    assert ops.conv3x3_plan(SW.RELU, 300, 64, 64, 16, 16, stats=True).kernel == K["wide_tiled"]
    assert ops.wgrad_plan(SW.AFFINE2, SW.IDENT, 1100, 64, 64, 8, 16, 1).kernel == K["wgrad1x1_stream"]
    assert ops.wgrad_plan(SW.AFFINE2, SW.IDENT, 1100, 64, 64, 8, 16, 1, per_sample=True).kernel == K["wide_tiled"]
    assert ops.wgrad_plan(SW.IDENT, SW.IDENT, 1100, 64, 48, 8, 16, 1).kernel == K["wide_tiled"]
    assert ops.wgrad_plan(SW.IDENT, SW.IDENT, 2000, 32, 3, 8, 32, 4, t_ones=True).kernel == K["wide_tiled"]
    assert ops.wgrad_plan(SW.IDENT, SW.IDENT, 800, 64, 64, 8, 16, 3, per_sample=True).kernel == K["wgrad_wide1"]     # (IDENT: no coefficients)
    assert ops.wgrad_plan(SW.AFFINE, SW.IDENT, 800, 64, 64, 8, 16, 3, per_sample=True).kernel == K["wide_tiled"]
    assert ops.wgrad_plan(SW.IDENT, SW.IDENT, 800, 16, 16, 16, 16, 3).kernel == K["resident"]
    assert ops.wgrad_plan(SW.IDENT, SW.IDENT, 8, 12, 20, 10, 10, 4).kernel == K["generic"]
    assert ops.conv1x1_bwd_fused_plan(SW.AFFINE2, 26, 16, 32, 16, 16).kernel == K["conv1x1_bwd_tiled"]
    with pytest.raises(ValueError, match="AFFINE2"):
        ops.wgrad_plan(SW.IDENT, SW.AFFINE2, 800, 64, 64, 8, 16, 3)        # refused as the launch refuses it
    with pytest.raises(ValueError, match="not built"):
        ops.conv1x1_bwd_fused_plan(SW.AFFINE2, 26, 16, 16, 16, 16)
    with pytest.raises(ValueError, match="even"):
        ops.conv4x4s2_plan(SW.IDENT, 2, 3, 32, 15, 128)


def test_plan_grids_are_the_slab_counts_the_callers_allocate(ops):
    """No grid moved: the plan's walkers are the slab counts dm_*_num_blocks report for the slabbed kernels."""
    from dynamorph_amd import _lib
    lib = _lib.load()
    for c in SW.WGRAD_CASES:
        p = SW.plan(ops, c)
        assert p.workgroups == lib.dm_wgrad_num_blocks(c.B, c.a, c.b, c.h, c.w, c.k), SW.case_id(c)
    for c in SW.BWD_CASES:
        p = SW.plan(ops, c)
        assert p.workgroups * p.walkers == lib.dm_conv1x1_bwd_fused_num_blocks(c.B, c.a, c.b, c.h, c.w)
    for B in (1, 3, 100, 513, 2600):
        assert ops.conv1x1_bwd_fused_plan(SW.IDENT, B, 64, 64, 8, 16).workgroups * 4 == lib.dm_conv1x1_bwd_fused_num_blocks(B, 64, 64, 8, 16)
        assert ops.wgrad_plan(0, 0, B, 64, 64, 8, 16, 1).workgroups == lib.dm_wgrad_num_blocks(B, 64, 64, 8, 16, 1)


def test_16_output_channels_never_reach_the_thin_stride_2_stream_kernel(ops):
    """conv_s2_thin_stream_kernel<CIN, 1> (16 output channels) is not reachable through dm_conv4x4s2: the streaming kernel needs
    128 input columns and a wide-tileable base grid (H % 16 == 0), at which a register-resident kernel takes 1-4 -> 16 channels;
    the operands that kernel refuses (an AFFINE2 input, the border-bias table beside side inputs) the streaming kernel refuses
    too.  DESIGN.md section 3.2e records it."""
    seen = set()
    for H in range(2, 130, 2):
        for cin in (1, 2, 3, 4):
            for mode in range(5):
                for kw in ({}, dict(stats=True), dict(mask=SW.AFFINE, stat_q="gate", stats=True), dict(bias_border=True),
                           dict(bias_border=True, mask=SW.AFFINE), dict(per_tile=True, stats=True), dict(scratch=False)):
                    for B in (1, 2, 300):
                        seen.add(ops.conv4x4s2_plan(mode, B, cin, 16, H, 128, **kw).kernel)
    assert SW.KERNELS["conv_s2_thin_stream"] not in seen and SW.KERNELS["resident"] in seen
    assert ops.conv4x4s2_plan(SW.IDENT, 2, 2, 32, 16, 128).kernel == SW.KERNELS["conv_s2_thin_stream"]


def test_old_stream_cases_run_the_kernel_the_table_says(ops):
    for (B, cin, nout, h, w, mode, epi), kernel in SW.OLD_S2_THIN.items():
        kw = {"bias": dict(bias=True), "none": {}, "gate": dict(mask=SW.AFFINE), "gate+q": dict(mask=SW.AFFINE, stat_q="gate"),
              "all": dict(bias=True, relu=True, mask=SW.AFFINE, resid=True, stat_q=True)}[epi]
        p = ops.conv4x4s2_plan(mode, B, cin, nout, h, w, stats=epi != "none", **kw)
        assert p.kernel == SW.KERNELS[kernel], (B, cin, nout, h, w, mode, epi, p)
    for (B, ci, co, h, mode, relu), kernel in SW.OLD_CONVT_THIN.items():
        p = ops.conv3x3_plan(mode, B, ci, 4 * co, h, 64, taps=9, pixel_shuffle=True, bias=True, relu=relu)
        assert p.kernel == SW.KERNELS[kernel], (B, ci, co, h, mode, relu, p)
