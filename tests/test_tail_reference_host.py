"""tests/helpers/tail_reference.py on the host, before any kernel is judged by it: the float64 references against
torch.nn.functional + autograd in float64; the exactness proof of every exact output of every exact case (fp32 in two
summation orders and float64 must agree bit for bit); every bound against an fp32 evaluation on the host (within a QUARTER
of the bound); the cap on undecided gates; and the wrong kernels the grid must catch -- each differing from the reference on
an exact output, or missing a bound by MUTATION_MARGIN, on a case of the grid the GPU test walks.  The worst ratios and
the case that catches each mutation are printed (pytest -s)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import tail_reference as T  # noqa: E402

QUARTER = 0.25
F64 = dict(rtol=1e-11, atol=1e-12)


def ratio(got, ref, bound):
    r = (got.double() - ref.double()).abs() / bound
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    return float(torch.nan_to_num(r, nan=0.0).max())


def report(name, worst, limit=QUARTER):
    print(f"[tail bound] {name}: worst fp32 ratio {worst:.3f} (limit {limit})")
    assert worst <= limit, f"{name}: fp32 evaluation at {worst:.3f} of the bound, limit {limit}"


# =========================================================================== the references are right
@pytest.mark.parametrize("NIN,mc,hw", [(2, 1, (8, 64)), (3, 3, (16, 12)), (1, None, (8, 128))])
def test_dec_tail_reference_matches_float64_autograd(NIN, mc, hw):
    gen = torch.Generator().manual_seed(NIN)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)            # noqa: E731
    B, (h, w) = 2, hw
    pre = r(B, 4, h, w).requires_grad_(True)
    w4, b4 = (r(4, 4, 4, 4) * 0.3).requires_grad_(True), r(4).requires_grad_(True)
    w6, b6 = r(NIN, 4, 1, 1).requires_grad_(True), r(NIN).requires_grad_(True)
    x = r(B, NIN, 2 * h, 2 * w)
    mask = None if mc is None else torch.randint(0, 3, (B, mc, 2 * h, 2 * w), generator=gen).double() / 2
    var = torch.linspace(0.5, 1.5, NIN).double()
    d2 = F.relu(pre)
    d4 = F.relu(F.conv_transpose2d(d2, w4, b4, stride=2, padding=1))
    dec = F.conv2d(d4, w6, b6)
    mm = torch.ones_like(x) if mask is None else mask
    loss = torch.mean(F.mse_loss(dec * mm, x * mm, reduction="none") / var.reshape(1, -1, 1, 1))
    (loss * 0.5).backward()
    ref = T.dec_tail_ref(d2.detach(), w4, b4, w6, b6, x, mask, var, 0.5)
    torch.testing.assert_close(ref["decoded"], dec.detach(), **F64)
    torch.testing.assert_close(ref["loss"], loss.detach(), **F64)
    torch.testing.assert_close(ref["g2"], pre.grad, **F64)
    torch.testing.assert_close(ref["dW4"], w4.grad, **F64)
    torch.testing.assert_close(ref["dW6"], w6.grad.reshape(NIN, 4), **F64)
    torch.testing.assert_close(ref["db6"], b6.grad, **F64)
    torch.testing.assert_close(ref["db4"], b4.grad, **F64)
    torch.testing.assert_close(ref["db2"], pre.grad.sum((0, 2, 3)), **F64)


@pytest.mark.parametrize("C4,NIN,form", [(4, 2, "g"), (8, 3, "ge"), (16, 1, "e")])
def test_head_reference_matches_float64_autograd(C4, NIN, form):
    gen = torch.Generator().manual_seed(C4 + NIN)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)            # noqa: E731
    B, h = 2, 8
    pre = r(B, C4, h, h).requires_grad_(True)
    w6, b6 = r(NIN, C4, 1, 1).requires_grad_(True), r(NIN).requires_grad_(True)
    x, ext = r(B, NIN, h, h), r(B, NIN, h, h)
    mask = torch.randint(0, 3, (B, NIN, h, h), generator=gen).double() / 2
    var = torch.linspace(0.5, 1.5, NIN).double()
    d4 = F.relu(pre)
    dec = F.conv2d(d4, w6, b6)
    loss = torch.mean(F.mse_loss(dec * mask, x * mask, reduction="none") / var.reshape(1, -1, 1, 1))
    total = (loss * 0.5 if "g" in form else 0.0) + ((dec * ext).sum() if "e" in form else 0.0)
    total.backward()
    ref = T.head_ref(d4.detach(), w6, b6, x, mask, var, 0.5 if "g" in form else None, ext if "e" in form else None)
    torch.testing.assert_close(ref["decoded"], dec.detach(), **F64)
    torch.testing.assert_close(ref["loss"], loss.detach(), **F64)
    torch.testing.assert_close(ref["g4"], pre.grad, **F64)
    torch.testing.assert_close(ref["dW6"], w6.grad.reshape(NIN, C4), **F64)
    torch.testing.assert_close(ref["db6"], b6.grad, **F64)
    torch.testing.assert_close(ref["db4"], pre.grad.sum((0, 2, 3)), **F64)


@pytest.mark.parametrize("NIN,C0,C1", T.E1_SHAPES)
def test_e1_references_against_an_explicit_ones_channel(NIN, C0, C1):
    w0, b0, w1, b1, dweff = [t.double() for t in T.e1_inputs(NIN, C0, C1, "randn", 10 * C1 + NIN)]
    weff, _ = T.e1_compose_ref(w0, b0, w1)
    x = torch.randn(2, NIN, 12, 12, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    direct = F.conv2d(F.conv2d(x, w0, b0), w1, b1, stride=2, padding=1)
    ones = torch.cat([x, torch.ones(2, 1, 12, 12, dtype=torch.float64)], 1)
    torch.testing.assert_close(F.conv2d(ones, weff, b1, stride=2, padding=1), direct, **F64)
    table, _ = T.e1_compose_border_ref(w0, b0, w1, b1)
    cls = torch.tensor([0, 1, 1, 1, 1, 2])
    bias = table[cls][:, cls].permute(2, 0, 1).unsqueeze(0)                  # (1, C1, 6, 6)
    torch.testing.assert_close(F.conv2d(x, weff[:, :NIN], None, stride=2, padding=1) + bias, direct, **F64)
    # the chain rule: gradients of sum(dweff * Weff(w0, b0, w1)) by autograd
    p = [t.clone().requires_grad_(True) for t in (w0, b0, w1)]
    m = torch.cat([p[0].reshape(C0, NIN), p[1].reshape(-1, 1)], 1)
    (torch.einsum("ocyx,ci->oiyx", p[2], m) * dweff).sum().backward()
    ch = T.e1_chain_ref(dweff, w0, b0, w1)
    torch.testing.assert_close(ch["dw0"], p[0].grad.reshape(C0, NIN), **F64)
    torch.testing.assert_close(ch["db0"], p[1].grad, **F64)
    torch.testing.assert_close(ch["dw1"], p[2].grad, **F64)


# =========================================================================== exact cases: the proof
def _reordered_tail(a):
    """The same case in another summation order: channels of d2 / d4 reversed, the batch reversed, the image mirrored
    left-right (w4 mirrored along kx to match).  Returns the inputs and the map of its outputs back."""
    fl = lambda t, *dims: None if t is None else torch.flip(t, dims)              # noqa: E731
    b = dict(a, d2=fl(a["d2"], 0, 1, 3), w4=fl(a["w4"], 0, 1, 3), b4=fl(a["b4"], 0), w6=fl(a["w6"], 1), x=fl(a["x"], 0, 3),
             mask=fl(a["mask"], 0, 3))
    back = dict(decoded=lambda t: fl(t, 0, 3), g2=lambda t: fl(t, 0, 1, 3), dW4=lambda t: fl(t, 0, 1, 3),
                dW6=lambda t: fl(t, 1), db4=lambda t: fl(t, 0), db2=lambda t: fl(t, 0))
    return b, back


@pytest.mark.parametrize("case", [c for c in T.tail_cases() + T.tail_impulse_cases() if c["exact"]], ids=lambda c: c["name"])
def test_exact_tail_cases_are_exact(case):
    a = T.tail_inputs(case)
    ref = T.dec_tail_ref(**a, dyadic=True)
    one = T.dec_tail_ref(**a, dyadic=True, dtype=torch.float32)
    b, back = _reordered_tail(a)
    two = T.dec_tail_ref(**b, dyadic=True, dtype=torch.float32)
    for name in case["exact"]:
        r64 = ref[name]
        assert torch.equal(r64.float().double(), r64), f"{case['name']}: {name} is not an fp32 number"
        assert torch.equal(one[name].double(), r64), f"{case['name']}: {name} differs between fp32 and float64"
        t2 = back.get(name, lambda t: t)(two[name])
        assert torch.equal(t2.double(), r64), f"{case['name']}: {name} depends on the order of summation"
    if case["kind"].startswith("impulse"):
        assert float(ref["db6"].abs().max()) > 0 and float(ref["loss"]) > 0, "an impulse that reaches no gradient"
    assert float((ref["decoded"] == 0).double().mean()) < 1.0


@pytest.mark.parametrize("case", [c for c in T.head_cases() if c["exact"]], ids=lambda c: c["name"])
def test_exact_head_cases_are_exact(case):
    a = T.head_inputs(case)
    ref = T.head_ref(**a)
    one = T.head_ref(**a, dtype=torch.float32)
    fl = lambda t, *dims: None if t is None else torch.flip(t, dims)              # noqa: E731
    b = dict(a, d4=fl(a["d4"], 1), w6=fl(a["w6"], 1))
    two = T.head_ref(**b, dtype=torch.float32)
    for name in case["exact"]:
        t2 = fl(two[name], 1) if name == "g4" else two[name]
        assert torch.equal(one[name].double(), ref[name]) and torch.equal(t2.double(), ref[name]), (case["name"], name)


@pytest.mark.parametrize("NIN,C0,C1", T.E1_SHAPES)
def test_exact_e1_cases_are_exact(NIN, C0, C1):
    w0, b0, w1, b1, dweff = T.e1_inputs(NIN, C0, C1, "dyadic", 100 * C1 + NIN)
    weff, _ = T.e1_compose_ref(w0, b0, w1)
    table, _ = T.e1_compose_border_ref(w0, b0, w1, b1)
    ch = T.e1_chain_ref(dweff, w0, b0, w1)
    for name, v in (("weff", weff), ("table", table), ("dw0", ch["dw0"]), ("db0", ch["db0"]), ("dw1", ch["dw1"])):
        assert torch.equal(v.float().double(), v), f"{name} is not an fp32 number"
    m = torch.cat([w0.reshape(C0, NIN), b0.reshape(-1, 1)], 1)
    assert torch.equal(torch.einsum("ocyx,ci->oiyx", w1, m).double(), weff)           # fp32, ATen's order
    assert torch.equal(torch.einsum("ocyx,ci->oiyx", w1.flip(1), m.flip(0)).double(), weff)


# =========================================================================== bounded cases: a quarter of the bound, the cap
def test_tail_bounds_hold_an_fp32_evaluation_to_a_quarter_and_few_gates_are_undecided():
    worst = {}
    for case in T.tail_cases():
        a = T.tail_inputs(case)
        dy = case["kind"] != "randn"
        for fused in (True, False):
            ref = T.dec_tail_ref(**a, fused=fused, dyadic=dy)
            got = T.dec_tail_ref(**a, fused=fused, dyadic=dy, dtype=torch.float32)
            assert ref["undecided"] <= T.UNDECIDED_CAP, (case["name"], ref["undecided"])
            for name in T.TAIL_ALL:
                if name in case["exact"]:
                    continue
                worst[name] = max(worst.get(name, 0.0), ratio(got[name], ref[name], ref["b_" + name]))
    for name, w in worst.items():
        report("decoder tail " + name, w)


def test_head_bounds_hold_an_fp32_evaluation_to_a_quarter():
    worst = {}
    for case in T.head_cases():
        a = T.head_inputs(case)
        ref, got = T.head_ref(**a), T.head_ref(**a, dtype=torch.float32)
        for name in ("decoded", "g4") + T.HEAD_SUMS:
            if name not in case["exact"]:
                worst[name] = max(worst.get(name, 0.0), ratio(got[name], ref[name], ref["b_" + name]))
    for name, w in worst.items():
        report("head " + name, w)


# =========================================================================== the wrong kernels
def _caught(ref, bad, names, exact):
    """The output that tells `bad` from `ref`: an exact output that differs at all, or a bounded one beyond
    MUTATION_MARGIN bounds."""
    for name in names:
        if name in exact:
            if not torch.equal(bad[name].double(), ref[name].double()):
                return name + " (exact)"
        elif ratio(bad[name], ref[name], ref["b_" + name]) > T.MUTATION_MARGIN:
            return name
    return None


# what each launch hands the GPU test: a catch only counts on an output the wrong kernel itself would write
LAUNCH_OUTPUTS = dict(forward=("decoded", "loss"), backward=("g2", "dW4", "dW6", "db6", "db4", "db2"),
                      train=("g2", "loss", "dW4", "dW6", "db6", "db4", "db2"))
# the wrong kernels that exist as a wrong FORWARD kernel too (WIDE tiles, its own grid cap)
FORWARD_MUTATIONS = ("seam_d2_zero", "halo_row_d4", "halo_col_twice", "mask_ch0")


def _first_catch(mut, launch):
    fused = launch == "train"
    for case in sorted(T.tail_impulse_cases() + T.tail_cases(), key=lambda c: c["B"]):
        L = T.tail_launch(case["B"], case["NIN"], case["H2"], case["W2"], fused)
        if mut in ("stale_seam", "ownerless_slab") and not (L["ntiles"] > L["grid"] or L["nslabs"] > L["grid"]):
            continue
        a = T.tail_inputs(case)
        dy = case["kind"] != "randn"
        ref = T.dec_tail_ref(**a, fused=fused, dyadic=dy)
        bad = T.dec_tail_ref(**a, fused=fused, dyadic=dy, mut=mut)
        hit = _caught(ref, bad, LAUNCH_OUTPUTS[launch], case["exact"])
        if hit:
            return f"{case['name']} ({launch}, {L['tiling']}) on {hit}"
    return None


@pytest.mark.parametrize("mut", T.TAIL_MUTATIONS)
def test_tail_mutations_are_caught(mut):
    """Every wrong kernel is caught on an output of the launch that would be wrong: the training form (EDGE at multiples of
    64) or the backward that is not fused (WIDE), and -- where the forward kernel has the same code -- the forward."""
    hits = {launch: _first_catch(mut, launch) for launch in ("train", "backward")}
    if mut in FORWARD_MUTATIONS:
        hits["forward"] = _first_catch(mut, "forward")
        assert hits["forward"], f"no case tells the wrong forward kernel '{mut}' from the reference"
    for launch, hit in hits.items():
        print(f"[tail mutation] {mut}: " + (f"caught by {hit}" if hit else f"does not apply to / is not caught through {launch}"))
    assert hits["train"] or hits["backward"], f"no case of the grid tells the wrong kernel '{mut}' from the reference"
    if mut in ("stale_seam",):
        assert hits["train"], "the EDGE read-ahead belongs to the training form"


@pytest.mark.parametrize("mut", T.HEAD_MUTATIONS)
def test_head_mutations_are_caught(mut):
    for case in sorted(T.head_cases(), key=lambda c: (mut != "skip_second_pass") * c["B"]):
        a = T.head_inputs(case)
        ref, bad = T.head_ref(**a), T.head_ref(**a, mut=mut)
        hit = _caught(ref, bad, ("decoded", "g4") + T.HEAD_SUMS, case["exact"])
        if hit:
            print(f"[tail mutation] head {mut}: caught by {case['name']} on {hit}")
            return
    pytest.fail(f"no head case tells the wrong kernel '{mut}' from the reference")


def test_border_table_mutation_is_caught():
    NIN, C0, C1 = T.E1_SHAPES[0]
    w0, b0, w1, b1, _ = T.e1_inputs(NIN, C0, C1, "dyadic", 100 * C1 + NIN)
    ref, _ = T.e1_compose_border_ref(w0, b0, w1, b1)
    bad, _ = T.e1_compose_border_ref(w0, b0, w1, b1, mut="no_b0_corner")
    assert not torch.equal(ref, bad)
    print(f"[tail mutation] border table without enc.0's bias in class (0, 0): caught by the exact case {(NIN, C0, C1)}")


# =========================================================================== latent tail
# (ids as they were while a second entry form, from enc.4's output, existed: "-False" is the (a3, coef3) form)
@pytest.mark.parametrize("nres", [0, 4, 2, 1], ids=lambda nres: f"{nres}-False")
def test_latent_tail_reference_matches_batch_of_one_batchnorm(nres):
    B, C = 5, 16
    a = T.lt_inputs(B, nres)
    ref = T.latent_tail_ref(**a)
    dd = T.d
    bn = lambda v, g, b, eps: F.batch_norm(v, None, None, dd(g), dd(b), True, 0.1, T.f32(eps))   # noqa: E731
    for i in range(B):
        c3 = dd(a["coef3"])
        t = torch.relu(c3[i, :, 0].reshape(1, C, 1, 1) * dd(a["a3"])[i:i + 1] + c3[i, :, 2].reshape(1, C, 1, 1))
        a4 = F.conv2d(t, dd(a["w10"]), dd(a["b10"]), padding=1)
        per = [a4]
        h = bn(a4, a["gamma4"], a["beta4"], a["eps4"])
        for wa, ba, ga, bea, ea, wb, bb, gb, beb, eb in a["res"]:
            ra = F.conv2d(torch.relu(h), dd(wa), dd(ba), padding=1)
            rb = F.conv2d(torch.relu(bn(ra, ga, bea, ea)), dd(wb).reshape(16, 32, 1, 1), dd(bb))
            per += [ra, rb]
            h = h + bn(rb, gb, beb, eb)
        torch.testing.assert_close(ref["z"][i:i + 1], h, rtol=1e-9, atol=1e-10 * float(ref["z"][i].abs().max()))
        assert len(per) == len(ref["stats"])
        for v, (name, s, _) in zip(per, ref["stats"]):
            want = torch.stack([v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))], 1)
            torch.testing.assert_close(s[i], want, rtol=1e-10, atol=1e-11 * float(want.abs().max()))


LT_HOST = [(2, 0), (2, 4), (513, 4), (600, 2), (1025, 1)]


def test_latent_tail_bounds_hold_an_fp32_evaluation_to_a_quarter_and_stay_a_check():
    worst = {}
    for (B, nres) in LT_HOST:
        a = T.lt_inputs(B, nres)
        ref, got = T.latent_tail_ref(**a), T.latent_tail_ref(**a, dtype=torch.float32)
        worst["z"] = max(worst.get("z", 0.0), ratio(got["z"], ref["z"], ref["b_z"]))
        for (name, s, bs), (_, s32, _) in zip(ref["stats"], got["stats"]):
            worst["statistics"] = max(worst.get("statistics", 0.0), ratio(s32, s, bs))
        # the bound stays a check for every patch, the small ones included: well under a percent of the patch's own z
        rel = float((ref["b_z"].amax((1, 2, 3)) / ref["z"].abs().amax((1, 2, 3))).max())
        print(f"[tail bound] latent tail B={B} nres={nres}: bound / max|z| per patch up to {rel:.1e}")
        assert rel < 5e-3, rel
        # patch b and patch b + 512 differ in scale
        if B > 512:
            sc = T.lt_patch_scale(B)
            assert bool((sc[512:] != sc[:B - 512]).all())
    for name, w in worst.items():
        report("latent tail " + name, w)


@pytest.mark.parametrize("mut", T.LT_MUTATIONS)
def test_latent_tail_mutations_are_caught(mut):
    for (B, nres) in LT_HOST:
        a = T.lt_inputs(B, nres)
        ref, bad = T.latent_tail_ref(**a), T.latent_tail_ref(**a, mut=mut)
        hit = "z" if ratio(bad["z"], ref["z"], ref["b_z"]) > T.MUTATION_MARGIN else None
        for (name, s, bs), (_, sb, _) in zip(ref["stats"], bad["stats"]):
            if ratio(sb, s, bs) > T.MUTATION_MARGIN:
                hit = hit or name
        if hit:
            print(f"[tail mutation] latent tail {mut}: caught by B={B} nres={nres} on {hit}")
            return
    pytest.fail(f"no latent-tail case tells the wrong kernel '{mut}' from the reference")


# =========================================================================== the grids reach what they claim
def test_grids_cross_every_cap():
    per = {}
    for case in T.tail_cases() + T.tail_impulse_cases():
        for fused in (True, False):
            L = T.tail_launch(case["B"], case["NIN"], case["H2"], case["W2"], fused)
            assert L["per_wg"] <= 4, "the row counts of the sums' bounds assume at most four tiles a workgroup"
            occ = T.tail_bwd_occ(case["NIN"], L["tiling"])
            key = (L["tiling"], occ)
            st = per.setdefault(key, set())
            st.add("below" if L["ntiles"] < 256 * occ else ("above_bwd" if L["ntiles"] <= 768 else "above_768"))
            if L["nslabs"] > L["grid"]:
                st.add("ownerless")
    for key in (("full", 3), ("full", 2), ("wide", 2), ("edge", 2)):
        assert "below" in per[key] and "above_768" in per[key], (key, per[key])
        if key[1] == 2:
            assert "above_bwd" in per[key] and "ownerless" in per[key], (key, per[key])
    assert {b for b, _ in T.lt_cases()} >= {1, 2, 511, 512, 513, 600, 1025} and len(T.lt_cases()) == 35
    # an impulse in a LATER tile of a workgroup, per tiling and per launch
    later = set()
    for case in T.tail_impulse_cases():
        for launch, fused in (("train", True), ("backward", False), ("forward", False)):
            t, grid = T.impulse_tiles(case, fused, forward=launch == "forward")
            if t >= grid:
                later.add((launch, T.tail_launch(case["B"], case["NIN"], case["H2"], case["W2"], fused)["tiling"], case["kind"]))
    for kind in ("impulse_d2", "impulse_x"):
        for key in (("train", "full"), ("train", "edge"), ("backward", "full"), ("backward", "wide"), ("forward", "full"),
                    ("forward", "wide")):
            assert key + (kind,) in later, (key, kind, sorted(later))


def test_every_instantiation_is_reached():
    """The backward dispatch has NIN 1 .. 4 x masked / not x {64 wide, WIDE, EDGE} x fused / not (EDGE: fused only); the
    forward NIN x {64 wide, WIDE}; the head C4 x NIN.  Both mask layouts (1 and NIN channels) must meet every tiling."""
    seen, masks = set(), set()
    for case in T.tail_cases() + T.tail_impulse_cases():
        for fused in (True, False):
            L = T.tail_launch(case["B"], case["NIN"], case["H2"], case["W2"], fused)
            seen.add((case["NIN"], case["mask"] is not None, L["tiling"], fused))
            masks.add((case["mask"], L["tiling"]))
    want = {(n, m, t, f) for n in (1, 2, 3, 4) for m in (False, True) for (t, f) in
            (("full", True), ("full", False), ("wide", True), ("wide", False), ("edge", True))}
    assert want <= seen, sorted(want - seen)
    assert {(m, t) for m in (None, 1, "nin") for t in ("full", "wide", "edge")} <= masks
    hs = {(c["C4"], c["NIN"]) for c in T.head_cases()}
    assert hs >= {(c4, n) for c4 in (4, 8, 16) for n in (1, 2, 3, 4)}
    hm = {(c["C4"], c["mask"]) for c in T.head_cases()} | set()
    assert hm >= {(c4, m) for c4 in (4, 8, 16) for m in (None, 1, "nin")}
    assert {(c["C4"], c["form"]) for c in T.head_cases()} >= {(c4, f) for c4 in (4, 8, 16) for f in ("g", "e", "ge")}
