"""tests/helpers/glue_reference.py on the host, before any kernel is judged by it: the float64 references against
torch.nn.BatchNorm2d / torch.optim.Adam in float64; every bound constant against an fp32 restatement of the kernel's
operation order over the grid the GPU test walks (the restatement must stay within a QUARTER of the bound, which is what
makes the constant a derived one; C_FIN and C_FIN_SHIFT are exact counts of one to five roundings and are held to the
bound itself); and the wrong kernels the grid must catch, each missing its bound by MUTATION_MARGIN somewhere.
The worst ratios are printed (pytest -s) and recorded next to the constants in the helper."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import glue_reference as G  # noqa: E402

QUARTER = 0.25


def ratio(got, ref, bound):
    got, ref = got.double(), ref.double()
    bad = ~torch.isfinite(got)
    r = ((got - ref).abs() / bound)
    r = torch.where(bad, torch.full_like(r, float("inf")), r)
    return float(torch.nan_to_num(r, nan=0.0).max())          # 0 / 0: an exact result under a zero bound


def report(name, worst, limit=QUARTER):
    print(f"[glue bound] {name}: worst restatement ratio {worst:.3f} (limit {limit})")
    assert worst <= limit, f"{name}: fp32 restatement at {worst:.3f} of the bound, limit {limit}"


# =========================================================================== the references are right
@pytest.mark.parametrize("shape", [(5, 6, 8, 8), (33, 3, 4, 12)])
def test_bn_references_match_float64_batchnorm(shape):
    B, Cn, H, W = shape
    gen = torch.Generator().manual_seed(B)
    a = torch.randn(shape, generator=gen, dtype=torch.float64) * 2 + 0.7
    dy = torch.randn(shape, generator=gen, dtype=torch.float64)
    bn = torch.nn.BatchNorm2d(Cn, eps=1e-3, momentum=0.25).double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(Cn, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(Cn, generator=gen))
        bn.running_mean.copy_(torch.randn(Cn, generator=gen))
        bn.running_var.copy_(torch.rand(Cn, generator=gen) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    bn.eps = G.f32(1e-3)     # momentum 0.25 is exact in fp32; eps 1e-3 is not: the module gets the value the ABI carries
    ar = a.clone().requires_grad_(True)
    bn(ar)
    sums = torch.stack([a.sum((0, 2, 3)), (a * a).sum((0, 2, 3))], -1)
    n = B * H * W
    y = bn(ar)            # (second call: running statistics move again -- compare against a second reference update)
    y.backward(dy)
    f1 = G.bn_finalize_ref(sums, n, bn.weight, bn.bias, rm0, rv0, 0.25, 1e-3)
    f2 = G.bn_finalize_ref(sums, n, bn.weight, bn.bias, f1["rm"], f1["rv"], 0.25, 1e-3)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(f2["rm"], bn.running_mean, **tol)
    torch.testing.assert_close(f2["rv"], bn.running_var, **tol)
    assert int(bn.num_batches_tracked) == 2
    sc, sh = f1["scale"].reshape(1, -1, 1, 1), f1["shift"].reshape(1, -1, 1, 1)
    torch.testing.assert_close(sc * a + sh, y.detach(), **tol)
    saved = torch.stack([f1["mean"], f1["invstd"]], -1)
    bsums = torch.stack([dy.sum((0, 2, 3)), (dy * a).sum((0, 2, 3))], -1)
    bw = G.bn_backward_ref(bsums, n, bn.weight, saved)
    torch.testing.assert_close(bw["dgamma"], bn.weight.grad, **tol)
    torch.testing.assert_close(bw["dbeta"], bn.bias.grad, **tol)
    c = lambda t: t.reshape(1, -1, 1, 1)                           # noqa: E731
    torch.testing.assert_close(c(bw["A"]) * dy + c(bw["Bc"]) * a + c(bw["Cc"]), ar.grad, **tol)
    # count == 0: fixed statistics, da = gamma invstd dy
    ev = G.bn_backward_ref(bsums, 0, bn.weight, saved)
    assert float(ev["Bc"].abs().max()) == 0.0 and float(ev["Cc"].abs().max()) == 0.0
    torch.testing.assert_close(ev["A"], bn.weight.detach() * f1["invstd"], **tol)
    ch = G.bn_apply_chain_ref(a, dy, bn.weight, bn.bias, 1e-3)
    torch.testing.assert_close(ch["y"], y.detach(), **tol)
    torch.testing.assert_close(ch["da"], ar.grad, **tol)
    torch.testing.assert_close(ch["dgamma"], bn.weight.grad, **tol)


def test_replay_reference_is_b_batch_of_one_calls():
    B, Cn, h = 9, 5, 6
    gen = torch.Generator().manual_seed(3)
    a = torch.randn(B, Cn, h, h, generator=gen, dtype=torch.float64) + 0.3
    bn = torch.nn.BatchNorm2d(Cn, momentum=0.25).double()
    with torch.no_grad():
        bn.running_mean.fill_(0.5)
        bn.running_var.fill_(2.0)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    for i in range(B):
        bn(a[i:i + 1])
    sums = torch.stack([a.sum((2, 3)), (a * a).sum((2, 3))], -1)
    rm, rv, b_rm, b_rv = G.bn_running_replay_ref(sums, h * h, rm0, rv0, 0.25)
    # (the reference feeds fp32-rounded statistics as the kernel does, the float64 module unrounded ones: U apart)
    assert ratio(rm, bn.running_mean, b_rm) <= 0.5 and ratio(rv, bn.running_var, b_rv) <= 0.5
    assert int(bn.num_batches_tracked) == B


def test_adam_reference_matches_float64_torch_adam():
    n = 4000
    for lr, b1, b2, eps in G.ADAM_HYPER:
        f = G.f32
        p0, _, _, _ = G.adam_state(n, 1, 1.0, 5)
        p = p0.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=f(lr), betas=(f(b1), f(b2)), eps=f(eps))
        mine = dict(p=p0.double(), m=torch.zeros(n, dtype=torch.float64), v=torch.zeros(n, dtype=torch.float64))
        for t in range(1, 6):
            g = torch.randn(n, generator=torch.Generator().manual_seed(40 + t), dtype=torch.float64) * 10.0 ** (t - 4)
            p.grad = g.clone()
            opt.step()
            mine = G.adam_ref(mine["p"], g, mine["m"], mine["v"], t, lr, b1, b2, eps)
            torch.testing.assert_close(mine["p"], p.detach(), rtol=1e-12, atol=1e-14)
        # a state pre-loaded at step 1e5
        st = opt.state[p]
        st["step"] = torch.tensor(99999.0)
        m0, v0 = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
        pb = p.detach().clone()
        p.grad = g.clone()
        opt.step()
        late = G.adam_ref(pb, g, m0, v0, 100000, lr, b1, b2, eps)
        torch.testing.assert_close(late["p"], p.detach(), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(late["v"], st["exp_avg_sq"], rtol=1e-12, atol=1e-30)


def test_recon_reference_is_the_model_loss():
    gen = torch.Generator().manual_seed(8)
    dec = torch.randn(3, 3, 8, 8, generator=gen, dtype=torch.float64).requires_grad_(True)
    x = torch.randn(3, 3, 8, 8, generator=gen, dtype=torch.float64)
    m = torch.randint(0, 3, (3, 1, 8, 8), generator=gen).double() / 2
    var = torch.tensor([0.05, 0.7, 4.0], dtype=torch.float64)
    loss = torch.mean(torch.nn.functional.mse_loss(dec * m, x * m, reduction="none") / var.reshape(1, 3, 1, 1))
    (loss * G.f32(1.3)).backward()
    ref = G.recon_loss_ref(dec, x, m, var, 1.3)
    torch.testing.assert_close(ref["loss"], loss.detach(), rtol=1e-13, atol=0)
    torch.testing.assert_close(ref["g"], dec.grad, rtol=1e-12, atol=1e-18)
    torch.testing.assert_close(ref["bias"], dec.grad.sum((0, 2, 3)), rtol=1e-12, atol=1e-16)


# =========================================================================== the constants, against the fp32 restatement
def test_c_stats_and_its_mutations():
    worst, caught = 0.0, {"drop_last_chunk": 0.0, "ignore_q": 0.0}
    for case in G.stats_cases():
        p, q = G.stats_inputs(case)
        s1, s2, b1, b2 = G.channel_stats_ref(p, q)
        got = G.channel_stats_f32(p, q).sum(0)
        worst = max(worst, ratio(got[:, 0], s1, b1), ratio(got[:, 1], s2, b2))
        bad = G.channel_stats_f32(p, q, drop_last_chunk=True).sum(0)
        caught["drop_last_chunk"] = max(caught["drop_last_chunk"], ratio(bad[:, 0], s1, b1), ratio(bad[:, 1], s2, b2))
        if q is not None:
            bad = G.channel_stats_f32(p, q, ignore_q=True).sum(0)
            caught["ignore_q"] = max(caught["ignore_q"], ratio(bad[:, 1], s2, b2))
    report("C_STATS", worst)
    for k, v in caught.items():
        assert v >= G.MUTATION_MARGIN, f"channel_stats mutation {k} only {v:.1f} bounds away"


def _finalize_f32(slabs, count, gamma, beta, rm, rv, momentum, eps, max_slabs=None, eps_outside=False):
    """bn_finalize_kernel on the host: double sums, then exactly its fp32 stores and fp32 products."""
    F = torch.float32
    s = slabs[:max_slabs].sum(0) if max_slabs else slabs.sum(0)
    n = float(count)
    mom, eps = G.f32(momentum), G.f32(eps)
    mean = s[:, 0] / n
    var = (s[:, 1] / n - mean * mean).clamp(min=0.0)
    mean_f = mean.to(F)
    invstd = ((1.0 / torch.sqrt(var) + eps) if eps_outside else 1.0 / torch.sqrt(var + eps)).to(F)
    g = torch.ones_like(mean_f) if gamma is None else gamma
    bt = torch.zeros_like(mean_f) if beta is None else beta
    scale = g * invstd
    shift = bt - mean_f * scale
    unb = n / (n - 1.0) if n > 1 else 1.0
    rm1 = (mom * mean + (1 - mom) * rm.double()).to(F)
    rv1 = (mom * (var * unb) + (1 - mom) * rv.double()).to(F)
    return dict(scale=scale, shift=shift, mean=mean_f, invstd=invstd, rm=rm1, rv=rv1)


def test_c_fin_on_synthetic_slabs_and_its_mutations():
    worst = {"C_FIN": 0.0, "C_FIN_SHIFT": 0.0}
    caught = {"slabs_beyond_1024_dropped": 0.0, "eps_outside_sqrt": 0.0}
    for nslabs, Cn, count, mom, eps, _form, k in G.finalize_grid():
        gen = torch.Generator().manual_seed(k)
        slabs = G.finalize_slabs(nslabs, Cn, count, k)
        gamma, beta = torch.rand(Cn, generator=gen) + 0.5, torch.randn(Cn, generator=gen)
        rm, rv = torch.randn(Cn, generator=gen), torch.rand(Cn, generator=gen) + 0.5
        ref = G.bn_finalize_ref(slabs.sum(0), count, gamma, beta, rm, rv, mom, eps)
        got = _finalize_f32(slabs, count, gamma, beta, rm, rv, mom, eps)
        for key in ("scale", "mean", "invstd", "rm", "rv"):
            worst["C_FIN"] = max(worst["C_FIN"], ratio(got[key], ref[key], ref["b_" + key]))
        worst["C_FIN_SHIFT"] = max(worst["C_FIN_SHIFT"], ratio(got["shift"], ref["shift"], ref["b_shift"]))
        bad = _finalize_f32(slabs, count, gamma, beta, rm, rv, mom, eps, max_slabs=1024)
        caught["slabs_beyond_1024_dropped"] = max(caught["slabs_beyond_1024_dropped"], ratio(bad["mean"], ref["mean"], ref["b_mean"]))
        bad = _finalize_f32(slabs, count, gamma, beta, rm, rv, mom, eps, eps_outside=True)
        caught["eps_outside_sqrt"] = max(caught["eps_outside_sqrt"], ratio(bad["invstd"], ref["invstd"], ref["b_invstd"]))
    report("C_FIN", worst["C_FIN"], 1.0)
    report("C_FIN_SHIFT", worst["C_FIN_SHIFT"], 1.0)
    for key, v in caught.items():
        assert v >= G.MUTATION_MARGIN, f"bn_finalize mutation {key} only {v:.1f} bounds away"


def test_c_replay_and_its_mutations():
    worst = 0.0
    caught = {"weights_shifted": 0.0, "biased_variance": 0.0, "count_one_unbias_inf": 0.0}
    for B, _spg, Cn, count, mom, k in G.per_sample_grid():
        gen = torch.Generator().manual_seed(100 + k)
        sums = G.synthetic_slabs(B, Cn, 100 + k) * count
        rm0, rv0 = torch.randn(Cn, generator=gen), torch.rand(Cn, generator=gen) + 0.5
        rm, rv, b_rm, b_rv = G.bn_running_replay_ref(sums, count, rm0, rv0, mom)
        gm, gv = G.bn_running_replay_closed(sums, count, rm0, rv0, mom)
        worst = max(worst, ratio(gm, rm, b_rm), ratio(gv, rv, b_rv))
        bm, bv = G.bn_running_replay_closed(sums, count, rm0, rv0, mom, weight_shift=1)
        caught["weights_shifted"] = max(caught["weights_shifted"], ratio(bm, rm, b_rm))
        if count > 1:
            _, bv = G.bn_running_replay_closed(sums, count, rm0, rv0, mom, biased=True)
            caught["biased_variance"] = max(caught["biased_variance"], ratio(bv, rv, b_rv))
        else:
            _, bv = G.bn_running_replay_closed(sums, count, rm0, rv0, mom, bad_unbias=True)
            caught["count_one_unbias_inf"] = max(caught["count_one_unbias_inf"], ratio(bv, rv, b_rv))
    report("C_REPLAY", worst)
    for key, v in caught.items():
        assert v >= G.MUTATION_MARGIN, f"replay mutation {key} only {v:.1f} bounds away"


def chain_f32(a, dy, gamma, beta, eps):
    """channel_stats -> bn_finalize -> apply and channel_stats(dy, a) -> bn_backward_finalize -> apply(AFFINE2), each step in
    the kernels' own precision on the host (batch mode)."""
    F = torch.float32
    n = a.numel() // a.shape[1]
    Cn = a.shape[1]
    fin = _finalize_f32(G.channel_stats_f32(a), n, gamma, beta, torch.zeros(Cn), torch.ones(Cn), 0.1, eps)
    c = lambda t: t.reshape(1, -1, 1, 1)                           # noqa: E731
    y = c(fin["scale"]) * a + c(fin["shift"])
    s = G.channel_stats_f32(dy, a).sum(0)
    mean, invstd, g = fin["mean"].double(), fin["invstd"].double(), gamma.double()
    dyxh = invstd * (s[:, 1] - mean * s[:, 0])
    scale = g * invstd
    c1, c2 = s[:, 0] / n, dyxh / n
    Bc = -scale * invstd * c2
    Cc = -scale * c1 - Bc * mean
    da = c(scale.to(F)) * dy + c(Bc.to(F)) * a + c(Cc.to(F))
    return y, da, dyxh.to(F), s[:, 0].to(F)


def test_c_var_and_c_bwd_on_the_chains():
    worst = {0.0: 0.0, 3.0: 0.0, 30.0: 0.0}
    for i, (B, Cn, h) in enumerate(G.CHAIN_SHAPES):
        for r in (0.0, 3.0, 30.0):
            a, dy, gamma, beta = G.chain_inputs(B, Cn, h, r, 300 + i)
            ref = G.bn_apply_chain_ref(a, dy, gamma, beta, 1e-5)
            y, da, dgamma, dbeta = chain_f32(a, dy, gamma, beta, 1e-5)
            worst[r] = max(worst[r], ratio(y, ref["y"], ref["b_y"]), ratio(da, ref["da"], ref["b_da"]),
                           ratio(dgamma, ref["dgamma"], ref["b_dgamma"]), ratio(dbeta, ref["dbeta"], ref["b_dbeta"]))
    for r, w in worst.items():
        report(f"C_VAR / C_BWD chain, r = {r:g}", w)


def test_reduce_order_and_its_mutation():
    worst, caught = 0.0, 0.0
    for n in (1, 15, 16, 17, 63, 64, 65, 512):
        for E in (1, 63, 64, 65):
            s = torch.randn(n, E, generator=torch.Generator().manual_seed(n * 100 + E))
            exact, bound, order = G.reduce_slabs_ref(s)
            worst = max(worst, ratio(order, exact, bound))
            caught = max(caught, ratio(G.reduce_order_f32(s, drop_partial_group=True), exact, bound))
    report("reduce_slabs (nslabs U sum|x|)", worst)
    assert caught >= G.MUTATION_MARGIN


def test_c_recon_and_its_mutations():
    worst = {"C_RECON": 0.0, "C_RECON_G": 0.0, "C_RECON_B": 0.0}
    caught = {"one_mask_factor": 0.0, "wrong_channel": 0.0}
    for i, (B, NIN, h, mc) in enumerate(G.RECON_CASES):
        dec, x, mask, var = G.recon_inputs(B, NIN, h, mc, 500 + i)
        ref = G.recon_loss_ref(dec, x, mask, var, 1.3)
        nb = G.recon_blocks(B, NIN)                                 # the launcher's own grid, nothing else
        loss, g, bias = G.recon_loss_f32(dec, x, mask, var, 1.3, nblocks=nb)
        worst["C_RECON"] = max(worst["C_RECON"], ratio(loss, ref["loss"], ref["b_loss"]))
        worst["C_RECON_G"] = max(worst["C_RECON_G"], ratio(g, ref["g"], ref["b_g"]))
        worst["C_RECON_B"] = max(worst["C_RECON_B"], ratio(bias, ref["bias"], ref["b_bias"]))
        if mask is not None:
            _, bg, _ = G.recon_loss_f32(dec, x, mask, var, 1.3, one_mask_factor=True)
            caught["one_mask_factor"] = max(caught["one_mask_factor"], float(((bg.double() - ref["g"]).abs() / (ref["b_g"] + 1e-300)).max()))
        # (only the cases with more than 1024 planes make a block cross channels: they are what catches this one)
        _, _, bb = G.recon_loss_f32(dec, x, mask, var, 1.3, nblocks=nb, wrong_channel=True)
        caught["wrong_channel"] = max(caught["wrong_channel"], ratio(bb, ref["bias"], ref["b_bias"]))
    for key, w in worst.items():
        report(key, w)
    for key, v in caught.items():
        assert v >= G.MUTATION_MARGIN, f"recon mutation {key} only {v:.1f} bounds away"


def test_c_adam_and_its_mutations():
    n = 20003
    worst = {"m": 0.0, "v": 0.0, "v_denormal": 0.0, "p": 0.0}
    caught = {"bc_t_minus_1": 0.0, "eps_inside": 0.0, "no_grad_scale": 0.0, "skip_tail": 0.0}
    for hi, (lr, b1, b2, eps) in enumerate(G.ADAM_HYPER):
        for t in G.ADAM_STEPS:
            for gi, gsc in enumerate(G.ADAM_GSCALES):
                p, g, m, v = G.adam_state(n, t, gsc, 1000 * hi + 10 * gi + int(math.log10(t)))
                for scale in ((1.0, 1.0 / 3) if gsc == 1.0 else (1.0,)):
                    ref = G.adam_ref(p, g, m, v, t, lr, b1, b2, eps, scale)
                    pn, mn, vn = G.adam_f32(p, g, m, v, t, lr, b1, b2, eps, scale)
                    worst["m"] = max(worst["m"], ratio(mn, ref["m"], ref["b_m"]))
                    normal = ref["v"] >= 2.0 ** -120             # below, the one denormal ulp of the bound is the bound
                    worst["v"] = max(worst["v"], ratio(vn[normal], ref["v"][normal], ref["b_v"][normal]) if normal.any() else 0.0)
                    worst["v_denormal"] = max(worst["v_denormal"], ratio(vn, ref["v"], ref["b_v"]))
                    worst["p"] = max(worst["p"], ratio(pn, ref["p"], ref["b_p"]))
                    for mut in caught:
                        if mut == "no_grad_scale" and scale == 1.0:
                            continue
                        if mut == "bc_t_minus_1" and t == 1:
                            continue                            # 1 - b^0 = 0: that wrong kernel divides by zero at step 1
                        bp, bm, bv = G.adam_f32(p, g, m, v, t, lr, b1, b2, eps, scale, mutation=mut)
                        if mut == "skip_tail":                  # the skipped tail shows in the moments (p moves by lr only)
                            caught[mut] = max(caught[mut], ratio(bm, ref["m"], ref["b_m"]), ratio(bv, ref["v"], ref["b_v"]))
                        else:
                            caught[mut] = max(caught[mut], ratio(bp, ref["p"], ref["b_p"]))
    report("C_ADAM_MV (m)", worst["m"])
    report("C_ADAM_MV (v)", worst["v"])
    report("C_ADAM_MV (v, denormal range: two products of half a denormal ulp each)", worst["v_denormal"], 1.0)
    report("C_ADAM_P", worst["p"])
    for key, v in caught.items():
        assert v >= G.MUTATION_MARGIN, f"Adam mutation {key} only {v:.1f} bounds away"
