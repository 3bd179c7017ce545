"""Runs the cases of tests/helpers/operand_contract.py on the device through the C ABI (the ctypes structs of
dynamorph_amd._lib, so that a case can set every field: a weight view without scratch, a mask that aliases stat_q, a
sentinel slab past the declared ones).

As a script: `operand_contract_run.py ENV OUT.json` runs every case of the routes marked ENV (the process was started with
that route's switches, which the library reads once) and writes {case id: [ok, message]} to OUT.json."""
import ctypes as C
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from dynamorph_amd import _lib as L  # noqa: E402
import operand_contract as OC  # noqa: E402
import operand_contract_fused as FC  # noqa: E402

NAN = float("nan")


def _d(t):
    return None if t is None else t.contiguous().cuda()


def _p(t):
    return None if t is None else t.data_ptr()


def _operand(p0, mode, coef, p1, ones, per_sample):
    bstride = coef.shape[1] * 4 if (per_sample and coef is not None) else 0
    return L.Operand(_p(p0), _p(p1), _p(coef), bstride, mode, 1 if ones else 0)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64)


def _check_close(name, got, ref, bound):
    got = got.double().cpu()
    if torch.isnan(got).any():
        return f"{name}: {int(torch.isnan(got).sum())} of {got.numel()} elements unwritten (NaN pre-fill left)"
    err = (got - ref).abs()
    bad = err > bound
    if bad.any():
        i = int((err / bound).flatten().argmax())
        return (f"{name}: {int(bad.sum())} of {got.numel()} beyond the bound; worst at flat {i}: got {got.flatten()[i]:.7g} "
                f"ref {ref.flatten()[i]:.7g} err {err.flatten()[i]:.3g} bound {bound.flatten()[i]:.3g}")
    return None


def run_case(case):
    """(ok, message): the call matched the reference within the bound, or was refused, exactly as the table says."""
    route = OC.ROUTE[case.route]
    lib = L.load()
    X = OC.make_inputs(case)
    stream = torch.cuda.current_stream().cuda_stream
    f = case.feats
    keep = []                 # the device copies stay alive until the call has been checked
    if route.entry == "wgrad":
        G = X["geom"]
        B, CS, CT, Hs, Ws, k = G["B"], G["CS"], G["CT"], G["Hs"], G["Ws"], G["k"]
        S, T = _d(X["S"]), _d(X["T"])
        sc, tc, sp1, tp1 = _d(X.get("scoef")), _d(X.get("tcoef")), _d(X.get("sp1")), _d(X.get("tp1"))
        keep += [S, T, sc, tc, sp1, tp1]
        so = _operand(S, OC._mode(f, "smode"), sc, sp1, "sones" in f, "sps" in f)
        to = _operand(T, OC._mode(f, "tmode"), tc, tp1, "tones" in f, "tps" in f)
        nb = lib.dm_wgrad_num_blocks(B, CS, CT, Hs, Ws, k)
        if case.B == OC.persistent_B(route) and not nb < OC.declared_units(route, B)[0]:
            return False, f"persistent-grid case: {nb} slabs for {OC.declared_units(route, B)[0]} units"
        E = CS * CT * k * k
        slabs = torch.full((nb + 1, E), NAN, device="cuda")
        slabs[nb] = OC.SENTINEL
        dst = torch.full((E,), NAN, device="cuda")
        pre = (slabs.clone(), dst.clone())
        rc = lib.dm_wgrad(C.byref(so), C.byref(to), _p(slabs), _p(dst), B, CS, CT, Hs, Ws, k, stream)
        return _verdict(case, rc, lib, [("dst", dst, pre[1]), ("slabs", slabs, pre[0])],
                        lambda R: [("weight gradient", dst, R["out"].flatten(), R["out_bound"].flatten())],
                        X, slabs, nb)
    if route.entry == "apply":
        G = X["geom"]
        x, cf, p1, res = _d(X["x"]), _d(X.get("coef")), _d(X.get("p1")), _d(X.get("resid"))
        keep += [x, cf, p1, res]
        o = _operand(x, OC._mode(f, "mode"), cf, p1, "ones" in f, "ps" in f)
        out = torch.full((G["B"], G["C"], G["H"], G["W"]), NAN, device="cuda")
        pre = out.clone()
        rc = lib.dm_apply(C.byref(o), _p(res), _p(out), G["B"], G["C"], G["H"], G["W"], stream)
        return _verdict(case, rc, lib, [("out", out, pre)],
                        lambda R: [("out", out, R["out"], R["out_bound"])], X, None, 0)
    big = route.entry != "apply" and case.B == OC.persistent_B(route)
    G = X["geom"]
    B, CIN, NOUT, H, W, taps, co = G["B"], G["CIN"], G["NOUT"], G["H"], G["W"], G["taps"], G["co"]
    x, cf, p1 = _d(X["x"]), _d(X.get("coef")), _d(X.get("p1"))
    wflat = _d(X["wflat"])
    keep += [x, cf, p1, wflat]
    o = _operand(x, OC._mode(f, "mode"), cf, p1, "ones" in f, "ps" in f)
    per_tile = 1 if "per_tile" in f else 0
    pix = 1 if route.entry == "pix" else 0
    if route.entry == "s2":
        nb = lib.dm_conv4x4s2_num_blocks(B, CIN, NOUT, H, W, per_tile)
        nscr = lib.dm_conv4x4s2_scratch_floats(CIN, NOUT, H, W, 1)
    else:
        nb = lib.dm_conv3x3_num_blocks(B, CIN, NOUT, H, W, taps, pix, per_tile)
        nscr = lib.dm_conv3x3_scratch_floats(CIN, NOUT, H, W, taps, pix, per_tile)
    if big and "per_tile" not in route.base and not nb < OC.declared_units(route, B)[0]:
        return False, f"persistent-grid case: {nb} slabs for {OC.declared_units(route, B)[0]} units"
    scratch = torch.empty(max(nscr, 1), device="cuda") if (route.scratch and nscr > 0) else None
    keep.append(scratch)
    off, sn, sc_, sky, skx = X["wview"]
    wv = L.WeightView(_p(wflat), off, sn, sc_, sky, skx, _p(scratch), nscr if scratch is not None else 0)
    mask = _d(X.get("mask"))
    mcoef = _d(X.get("mcoef"))
    keep += [mask, mcoef]
    if mask is None:
        mo = L.Operand(None, None, None, 0, 0, 0)
    else:
        mmode = 2 if f & {"mask_aff", "mask_aff_ps"} else 0
        mp1 = None
        if "mask_relu" in f:
            mmode = 1
        if "mask_affine2" in f:
            mmode, mp1 = 4, mask
        if "mask_affine_relu" in f:
            mmode = 3
        mo = _operand(mask, mmode, mcoef, mp1, "mask_ones" in f, "mask_aff_ps" in f)
    bias, border, resid, stat_q = _d(X.get("bias")), _d(X.get("bias_border")), _d(X.get("resid")), _d(X.get("stat_q"))
    keep += [bias, border, resid, stat_q]
    if "stat_q_mask" in f:
        stat_q = mask
    stats = None
    if "stats" in f:
        stats = torch.full((nb + 1, co, 2), NAN, device="cuda", dtype=torch.float64)
        stats[nb] = OC.SENTINEL
    ep = L.Epilogue(_p(bias), _p(border), 1 if "relu" in f else 0, per_tile, mo, _p(resid), _p(stat_q), _p(stats))
    out = torch.full((B, co, G["Ho"], G["Wo"]), NAN, device="cuda")
    pre = [("out", out, out.clone())] + ([("stats", stats, stats.clone())] if stats is not None else [])
    if route.entry == "s2":
        rc = lib.dm_conv4x4s2(C.byref(o), C.byref(wv), _p(out), C.byref(ep), B, CIN, NOUT, H, W, stream)
    else:
        rc = lib.dm_conv3x3(C.byref(o), C.byref(wv), _p(out), C.byref(ep), B, CIN, NOUT, H, W, taps, pix, stream)

    def compare(R):
        items = [("out", out, R["out"], R["out_bound"])]
        if stats is not None:
            st = stats[:nb]
            if per_tile:
                if nb % B:
                    return [("stats", None, f"per-tile slabs: {nb} slabs do not group by {B} samples", None)]
                st = st.view(B, nb // B, co, 2).sum(1)
            else:
                st = st.sum(0)
            items.append(("stats", st, R["stats"], R["stats_bound"]))
            items.append(("declared slabs", stats[:nb], None, None))
        return items
    return _verdict(case, rc, lib, pre, compare, X, stats, nb)


def _verdict(case, rc, lib, pre, compare, X, slabs, nb, reference=OC.reference):
    torch.cuda.synchronize()
    if case.expect == "refuse":
        if rc > 0:
            return False, f"expected a refusal ({case.why}), got HIP error {rc}"
        if rc == 0:
            msg = _compare(compare(reference(case, X)), nb)
            return False, f"expected a refusal ({case.why}), got rc 0 and " + (f"a WRONG result: {msg}" if msg else "a result within the bound")
        if not lib.dm_last_error():
            return False, "refused without a dm_last_error message"
        for name, t, p in pre:
            if not torch.equal(_bits(t), _bits(p)):
                return False, f"refused (rc {rc}) but {name} was written"
        return True, f"refused: {lib.dm_last_error().decode()}"
    if rc != 0:
        return False, f"expected a match, got rc {rc}: {lib.dm_last_error().decode()}"
    msg = _compare(compare(reference(case, X)), nb)
    if msg:
        return False, msg
    if slabs is not None and not bool((slabs[nb] == OC.SENTINEL).all()):
        return False, "the slab past the declared ones was written"
    return True, "match"


def run_fused(case):
    """(ok, message) of one fused backward case: dx, the statistics slabs and the weight-gradient slabs against float64,
    every declared slab written, the slab past them untouched; or a refusal that wrote nothing."""
    lib = L.load()
    name, entry, shape, _ = FC.FROUTE[case.route]
    X = FC.make_fused_inputs(case)
    G = X["geom"]
    B, CD, CX, H, W = G["B"], G["CD"], G["CX"], G["H"], G["W"]
    f = case.feats
    stream = torch.cuda.current_stream().cuda_stream
    keep = {k: _d(v) for k, v in X.items() if isinstance(v, torch.Tensor)}
    g = keep.get
    if entry == "convt":
        nb = lib.dm_convt_bwd_fused_num_blocks(B, CD, CX, H, W)
        dx = torch.full((B, CD, H, W), NAN, device="cuda")
        nx = CD
    else:
        nb = {"bwd_s2": lib.dm_conv_bwd_s2_fused_num_blocks, "c1x1": lib.dm_conv1x1_bwd_fused_num_blocks,
              "c3x3": lib.dm_conv3x3_bwd_fused_num_blocks, "c4s2": lib.dm_conv4x4s2_bwd_fused_num_blocks}[entry](B, CD, CX, H, W)
        dx = torch.full((B, CX, G["xh"], G["xw"]), NAN, device="cuda")
        nx = CX
    if nb <= 0:
        return False, f"num_blocks {nb} for a built shape"
    E = X["w"].numel()
    wsl = torch.full((nb + 1, E), NAN, device="cuda")
    wsl[nb] = OC.SENTINEL
    stats = None
    if "no_stats" not in f:
        stats = torch.full((nb + 1, nx, 2), NAN, device="cuda", dtype=torch.float64)
        stats[nb] = OC.SENTINEL
    pre = [("dx", dx, dx.clone()), ("wslabs", wsl, wsl.clone())] + ([("stats", stats, stats.clone())] if stats is not None else [])
    if entry == "convt":
        rc = lib.dm_convt_bwd_fused(_p(g("S")), _p(g("G")), _p(g("w")), _p(dx), _p(stats), _p(wsl),
                                    1 if "mask_relu" in f else 0, B, CD, CX, H, W, stream)
    else:
        dy = _operand(g("dy"), FC._dy_mode(f), g("dycoef"), g("dyp1"), "dy_ones" in f, "dy_ps" in f)
        if entry == "bwd_s2":
            tmode = 0 if "in0" in f else (4 if "in4" in f else 3)
            tin = _operand(g("x"), tmode, g("xcoef"), g("xp1"), False, "in_ps" in f)
            mask = _operand(g("x"), 2 if "mask_aff" in f else 0, g("xcoef"), None, False, False)
            wv = L.WeightView(_p(g("w")), 0, 16, CX * 16, 4, 1, None, 0)
            ep = L.Epilogue(None, None, 0, 0, mask, _p(g("resid")), None if "no_stat_q" in f else _p(g("x")), _p(stats))
            rc = lib.dm_conv_bwd_s2_fused(C.byref(dy), C.byref(tin), C.byref(wv), _p(dx), C.byref(ep), _p(wsl), B, CD, CX, H, W,
                                          stream)
        elif entry == "c1x1":
            rc = lib.dm_conv1x1_bwd_fused(C.byref(dy), _p(g("x")), _p(g("xcoef")), _p(g("w")), _p(dx), _p(stats), _p(wsl),
                                          B, CD, CX, H, W, stream)
        elif entry == "c3x3":
            rc = lib.dm_conv3x3_bwd_fused(C.byref(dy), _p(g("x")), _p(g("xcoef")), _p(g("w")), _p(g("resid")), _p(g("q")),
                                          _p(dx), _p(stats), _p(wsl), B, CD, CX, H, W, stream)
        else:
            rc = lib.dm_conv4x4s2_bwd_fused(C.byref(dy), _p(g("x")), _p(g("xcoef")), _p(g("w")), _p(dx), _p(stats), _p(wsl),
                                            B, CD, CX, H, W, stream)

    def compare(R):
        items = [("dx", dx, R["dx"], R["dx_bound"]), ("weight gradient", wsl[:nb].sum(0, dtype=torch.float64),
                                                        R["dw"].flatten(), R["dw_bound"].flatten())]
        if stats is not None:
            items += [("stats", stats[:nb].sum(0), R["stats"], R["stats_bound"]), ("declared slabs", stats[:nb], None, None)]
        items.append(("declared weight slabs", wsl[:nb], None, None))
        return items
    torch.cuda.synchronize()
    if case.expect == "refuse":
        return _verdict(case, rc, lib, pre, compare, X, None, nb, reference=FC.fused_reference)
    ok, msg = _verdict(case, rc, lib, pre, compare, X, None, nb, reference=FC.fused_reference)
    if ok and not (bool((wsl[nb] == OC.SENTINEL).all()) and (stats is None or bool((stats[nb] == OC.SENTINEL).all()))):
        return False, "the slab past the declared ones was written"
    return ok, msg


def _compare(items, nb):
    """None when every declared output is written and within its bound, else what is not."""
    for name, got, ref, bound in items:
        if got is None:
            return ref
        if ref is None:                       # declared slabs: every one written
            if torch.isnan(got).any():
                return f"{name}: {int(torch.isnan(got).any(-1).any(-1).sum())} of {nb} slabs left unwritten"
            continue
        msg = _check_close(name, got, ref, bound)
        if msg:
            return msg
    return None


def main():
    env, path = sys.argv[1], sys.argv[2]
    res = {}
    for case in OC.all_cases(env):
        try:
            res[case.id] = list(run_case(case))
        except Exception as e:          # a host-side error of one case must not hide the others' results
            res[case.id] = [False, f"{type(e).__name__}: {e}"]
    with open(path, "w") as fh:
        json.dump(res, fh)


if __name__ == "__main__":
    main()
