#!/usr/bin/env python3
"""The partial eigensolver behind the PCA fits (csrc/eig.hip, dynamorph_amd/eig.py), everything resident:

  apply     dm_eig_apply beside torch.matmul(A, Q) (rocBLAS) on the same operands per (n, b): 8 n^2 / t against the 6.29 TB/s
            copy rate, 2 n^2 b / t, and whether the two products agree to the summation bound.
  step      one Rayleigh-Ritz step of the driver at (n, b), split into the application and the torch glue (QR, block
            products, the b x b eigh, the read-back).
  finalize  pca.finalize (order F) and pca.finalize_samples (order N) with eigensolver="partial" beside "full" -- the parent's
            eigh -- on the same matrices: the planted spectra of tests/helpers/pca_fixture.py scaled up.
  fit       whole fits, partial beside full: WidePCA(0.5) at F = 65536, PCA(0.5) at F = 4096, init="pca" (two components).

Medians of device-event times after a warm-up of the same shape, the candidates taking turns inside every repetition.  Prints
one JSON line per record.

    timeout -k 10 900 python tools/eigbench.py --out profiles/eig_eigbench.jsonl
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dynamorph_amd import eig, ops  # noqa: E402
from dynamorph_amd import pca as P  # noqa: E402
from dynamorph_amd.umap_layout import pca_coordinates  # noqa: E402

HBM_RATE = 6.29e12              # bytes/s, measured float4 copy (8.0e12 datasheet)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def alternated(fns, reps, warm=1):
    """{name: (median, min, max)} of device-event times, the candidates taking turns within every repetition."""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in fns}
    for _ in range(reps):
        for n, fn in fns.items():
            ts[n].append(timed(fn))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in ts.items()}


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def planted_rows(N, F, dev, seed=0, n_planted=40):
    """tests/helpers/pca_fixture.py's recipe at any size, fp32 on the device: 40 planted directions of strength 96 .. 18, unit
    noise of +-32 / 1024 and a common offset."""
    g = torch.Generator(device=dev).manual_seed(seed)
    s = torch.arange(96, 96 - 2 * n_planted, -2, device=dev, dtype=torch.float32)
    u = torch.randint(-16, 17, (N, n_planted), device=dev, generator=g).float()
    r = torch.randint(0, 2, (n_planted, F), device=dev, generator=g).float() * 2 - 1
    x = (u * s) @ r
    for lo in range(0, N, 4096):
        x[lo:lo + 4096] += torch.randint(-32, 33, (min(4096, N - lo), F), device=dev, generator=g).float()
    return x * 2.0 ** -10 + 30.0


def symmetric(n, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    A = torch.randn((n, n), device=dev, dtype=torch.float64, generator=g)
    return (A + A.T) * 0.5


def bench_apply(n, b, dev, reps, out):
    A = symmetric(n, dev)
    Q = torch.randn((n, b), device=dev, dtype=torch.float64)
    ws = ops.eig_workspace(n, b, A)
    Y, Y2 = torch.empty_like(Q), torch.empty_like(Q)
    t = alternated({"kernel": lambda: ops.eig_apply(A, Q, out=Y, workspace=ws), "matmul": lambda: torch.matmul(A, Q, out=Y2)}, reps)
    tk, tm = t["kernel"][0], t["matmul"][0]
    bound = (n + 1) * 2.0 ** -52 * (A.abs() @ Q.abs())
    tiles, splits, rows, stage = ops.eig_plan(n, b)
    emit({"what": "eig_apply", "n": n, "b": b, "reps": reps, "row_tiles": tiles, "splits": splits, "stage": stage,
          "kernel_s": tk, "kernel_min_max_s": t["kernel"][1:], "matmul_s": tm, "matmul_min_max_s": t["matmul"][1:],
          "matmul_over_kernel": tm / tk, "kernel_a_tbytes_per_s": 8.0 * n * n / tk / 1e12,
          "kernel_share_of_copy_rate": 8.0 * n * n / tk / HBM_RATE, "kernel_tflops": 2.0 * n * n * b / tk / 1e12,
          "matmul_a_tbytes_per_s": 8.0 * n * n / tm / 1e12, "matmul_tflops": 2.0 * n * n * b / tm / 1e12,
          "agree_within_bound": bool(((Y - Y2).abs() <= bound).all())}, out)


def bench_step(n, b, dev, reps, out):
    A = symmetric(n, dev)
    Q = torch.linalg.qr(torch.randn((n, b), device=dev, dtype=torch.float64))[0].contiguous()       # (qr returns columns)
    ws = ops.eig_workspace(n, b, A)
    state = {"Y": ops.eig_apply(A, Q, workspace=ws)}

    def apply():
        state["Y"] = ops.eig_apply(A, Q, workspace=ws)

    def glue():                                                 # what top_eigenpairs does around one application
        Y = state["Y"]
        H = Q.T @ Y
        evals, S = torch.linalg.eigh((H + H.T) * 0.5)
        X, AX = Q @ S, Y @ S
        res = torch.linalg.vector_norm(AX - X * evals, dim=0)
        torch.stack((evals, res)).cpu()
        torch.linalg.qr(AX)

    t = alternated({"apply": apply, "glue": glue}, reps)
    emit({"what": "eig_step", "n": n, "b": b, "reps": reps, "apply_s": t["apply"][0], "glue_s": t["glue"][0],
          "glue_share_of_step": t["glue"][0] / (eig.APPLIES_PER_STEP * t["apply"][0] + t["glue"][0]),
          "applies_per_step": eig.APPLIES_PER_STEP}, out)


def _agree(a, b):
    ra, rb = a["explained_variance_ratio_"], b["explained_variance_ratio_"]
    return bool(a["n_components_"] == b["n_components_"] and abs(ra - rb).max() <= 1e-9 * ra.max())


def bench_finalize(N, F, dev, reps, out):
    x = planted_rows(N, F, dev).double()
    mean = x.mean(0)
    xc = x - mean
    mats = {"finalize": xc.T @ xc, "finalize_samples": xc @ xc.T}
    del x, xc
    for what, M in mats.items():
        res = {}

        def run(solver):
            if what == "finalize":
                res[solver] = P.finalize(M, mean, N, 0.5, eigensolver=solver)
            else:
                res[solver] = P.finalize_samples(M.clone(), N, F, 0.5, eigensolver=solver)
        t = alternated({"partial": lambda: run("partial"), "full": lambda: run("full")}, reps)
        info = res["partial"]["eig_info_"] or {}
        emit({"what": what, "order": M.shape[0], "N": N, "F": F, "reps": reps, "route": res["partial"]["eigensolver_"],
              "partial_s": t["partial"][0], "partial_min_max_s": t["partial"][1:], "full_s": t["full"][0],
              "full_min_max_s": t["full"][1:], "full_over_partial": t["full"][0] / t["partial"][0],
              "n_components": res["partial"]["n_components_"], "block": info.get("block"), "applies": info.get("applies"),
              "agree": _agree(res["partial"], res["full"])}, out)


def bench_fit(kind, N, F, dev, reps, out):
    x = planted_rows(N, F, dev)
    fits = {}

    def run(solver):
        if kind == "pca_init":
            fits[solver] = pca_coordinates(x, eigensolver=solver)
        else:
            cls = P.WidePCA if F > P.MAX_FEATURES else P.PCA
            fits[solver] = cls(0.5, eigensolver=solver).fit(x)
    t = alternated({"partial": lambda: run("partial"), "full": lambda: run("full")}, reps)
    rec = {"what": "fit_" + kind, "N": N, "F": F, "reps": reps, "partial_s": t["partial"][0], "full_s": t["full"][0],
           "partial_min_max_s": t["partial"][1:], "full_min_max_s": t["full"][1:], "full_over_partial": t["full"][0] / t["partial"][0]}
    if kind == "pca_init":
        d = (fits["partial"] - fits["full"]).abs().max().item()
        rec["max_score_difference"] = d
    else:
        p = fits["partial"]
        rec.update(route=p.eigensolver_, n_components=p.n_components_, applies=(p.eig_info_ or {}).get("applies"),
                   agree=_agree(p.__dict__, fits["full"].__dict__))
    emit(rec, out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", nargs="+", default=["apply", "step", "finalize", "fit"],
                    choices=["apply", "step", "finalize", "fit"])
    ap.add_argument("--orders", type=int, nargs="+", default=[4096, 8192, 20000])
    ap.add_argument("--blocks", type=int, nargs="+", default=[32, 64, 256])
    ap.add_argument("--fit-rows", type=int, nargs="+", default=[8192, 20000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--slow-reps", type=int, default=1, help="repetitions of the records that run a full eigh")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eigbench needs a GPU: there is no CPU path to measure")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        if "apply" in a.sections:
            for n in a.orders:
                for b in a.blocks:
                    bench_apply(n, b, dev, a.reps, a.out)
        if "step" in a.sections:
            for n in a.orders:
                for b in (32, 256):
                    bench_step(n, b, dev, a.reps, a.out)
        if "finalize" in a.sections:
            for N in a.fit_rows:
                bench_finalize(N, 4096, dev, a.slow_reps, a.out)
        if "fit" in a.sections:
            for N in a.fit_rows:
                bench_fit("wide", N, 65536, dev, a.slow_reps, a.out)
            bench_fit("narrow", max(a.fit_rows), 4096, dev, a.slow_reps, a.out)
            bench_fit("pca_init", min(a.fit_rows), 65536, dev, a.slow_reps, a.out)


if __name__ == "__main__":
    main()
