#!/usr/bin/env python3
"""Latent PCA on the device (csrc/pca.hip, dynamorph_amd/pca.py): the Gram kernel at F = 4096 over N rows resident in HBM,
the column sums and the transform (k = 16, 64) against HBM bandwidth, the float64 eigendecomposition on the device and on
the host, and the end-to-end fit from a pinned host array.  --cpu: scikit-learn's PCA(0.5) fit of N = 20 000 rows for
comparison.  Prints one JSON line per record.

    timeout -k 10 900 python tools/pcabench.py --rows 1048576 --out profiles/pcabench.jsonl
"""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dynamorph_amd import ops  # noqa: E402
from dynamorph_amd.pca import PCA  # noqa: E402

PEAK_F32_MATRIX = 157.3e12      # 256 CU x 4 SIMD x 64 FLOP/clk x 2.4 GHz (MI355X_MICROARCH.md)
PEAK_CLOCK = 2.4e9
HBM_BW = 8.0e12


def sclk_hz():
    """Current shader clock as the driver reports it (read only), or None."""
    for path in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            for line in open(path):
                if line.strip().endswith("*"):
                    return float(line.split(":")[1].strip().rstrip("*").strip().lower().replace("mhz", "")) * 1e6
        except (OSError, ValueError, IndexError):
            continue
    return None


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / reps


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--features", type=int, default=4096)
    ap.add_argument("--host-rows", type=int, default=1 << 18, help="rows of the pinned host array of the end-to-end fit")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true", help="also time scikit-learn's PCA(0.5) fit at N = 20 000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcabench needs a GPU")
    N, F = a.rows, a.features
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn((N, F), device=dev, generator=g).add_(30.0)
    s = (ops.pca_colsum(X) / N).float()
    ws = torch.empty(ops.L.load().dm_pca_gram_workspace_bytes(N, F) // 8, dtype=torch.float64, device=dev)
    G = torch.empty((F, F), dtype=torch.float64, device=dev)
    clk0 = sclk_hz()
    t = timed(lambda: ops.pca_gram(X, s, G=G, workspace=ws), a.reps)
    clk1 = sclk_hz()
    flop = N * F * (F + 1)
    clk = max(c for c in (clk0, clk1, 0.0) if c is not None) or None
    peak_at_clk = PEAK_F32_MATRIX * (clk / PEAK_CLOCK) if clk else None
    emit({"record": "gram", "N": N, "F": F, "s": t, "tflops": flop / t / 1e12, "frac_peak_spec": flop / t / PEAK_F32_MATRIX,
          "sclk_mhz": clk / 1e6 if clk else None,
          "frac_peak_at_clock": flop / t / peak_at_clk if peak_at_clk else None,
          "note": "FLOP = N*F*(F+1) (upper triangle); call time incl. the split reduction"}, a.out)
    cws = torch.empty(ops.L.load().dm_pca_colsum_workspace_bytes(N, F) // 8, dtype=torch.float64, device=dev)
    sums = torch.empty(F, dtype=torch.float64, device=dev)
    t = timed(lambda: ops.pca_colsum(X, sums=sums, workspace=cws), a.reps * 3)
    emit({"record": "colsum", "N": N, "F": F, "s": t, "tbs": 4 * N * F / t / 1e12, "frac_hbm": 4 * N * F / t / HBM_BW}, a.out)
    for k in (16, 64):
        V = torch.linalg.qr(torch.randn(F, k, device=dev))[0].T.contiguous()
        Y = torch.empty((N, k), device=dev)
        t = timed(lambda: ops.pca_transform(X, V, s, out=Y), a.reps * 3)
        nbytes = 4 * N * (F + k)
        emit({"record": "transform", "N": N, "F": F, "k": k, "s": t, "tbs": nbytes / t / 1e12,
              "frac_hbm": nbytes / t / HBM_BW, "tflops": 2 * N * F * k / t / 1e12}, a.out)
    C = G / (N - 1)
    for where in ("cuda", "cpu"):
        Cw = C.to(where)
        torch.linalg.eigh(Cw[:256, :256])
        if where == "cuda":
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.linalg.eigh(Cw)
        if where == "cuda":
            torch.cuda.synchronize()
        emit({"record": "eigh", "F": F, "device": where, "s": time.perf_counter() - t0,
              "threads": torch.get_num_threads()}, a.out)
    del X, ws, G, C
    torch.cuda.empty_cache()
    hn = a.host_rows
    while True:
        try:
            H = torch.empty((hn, F), dtype=torch.float32, pin_memory=True)
            break
        except RuntimeError:
            hn //= 2
    H.normal_().add_(30.0)
    p = PCA(0.5, chunk_rows=65536)
    p.fit(H[:131072])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p.fit(H)
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    emit({"record": "fit_pinned_host", "N": hn, "F": F, "chunk_rows": 65536, "s": t, "rows_per_s": hn / t,
          "n_components": p.n_components_, "note": "moments streamed over PCIe + eigh on the device + selection"}, a.out)
    if a.cpu:
        from sklearn.decomposition import PCA as SkPCA
        Xc = H[:20000].numpy().copy()
        t0 = time.perf_counter()
        sk = SkPCA(0.5, svd_solver="auto").fit(Xc)
        emit({"record": "sklearn_fit", "N": 20000, "F": F, "s": time.perf_counter() - t0, "solver": sk._fit_svd_solver,
              "threads": os.environ.get("OMP_NUM_THREADS")}, a.out)
        t0 = time.perf_counter()
        PCA(0.5).fit(Xc)
        torch.cuda.synchronize()
        emit({"record": "gpu_fit_same_rows", "N": 20000, "F": F, "s": time.perf_counter() - t0}, a.out)


if __name__ == "__main__":
    main()
