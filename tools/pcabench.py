#!/usr/bin/env python3
"""Latent PCA on the device (csrc/pca.hip, dynamorph_amd/pca.py): the Gram kernel at F = 4096 over N rows resident in HBM,
the column sums and the transform (k = 16, 64) against HBM bandwidth, the float64 eigendecomposition on the device and on
the host, and the end-to-end fit from a pinned host array.  --cpu: scikit-learn's PCA(0.5) fit of N = 20 000 rows for
comparison.  Prints one JSON line per record.

    timeout -k 10 900 python tools/pcabench.py --rows 1048576 --out profiles/pcabench.jsonl

--wide: the sample-space route for latents wider than 16384 features (WidePCA; defaults --rows 8192 --features 65536): the row
Gram matrix, the components product (k = 9, 64), double-centring + eigh, the resident fit and the fit from a pinned host
array; dm_pca_rowgram beside dm_pca_gram and one k-NN Gram panel at N = 8192, F = 16384 in the same process; with --cpu
scikit-learn's PCA(0.5) on the first 2000 rows.  --eigh-rows N ...: only the float64 eigh of an N x N Gram matrix per N.

    timeout -k 10 900 python tools/pcabench.py --wide --cpu --out profiles/pca_wide_pcabench.jsonl
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
from dynamorph_amd.pca import MAX_FEATURES, PCA, WidePCA, finalize_samples  # noqa: E402

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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def planted(N, F, dev, seed=0):
    """Latent-like rows: eight strong directions over unit noise and a common offset of 30 (PCA(0.5) keeps a handful)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.randn((N, F), device=dev, generator=g).add_(30.0)
    X.addmm_(torch.randn((N, 8), device=dev, generator=g), torch.randn((8, F), device=dev, generator=g), alpha=3.0)
    return X


def eigh_only(rows, out):
    """The float64 eigh of an N x N Gram matrix of random rows, on the device: what bounds the fit at large N."""
    dev = torch.device("cuda:0")
    for N in rows:
        A = torch.randn((N, 512), device=dev, dtype=torch.float64)
        Kc = A @ A.T
        del A
        torch.linalg.eigh(Kc[:256, :256])
        t, _ = wall(lambda: torch.linalg.eigh(Kc))
        emit({"record": "eigh_rows", "N": N, "device": "cuda", "s": t,
              "peak_mem_gib": torch.cuda.max_memory_allocated() / 2 ** 30}, out)
        del Kc
        torch.cuda.empty_cache()


def wide(a):
    N, F = a.rows or 8192, a.features or 65536
    dev = torch.device("cuda:0")
    lib = ops.L.load()
    X = planted(N, F, dev)
    p = WidePCA(0.5)
    mean, s, K = p.gram(X)
    ws = torch.empty(max(lib.dm_pca_rowgram_workspace_bytes(N, F), 8) // 8, dtype=torch.float64, device=dev)
    clk0 = sclk_hz()
    t = timed(lambda: ops.pca_rowgram(X, s, K=K, workspace=ws), a.reps)
    clk = max(c for c in (clk0, sclk_hz(), 0.0) if c is not None) or None
    flop = N * (N + 1) * F
    emit({"record": "rowgram", "N": N, "F": F, "s": t, "tflops": flop / t / 1e12, "frac_peak_spec": flop / t / PEAK_F32_MATRIX,
          "sclk_mhz": clk / 1e6 if clk else None, "workspace_mb": ws.numel() * 8 / 2 ** 20,
          "note": "FLOP = 2 N (N + 1) F / 2 (upper triangle); call time incl. the range reduction / mirror"}, a.out)
    del ws
    for k in (9, 64):
        W = torch.randn((k, N), device=dev) / N ** 0.5
        V = torch.empty((k, F), dtype=torch.float64, device=dev)
        t = timed(lambda: ops.pca_components(X, W, s, out=V), a.reps)
        emit({"record": "components", "N": N, "F": F, "k": k, "s": t, "tbs": 4 * N * F / t / 1e12,
              "frac_hbm": 4 * N * F / t / HBM_BW, "tflops": 2 * N * F * k / t / 1e12}, a.out)
        del W, V
    finalize_samples(K[:256, :256].clone(), 256, F, 0.5)
    t, fit = wall(lambda: finalize_samples(K.clone(), N, F, 0.5))
    emit({"record": "centre_eigh", "N": N, "device": "cuda", "s": t, "n_components": fit["n_components_"],
          "note": "double-centring + float64 eigh + selection (finalize_samples)"}, a.out)
    del K, fit
    t, _ = wall(lambda: p.fit(X))
    emit({"record": "fit_resident", "N": N, "F": F, "s": t, "rows_per_s": N / t, "n_components": p.n_components_}, a.out)
    Y = p.transform(X)
    t = timed(lambda: p.transform(X), a.reps)
    emit({"record": "transform_blocks", "N": N, "F": F, "k": p.n_components_, "s": t, "tbs": 4 * N * F / t / 1e12,
          "frac_hbm": 4 * N * F / t / HBM_BW}, a.out)
    del Y
    H = torch.empty((N, F), dtype=torch.float32, pin_memory=True)
    H.copy_(X)
    t, _ = wall(lambda: WidePCA(0.5).fit(H))
    emit({"record": "fit_pinned_host", "N": N, "F": F, "s": t, "rows_per_s": N / t,
          "note": "upload over PCIe into one resident matrix + the resident fit"}, a.out)
    if a.cpu:
        from sklearn.decomposition import PCA as SkPCA
        Xc = H[:2000].numpy().copy()
        t0 = time.perf_counter()
        sk = SkPCA(0.5, svd_solver="auto").fit(Xc)
        emit({"record": "sklearn_fit", "N": 2000, "F": F, "s": time.perf_counter() - t0, "solver": sk._fit_svd_solver,
              "n_components": int(sk.n_components_), "threads": os.environ.get("OMP_NUM_THREADS")}, a.out)
        WidePCA(0.5).fit(Xc)
        t, q = wall(lambda: WidePCA(0.5).fit(Xc))
        emit({"record": "gpu_fit_same_rows", "N": 2000, "F": F, "s": t, "n_components": q.n_components_}, a.out)
    del H, X
    torch.cuda.empty_cache()
    # the three Gram kernels at a shape all of them accept, in this process
    from dynamorph_amd import knn as KN
    N2, F2 = 8192, MAX_FEATURES
    X = planted(N2, F2, dev, seed=1)
    s = KN.column_shift(X)
    ws = torch.empty(max(lib.dm_pca_rowgram_workspace_bytes(N2, F2), 8) // 8, dtype=torch.float64, device=dev)
    K = torch.empty((N2, N2), dtype=torch.float64, device=dev)
    t = timed(lambda: ops.pca_rowgram(X, s, K=K, workspace=ws), a.reps)
    emit({"record": "rowgram_common_shape", "N": N2, "F": F2, "s": t, "tflops": N2 * (N2 + 1) * F2 / t / 1e12}, a.out)
    del ws, K
    ws = torch.empty(lib.dm_pca_gram_workspace_bytes(N2, F2) // 8, dtype=torch.float64, device=dev)
    G = torch.empty((F2, F2), dtype=torch.float64, device=dev)
    t = timed(lambda: ops.pca_gram(X, s, G=G, workspace=ws), a.reps)
    emit({"record": "gram_common_shape", "N": N2, "F": F2, "s": t, "tflops": N2 * F2 * (F2 + 1) / t / 1e12}, a.out)
    del ws, G
    cr = min(KN.DEFAULT_CHUNK_ROWS, N2)
    ws = ops.knn_workspace(cr, N2, F2, 15, ops.KNN_DEFAULT_SLACK, X)
    t = timed(lambda: ops.knn(X, k=15, rows=(0, cr), shift=s, include_self=True, workspace=ws), a.reps)
    emit({"record": "knn_panel_common_shape", "N": N2, "F": F2, "R": cr, "k": 15, "s": t,
          "tflops_of_call": 2.0 * cr * N2 * F2 / t / 1e12,
          "note": "whole dm_knn call (norms + Gram panel + select + refine); FLOP = 2 R M F"}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=None, help="default 1048576 (8192 with --wide)")
    ap.add_argument("--features", type=int, default=None, help="default 4096 (65536 with --wide)")
    ap.add_argument("--wide", action="store_true", help="the sample-space route (WidePCA) instead of the covariance route")
    ap.add_argument("--eigh-rows", type=int, nargs="+", default=None, help="only: float64 eigh of an N x N matrix per N")
    ap.add_argument("--host-rows", type=int, default=1 << 18, help="rows of the pinned host array of the end-to-end fit")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", action="store_true", help="also time scikit-learn's PCA(0.5) fit at N = 20 000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pcabench needs a GPU")
    if a.eigh_rows:
        return eigh_only(a.eigh_rows, a.out)
    if a.wide:
        return wide(a)
    N, F = a.rows or 1 << 20, a.features or 4096
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
