#!/usr/bin/env python3
"""The k-means of the latents on the device (csrc/kmeans.hip, dynamorph_amd/kmeans.py) with X resident:
per (N, F, K) the labelling pass (dm_kmeans_assign), the per-cluster sums (dm_kmeans_sums) and one whole Lloyd iteration
(both, plus the centre update), beside the same iteration composed from the parts that existed before -- ops.knn(C, X panel,
k = 1) per 2048 rows plus a float64 index_add_ -- alternated in one process; medians of device-event times after a warm-up
of the same shape.  The labelling pass is set against its two bounds (2 N K F FLOP at the f32 matrix peak, 4 N F bytes at the
HBM rate) and says which one binds; the rows redone exactly and the whole fit at n_init = 1 from given centres follow.
With --cpu: one scikit-learn KMeans(n_init=1, init=C0) fit on 16 threads at the smallest N (a baseline, not an oracle).
Prints one JSON line per record.

    timeout -k 10 900 python tools/kmeansbench.py --rows 20000 100000 --features 4096 256 --clusters 4 64 256 \\
        --out profiles/kmeans_kmeansbench.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dynamorph_amd import KMeans  # noqa: E402
from dynamorph_amd import knn as KN  # noqa: E402
from dynamorph_amd import ops  # noqa: E402

F32_MATRIX_PEAK = 157.3e12      # FLOP/s, v_mfma_f32_32x32x2_f32 (datasheet = vector peak)
HBM_RATE = 6.29e12              # bytes/s, measured float4 copy (8.0e12 datasheet)
PANEL_ROWS = 2048               # knn_query's default chunk


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


def planted(N, F, K, dev, seed=0, sep=1.0):
    """K planted clusters: sep * randn(K, F)[label] + randn(N, F), fp32 on the device; and K of its rows as first centres."""
    g = torch.Generator(device=dev).manual_seed(seed)
    cen = torch.randn((K, F), device=dev, generator=g) * sep
    lab = torch.randint(0, K, (N,), device=dev, generator=g)
    x = torch.randn((N, F), device=dev, generator=g)
    for lo in range(0, N, 16384):
        x[lo:lo + 16384] += cen[lab[lo:lo + 16384]]
    rows = torch.randperm(N, device=dev, generator=g)[:K].sort().values
    return x, x[rows].contiguous()


def bench_shape(N, F, K, dev, reps, out, cpu):
    x, C0 = planted(N, F, K, dev)
    s = KN.column_shift(x)
    ws = ops.kmeans_workspace(N, F, K, x)
    labels = torch.empty(N, dtype=torch.int32, device=dev)
    sums = torch.empty((K, F), dtype=torch.float64, device=dev)
    counts = torch.empty(K, dtype=torch.int64, device=dev)
    state = {}

    def assign():
        state["n"] = ops.kmeans_assign(x, C0, s, labels=labels, want_dist=False, workspace=ws)[2]

    def sum_rows():
        ops.kmeans_sums(x, labels, K, sums, counts, workspace=ws)

    def iteration():
        assign()
        sum_rows()
        state["C"] = (sums / counts.double()[:, None]).float()

    # the same iteration from the parts of the k-NN graph: the exact nearest centre of every row, panel by panel, and the sums
    cr = min(PANEL_ROWS, N)
    kws = ops.knn_workspace(cr, K, F, 1, ops.KNN_DEFAULT_SLACK, x)
    sc = KN.column_shift(C0)
    idx = torch.empty((N, 1), dtype=torch.int32, device=dev)
    dist = torch.empty((N, 1), dtype=torch.float32, device=dev)
    sums2 = torch.empty((K, F), dtype=torch.float64, device=dev)

    def composed():
        sums2.zero_()
        for lo in range(0, N, cr):
            m = min(cr, N - lo)
            ops.knn(C0, x[lo:lo + m], k=1, shift=sc, out=(idx[lo:lo + m], dist[lo:lo + m]), workspace=kws)
            sums2.index_add_(0, idx[lo:lo + m, 0].long(), x[lo:lo + m].double())
        cnt = torch.bincount(idx[:, 0].long(), minlength=K)
        state["C2"] = (sums2 / cnt.double()[:, None]).float()

    t = alternated({"iteration": iteration, "composed": composed, "assign": assign, "sums": sum_rows}, reps)
    same = bool(torch.equal(labels, idx[:, 0]))
    flop, nbytes = 2.0 * N * K * F, 4.0 * N * F
    ta, tsu = t["assign"][0], t["sums"][0]
    t_flop, t_mem = flop / F32_MATRIX_PEAK, nbytes / HBM_RATE
    rec = {"what": "kmeans_iteration", "N": N, "F": F, "K": K, "reps": reps,
           "iteration_s": t["iteration"][0], "iteration_min_max_s": t["iteration"][1:],
           "composed_s": t["composed"][0], "composed_min_max_s": t["composed"][1:],
           "composed_over_iteration": t["composed"][0] / t["iteration"][0],
           "labels_equal_composed": same,
           "assign_s": ta, "assign_tflops": flop / ta / 1e12, "assign_share_of_f32_matrix_peak": t_flop / ta,
           "assign_x_tbytes_per_s": nbytes / ta / 1e12, "assign_share_of_hbm_rate": t_mem / ta,
           "assign_bound": "matrix" if t_flop > t_mem else "hbm", "assign_share_of_bound": max(t_flop, t_mem) / ta,
           "sums_s": tsu, "sums_x_tbytes_per_s": nbytes / tsu / 1e12,
           "rechecked_rows": int(state["n"].item())}
    emit(rec, out)

    C0h = C0.cpu().numpy()
    model = KMeans(K, init=C0h, n_init=1)
    model.fit(x)                                                   # warm-up of the same shape
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.fit(x)
    torch.cuda.synchronize()
    fit_s = time.perf_counter() - t0
    rec = {"what": "kmeans_fit", "N": N, "F": F, "K": K, "n_init": 1, "fit_wall_s": fit_s, "n_iter": model.n_iter_,
           "per_iteration_s": fit_s / model.n_iter_, "inertia": model.inertia_, "rechecked_rows": model.rechecked_}
    emit(rec, out)
    if cpu:
        try:
            from sklearn.cluster import KMeans as SkKMeans
            from threadpoolctl import threadpool_limits
        except ImportError:
            emit({"what": "sklearn_fit", "N": N, "F": F, "K": K, "skipped": "scikit-learn or threadpoolctl does not import"}, out)
        else:
            xh = x.cpu().numpy()
            with threadpool_limits(limits=16):
                t0 = time.perf_counter()
                sk = SkKMeans(n_clusters=K, init=C0h, n_init=1, algorithm="lloyd").fit(xh)
                cpu_s = time.perf_counter() - t0
            emit({"what": "sklearn_fit", "N": N, "F": F, "K": K, "threads": 16, "fit_wall_s": cpu_s, "n_iter": int(sk.n_iter_),
                  "inertia": float(sk.inertia_), "labels_equal_gpu": bool(np.array_equal(sk.labels_, model.labels_)),
                  "cpu_over_gpu": cpu_s / fit_s}, out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--features", type=int, nargs="+", default=[4096, 256])
    ap.add_argument("--clusters", type=int, nargs="+", default=[4, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true", help="also fit scikit-learn's KMeans on 16 threads at the smallest N")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kmeansbench needs a GPU: there is no CPU path to measure")
    dev = torch.device("cuda:0")
    with torch.no_grad():
        for N in a.rows:
            for F in a.features:
                for K in a.clusters:
                    bench_shape(N, F, K, dev, a.reps, a.out, a.cpu and N == min(a.rows))


if __name__ == "__main__":
    main()
