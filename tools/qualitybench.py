#!/usr/bin/env python3
"""Neighbour ranks on the device (dm_knn_ranks, csrc/knn.hip; dynamorph_amd/quality.py) at F = 4096:
per N the rank pass of all rows beside knn_graph at the same N, F, k in the same process (medians of device-event times after
a warm-up of the same shape; the targets are the graph's own columns), the columns the filter could not decide and the rows
redone on pcabench's data (30 + randn) and on z_before / z_after of a seeded, untrained VQ_VAE, and with --cpu
sklearn.manifold.trustworthiness at N = 20 000 beside quality.trustworthiness on the same data.  One JSON line per record.

    timeout -k 10 900 python tools/qualitybench.py --rows 20000 100000 --out profiles/quality_f4096_qualitybench.jsonl

Kernel times (rank_count_kernel beside knn_select_kernel, which reads the same panel row five times) are not separable by
events around the calls: take them from a run of their own under
`rocprofv3 --kernel-trace --stats -- python tools/qualitybench.py --rows 20000 --panel-only`."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from knnbench import emit, encoder_latents, medians  # noqa: E402
from dynamorph_amd import knn as K  # noqa: E402
from dynamorph_amd import ops  # noqa: E402
from dynamorph_amd import quality as Q  # noqa: E402


def graph_on_device(x, k, cr, shift):
    """knn_graph(include_self=False)'s panel walk without the copy to the host: run() -> (indices, fallback counters)."""
    M, F = x.shape
    ws = ops.knn_workspace(cr, M, F, k, ops.KNN_DEFAULT_SLACK, x)
    idx = torch.empty((M, k), dtype=torch.int32, device=x.device)
    dist = torch.empty((M, k), dtype=torch.float32, device=x.device)

    def run():
        return idx, [ops.knn(x, k=k, rows=(lo, min(cr, M - lo)), shift=shift, out=(idx[lo:lo + cr], dist[lo:lo + cr]),
                             workspace=ws)[2] for lo in range(0, M, cr)]
    return run


def ranks_on_device(x, targets, cr, shift, cap=None):
    """neighbor_ranks' panel walk without the copies: run() -> (ranks, [(ambiguous, redone) counters per panel])."""
    M, F = x.shape
    c = targets.shape[1]
    cap = ops.knn_ranks_default_cap(c, M) if cap is None else cap
    ws = torch.empty(ops.L.load().dm_knn_ranks_workspace_bytes(cr, M, F, c, cap), dtype=torch.uint8, device=x.device)
    ranks = torch.empty((M, c), dtype=torch.int32, device=x.device)

    def run():
        return ranks, [ops.knn_ranks(x, targets[lo:lo + cr], rows=(lo, min(cr, M - lo)), shift=shift, cap=cap,
                                     out=ranks[lo:lo + cr], workspace=ws)[1:] for lo in range(0, M, cr)]
    return run, ws.numel(), cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[20000, 100000])
    ap.add_argument("--features", type=int, default=4096)
    ap.add_argument("--ks", type=int, nargs="+", default=[15])
    ap.add_argument("--chunk-rows", type=int, default=K.DEFAULT_CHUNK_ROWS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--panel-only", action="store_true", help="one panel of the graph and of the ranks per shape (for a kernel trace)")
    ap.add_argument("--count-rows", type=int, default=8192, help="rows of the ambiguous-column records")
    ap.add_argument("--cpu", action="store_true", help="also sklearn.manifold.trustworthiness at N = 20 000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qualitybench needs a GPU")
    dev = torch.device("cuda:0")
    F = a.features
    for N in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn((N, F), device=dev, generator=g).add_(30.0)          # pcabench's data
        s = K.column_shift(X)
        cr = min(a.chunk_rows, N)
        for k in a.ks:
            graph = graph_on_device(X, k, cr, s)
            idx, _ = graph()
            targets = idx.clone()
            rank, ws_bytes, cap = ranks_on_device(X, targets, cr, s)
            if a.panel_only:
                ops.knn(X, k=k, rows=(0, cr), shift=s)
                ops.knn_ranks(X, targets[:cr], rows=(0, cr), shift=s)
                torch.cuda.synchronize()
                continue
            tg, glo, ghi = medians(lambda: graph(), a.reps)
            tr, rlo, rhi = medians(lambda: rank(), a.reps)
            ranks, counts = rank()
            tot = torch.stack([torch.cat(c) for c in counts]).sum(0, dtype=torch.int64).tolist()
            own = bool((ranks == torch.arange(1, k + 1, device=dev, dtype=torch.int32)).all().item())
            emit({"record": "rank_pass", "N": N, "F": F, "k": k, "chunk_rows": cr, "s_rank_pass": tr, "s_min": rlo, "s_max": rhi,
                  "s_knn_graph": tg, "s_graph_min": glo, "s_graph_max": ghi, "rank_pass_over_graph": tr / tg,
                  "tflops_rank_pass": 2.0 * N * N * F / tr / 1e12, "ambiguous_per_row": tot[0] / N, "rows_redone": tot[1],
                  "cap": cap, "workspace_mb": ws_bytes / 2 ** 20, "own_columns_have_rank_c_plus_1": own}, a.out)
        del X
        torch.cuda.empty_cache()
    if a.panel_only:
        return
    n = a.count_rows
    g = torch.Generator(device=dev).manual_seed(2)
    kinds = {"pcabench": torch.randn((n, F), device=dev, generator=g).add_(30.0)}
    try:
        zb, za = encoder_latents(min(n, 4096), dev)
        kinds["z_before"], kinds["z_after"] = torch.from_numpy(zb).to(dev), torch.from_numpy(za).to(dev)
    except Exception as ex:                                                  # noqa: BLE001
        emit({"record": "ambiguous", "data": "z_before / z_after", "error": repr(ex), "note": "not measured"}, a.out)
    for name, x in kinds.items():
        for k in a.ks:
            tgt = K.knn_graph(x, k, include_self=False)[0]
            t0 = time.perf_counter()
            ranks, namb, nredo = Q.neighbor_ranks(x, tgt, return_counts=True)
            emit({"record": "ambiguous", "data": name, "N": x.shape[0], "F": x.shape[1], "k": k, "ambiguous_per_row":
                  namb / x.shape[0], "rows_redone": nredo, "s_wall": time.perf_counter() - t0,
                  "own_columns_have_rank_c_plus_1": bool((ranks == np.arange(1, k + 1)).all())}, a.out)
    if a.cpu:
        try:
            from sklearn.manifold import trustworthiness
        except ImportError:
            emit({"record": "sklearn_trustworthiness", "note": "not measured: scikit-learn does not import here"}, a.out)
            return
        g = torch.Generator(device=dev).manual_seed(0)
        Xc = torch.randn((20000, F), device=dev, generator=g).add_(30.0)
        Y = (Xc - Xc.mean(0))[:, :2].contiguous()                            # any embedding: two centred columns
        Q.trustworthiness(Xc, Y, 15)
        t0 = time.perf_counter()
        t_gpu = Q.trustworthiness(Xc, Y, 15)
        s_gpu = time.perf_counter() - t0
        t0 = time.perf_counter()
        t_cpu = trustworthiness(Xc.cpu().numpy(), Y.cpu().numpy(), n_neighbors=15)
        emit({"record": "sklearn_trustworthiness", "N": 20000, "F": F, "k": 15, "s": time.perf_counter() - t0, "s_gpu_wall": s_gpu,
              "value_sklearn": float(t_cpu), "value_gpu": t_gpu, "threads": os.environ.get("OMP_NUM_THREADS")}, a.out)


if __name__ == "__main__":
    main()
