#!/usr/bin/env python3
"""The exact k-nearest-neighbour graph on the device (csrc/knn.hip, dynamorph_amd/knn.py) at F = 4096: the whole graph of N
resident rows for k = 15 and 200 (median of device-event times after a warm-up of the same shape), one panel's call beside
dm_pca_gram on the same rows in the same process, the share of rows that took the exact fallback on four kinds of data, and
with --cpu scikit-learn's brute-force NearestNeighbors at N = 20 000 when it imports.  Prints one JSON line per record.

    timeout -k 10 900 python tools/knnbench.py --rows 20000 100000 --out profiles/knn_bench.jsonl

Kernel times (the Gram panel against select / refine) are not separable by events around dm_knn: take them from a run of
their own under `rocprofv3 --kernel-trace --stats -- python tools/knnbench.py --rows 20000 --panel-only`.

--wide: the graph of latents wider than 16384 features at F = 65536 instead -- per (data, N, k) the
row Gram matrix, the graph behind it with the pair-once refine and with knn_refine_kernel on the same candidate lists
(alternated twice, medians), the fallback rows and the share of candidate slots that needed an evaluation of their own; at
N = 8192, F = 16384 the wide route beside knn_graph; with --cpu scikit-learn's brute force at the smallest N.

    timeout -k 10 900 python tools/knnbench.py --wide --rows 2000 8192 20000 --cpu --out profiles/knn_wide_knnbench.jsonl
    rocprofv3 --kernel-trace --stats -- python tools/knnbench.py --wide --rows 8192 --panel-only
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
from dynamorph_amd import knn as K  # noqa: E402
from dynamorph_amd import ops  # noqa: E402


def medians(fn, reps, warm=1):
    """Median and spread of `reps` device-event times of fn() after `warm` calls of the same shape."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return statistics.median(ts), min(ts), max(ts)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def graph_on_device(x, k, chunk_rows, shift, slack=None):
    """knn_graph's panel walk without the copy to the host: (indices, distances, fallback counter tensors)."""
    M, F = x.shape
    sl = ops.KNN_DEFAULT_SLACK if slack is None else slack
    cr = min(chunk_rows, M)
    ws = ops.knn_workspace(cr, M, F, k, sl, x)
    idx = torch.empty((M, k), dtype=torch.int32, device=x.device)
    dist = torch.empty((M, k), dtype=torch.float32, device=x.device)

    def run():
        return [ops.knn(x, k=k, rows=(lo, min(cr, M - lo)), shift=shift, slack=sl, include_self=True,
                        out=(idx[lo:lo + cr], dist[lo:lo + cr]), workspace=ws)[2] for lo in range(0, M, cr)]
    return run


def encoder_latents(n, dev):
    """z_before / z_after (n, 4096) of a seeded, untrained VQ_VAE on synthetic patches."""
    from dynamorph_amd import VQ_VAE
    from dynamorph_amd.patch_vae import encode_patches
    torch.manual_seed(0)
    model = VQ_VAE().to(dev).eval()
    patches = torch.randn((n, 2, 128, 128), generator=torch.Generator().manual_seed(1))
    return encode_patches(model, patches, device=str(dev))


def wide_planted(N, F, dev, seed=0, offset=30.0):
    """The planted rows of tests/helpers/knn_wide_fixtures.py on the device: offset + randn(N, 8) randn(8, F) + 0.05 randn."""
    g = torch.Generator(device=dev).manual_seed(seed)
    a, b = torch.randn((N, 8), device=dev, generator=g), torch.randn((8, F), device=dev, generator=g)
    return torch.randn((N, F), device=dev, generator=g).mul_(0.05).addmm_(a, b).add_(offset)


def z32_latents(n, dev):
    """z_after (n, 65536) of a seeded, untrained VQ_VAE_z32 at the example configuration's widths on synthetic patches."""
    from dynamorph_amd import VQ_VAE_z32
    from dynamorph_amd.patch_vae import encode_patches
    torch.manual_seed(0)
    model = VQ_VAE_z32(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512).to(dev).eval()
    out = []
    for lo in range(0, n, 1024):                                             # (the host copy of all patches would be 1 GB)
        patches = torch.randn((min(1024, n - lo), 2, 128, 128), generator=torch.Generator().manual_seed(1 + lo))
        out.append(torch.from_numpy(encode_patches(model, patches, device=str(dev))[1]).to(dev))
    return torch.cat(out)


def wide_graph_on_device(x, g, k, pair_once, slack=None):
    """wide_knn_graph behind a given Gram matrix without the copy to the host."""
    N, F = x.shape
    sl = ops.KNN_DEFAULT_SLACK if slack is None else slack
    ws = torch.empty(ops.L.load().dm_knn_wide_self_workspace_bytes(N, F, k, sl), dtype=torch.uint8, device=x.device)
    out = (torch.empty((N, k), dtype=torch.int32, device=x.device), torch.empty((N, k), dtype=torch.float32, device=x.device))
    return lambda: ops.knn_wide_self(x, g[2], k=k, shift=g[1], slack=sl, include_self=True, pair_once=pair_once, out=out,
                                     workspace=ws)


def wide_main(a, dev):
    from dynamorph_amd.pca import WidePCA
    F = a.features
    kinds = [("planted", lambda N: wide_planted(N, F, dev))]
    if not a.panel_only:
        kinds.append(("z32_after", lambda N: z32_latents(N, dev) if N <= a.fallback_rows else None))
    for name, make in kinds:
        for N in a.rows:
            try:
                X = make(N)
            except Exception as ex:                                          # noqa: BLE001
                emit({"record": "wide_graph", "data": name, "N": N, "error": repr(ex), "note": "not measured"}, a.out)
                continue
            if X is None:
                emit({"record": "wide_graph", "data": name, "N": N, "note": "not measured: above --fallback-rows"}, a.out)
                continue
            F_ = X.shape[1]
            p = WidePCA()
            if a.panel_only:
                g = p.gram(X)
                for k in a.ks:
                    for once in (True, False):
                        wide_graph_on_device(X, g, k, once)()
                torch.cuda.synchronize()
                continue
            g = p.gram(X)
            t_gram, lo, hi = medians(lambda: p.gram(X), a.reps)
            for k in a.ks:
                runs = {True: wide_graph_on_device(X, g, k, True), False: wide_graph_on_device(X, g, k, False)}
                ts = {True: [], False: []}
                for _ in range(2):                                           # alternated twice
                    for once in (True, False):
                        ts[once].append(medians(runs[once], a.reps)[0])
                _, _, nfb, npairs = runs[True]()
                Kc = min(k - 1 + ops.KNN_DEFAULT_SLACK, N - 1)
                same = all(torch.equal(u, v) for u, v in zip(runs[True]()[:2], [t.clone() for t in runs[False]()[:2]]))
                t1, t0 = statistics.median(ts[True]), statistics.median(ts[False])
                emit({"record": "wide_graph", "data": name, "N": N, "F": F_, "k": k, "s_rowgram": t_gram,
                      "rowgram_tflops": N * (N + 1) * F_ / t_gram / 1e12, "s_graph_behind_gram_pair_once": t1,
                      "s_graph_behind_gram_plain_refine": t0, "s_runs_pair_once": ts[True], "s_runs_plain_refine": ts[False],
                      "s_whole_graph": t_gram + t1, "pair_once_saves_s": t0 - t1, "same_bits": bool(same),
                      "fallback_rows": int(nfb.item()), "fallback_share": int(nfb.item()) / N,
                      "pairs_per_slot": int(npairs.item()) / (N * Kc)}, a.out)
            del X, g
            torch.cuda.empty_cache()
    if a.panel_only:
        return
    # the shape both routes accept: the whole graph, wide self route beside knn_graph
    N2, F2 = 8192, K.MAX_FEATURES
    X = wide_planted(N2, F2, dev, seed=1)
    s = K.column_shift(X)
    p = WidePCA()
    for k in a.ks:
        narrow = graph_on_device(X, k, min(a.chunk_rows, N2), s)
        t_n = medians(narrow, a.reps)[0]

        def whole():
            g = p.gram(X)
            return wide_graph_on_device(X, g, k, True)()
        t_w = medians(whole, a.reps)[0]
        t_g = medians(lambda: p.gram(X), a.reps)[0]
        emit({"record": "common_shape", "N": N2, "F": F2, "k": k, "s_knn_graph": t_n, "s_wide_graph": t_w, "s_rowgram": t_g,
              "note": "whole graphs on the device, no copy to the host; the wide time includes allocating K and the workspace"},
             a.out)
    del X
    torch.cuda.empty_cache()
    if a.cpu:
        try:
            from sklearn.neighbors import NearestNeighbors
        except ImportError:
            emit({"record": "sklearn_brute", "note": "not measured: scikit-learn does not import here"}, a.out)
            return
        N = min(a.rows)
        Xc = wide_planted(N, F, dev)
        Xh = Xc.cpu().numpy()
        for k in a.ks:
            t0 = time.perf_counter()
            NearestNeighbors(n_neighbors=k, algorithm="brute").fit(Xh).kneighbors(Xh)
            t_cpu = time.perf_counter() - t0
            K.wide_knn_graph(Xc, k)
            t0 = time.perf_counter()
            K.wide_knn_graph(Xc, k)
            emit({"record": "sklearn_brute", "N": N, "F": F, "k": k, "s": t_cpu, "s_gpu_wall": time.perf_counter() - t0,
                  "threads": os.environ.get("OMP_NUM_THREADS")}, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=None)
    ap.add_argument("--features", type=int, default=None)
    ap.add_argument("--wide", action="store_true", help="the graph of latents wider than 16384 features (default F = 65536)")
    ap.add_argument("--ks", type=int, nargs="+", default=[15, 200])
    ap.add_argument("--chunk-rows", type=int, default=K.DEFAULT_CHUNK_ROWS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--panel-only", action="store_true", help="one panel call per shape and nothing else (for a kernel trace)")
    ap.add_argument("--fallback-rows", type=int, default=8192, help="rows of the fallback-share records")
    ap.add_argument("--cpu", action="store_true", help="also time scikit-learn's brute-force NearestNeighbors at N = 20 000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knnbench needs a GPU")
    dev = torch.device("cuda:0")
    a.rows = a.rows or ([2000, 8192, 20000] if a.wide else [20000, 100000])
    a.features = a.features or (65536 if a.wide else 4096)
    if a.wide:
        return wide_main(a, dev)
    F = a.features
    for N in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn((N, F), device=dev, generator=g).add_(30.0)          # pcabench's data
        s = K.column_shift(X)
        cr = min(a.chunk_rows, N)
        for k in a.ks:
            ws = ops.knn_workspace(cr, N, F, k, ops.KNN_DEFAULT_SLACK, X)
            t, lo, hi = medians(lambda: ops.knn(X, k=k, rows=(0, cr), shift=s, include_self=True, workspace=ws), a.reps)
            emit({"record": "panel_call", "N": N, "F": F, "k": k, "R": cr, "s": t, "s_min": lo, "s_max": hi,
                  "tflops_of_call": 2.0 * cr * N * F / t / 1e12, "workspace_mb": ws.numel() / 2 ** 20,
                  "note": "whole dm_knn call (norms + Gram panel + select + refine + empty fallback rounds); FLOP = 2 R M F"},
                 a.out)
            del ws
        if a.panel_only:
            continue
        gws = torch.empty(ops.L.load().dm_pca_gram_workspace_bytes(N, F) // 8, dtype=torch.float64, device=dev)
        G = torch.empty((F, F), dtype=torch.float64, device=dev)
        t, lo, hi = medians(lambda: ops.pca_gram(X, s, G=G, workspace=gws), a.reps)
        emit({"record": "pca_gram_same_rows", "N": N, "F": F, "s": t, "s_min": lo, "s_max": hi,
              "tflops": N * F * (F + 1) / t / 1e12, "note": "FLOP = N F (F + 1), upper triangle, as pcabench counts"}, a.out)
        del gws, G
        for k in a.ks:
            run = graph_on_device(X, k, cr, s)
            t, lo, hi = medians(run, a.reps)
            nfb = int(torch.cat(run()).sum().item())
            emit({"record": "graph", "N": N, "F": F, "k": k, "chunk_rows": cr, "s": t, "s_min": lo, "s_max": hi,
                  "tflops": 2.0 * N * N * F / t / 1e12, "rows_per_s": N / t, "fallback_rows": nfb,
                  "fallback_share": nfb / N}, a.out)
        del X
        torch.cuda.empty_cache()
    if a.panel_only:
        return
    n = a.fallback_rows
    g = torch.Generator(device=dev).manual_seed(2)
    kinds = {"pcabench": (torch.randn((n, F), device=dev, generator=g).add_(30.0), True),
             "offset": (torch.randn((n, F), device=dev, generator=g).mul_(1e-2).add_(3.0), True)}
    kinds["offset_no_shift"] = (kinds["offset"][0], False)
    try:
        zb, za = encoder_latents(min(n, 4096), dev)
        kinds["z_before"] = (torch.from_numpy(zb).to(dev), True)
        kinds["z_after"] = (torch.from_numpy(za).to(dev), True)
    except Exception as ex:                                              # noqa: BLE001
        emit({"record": "fallback_share", "data": "z_before / z_after", "error": repr(ex), "note": "not measured"}, a.out)
    for name, (x, shifted) in kinds.items():
        for k in a.ks:
            if k > x.shape[0] - 1:
                continue
            t0 = time.perf_counter()
            _, _, nfb = K.knn_graph(x, k, shift="mean" if shifted else None, return_fallback=True)
            emit({"record": "fallback_share", "data": name, "N": x.shape[0], "F": x.shape[1], "k": k, "fallback_rows": nfb,
                  "fallback_share": nfb / x.shape[0], "s_wall": time.perf_counter() - t0}, a.out)
    if a.cpu:
        try:
            from sklearn.neighbors import NearestNeighbors
        except ImportError:
            emit({"record": "sklearn_brute", "note": "not measured: scikit-learn does not import here"}, a.out)
            return
        g = torch.Generator(device=dev).manual_seed(0)
        Xc = torch.randn((20000, F), device=dev, generator=g).add_(30.0)
        Xh = Xc.cpu().numpy()
        for k in a.ks:
            t0 = time.perf_counter()
            NearestNeighbors(n_neighbors=k, algorithm="brute").fit(Xh).kneighbors(Xh)
            t_cpu = time.perf_counter() - t0
            K.knn_graph(Xc, k)
            t0 = time.perf_counter()
            K.knn_graph(Xc, k)
            emit({"record": "sklearn_brute", "N": 20000, "F": F, "k": k, "s": t_cpu, "s_gpu_wall": time.perf_counter() - t0,
                  "threads": os.environ.get("OMP_NUM_THREADS")}, a.out)


if __name__ == "__main__":
    main()
