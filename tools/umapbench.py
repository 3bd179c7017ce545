#!/usr/bin/env python3
"""The UMAP embedding behind the exact k-NN graph (csrc/umap.hip, dynamorph_amd/umap_layout.py) on one device, on knnbench's
data (30 + randn, F = 4096): per (N, k) the stages of a fit -- smooth distances, memberships, symmetrisation, initialisation
(PCA scores, rescaling, jitter), one layout epoch (median over all epochs of a fit, for each lanes-per-vertex form) -- by
device events after a warm-up of the same shape, the whole fit_graph by the host clock (it ends in a copy to the host), and
stored / fired entries per second of the epoch kernel.  With umap-learn importable, umap.UMAP with the same precomputed_knn is
timed beside it: a baseline, not an oracle.  Prints one JSON line per record.

    timeout -k 10 900 python tools/umapbench.py --rows 20000 100000 --ks 15 200 --out profiles/umap_f4096_umapbench.jsonl

--transform: the transform of new rows instead -- per (N, k) a model fitted on N rows, then R queries
of the same distribution: the query graph, the prepare stage, the layout in ONE launch for each lanes-per-query form, the same
layout launched epoch by epoch through the range arguments, and the whole UMAPEmbedding.transform by the host clock.

    timeout -k 10 900 python tools/umapbench.py --transform --rows 100000 --queries 20000 --ks 15 200 --out profiles/umap_transform_f4096_umapbench.jsonl

--wide: one fit of latents wider than 16384 features (default F = 65536, N = 8192, n = 200): the whole
UMAPEmbedding.fit_transform by the host clock with the ONE row Gram matrix it shares between the graph and the PCA
initialisation, the same steps with the matrix computed twice, and the Gram matrix's own time.

    timeout -k 10 900 python tools/umapbench.py --wide --out profiles/knn_wide_umapbench.jsonl

What bounds the epoch kernel is not separable by events: take counters from a run of their own
(`rocprofv3 --pmc ... -- python tools/umapbench.py --rows 100000 --ks 15 --epochs-only`).
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
from dynamorph_amd import umap_layout as U  # noqa: E402


def timed(fn, reps=3, warm=1):
    """(result of the last call, median seconds of `reps` device-event times after `warm` calls)."""
    for _ in range(warm):
        out = fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return out, statistics.median(ts)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def layout(indptr, cols, eps, eps_neg, y0, n_epochs, group, seed=0):
    """A whole layout with an event pair round every epoch: (final positions, seconds per epoch)."""
    nxt, nxt_neg = eps.clone(), eps_neg.clone()
    y, other = y0.clone(), torch.empty_like(y0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_epochs + 1)]
    ev[0].record()
    for n in range(n_epochs):
        ops.umap_epoch(indptr, cols, eps, eps_neg, nxt, nxt_neg, y, other, n, n_epochs, 1.58, 0.9, 1.0, seed, group)
        y, other = other, y
        ev[n + 1].record()
    torch.cuda.synchronize()
    return y, [ev[n].elapsed_time(ev[n + 1]) / 1e3 for n in range(n_epochs)]


def data(N, a, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    if a.intrinsic_dim > 0:
        D = a.intrinsic_dim
        basis = torch.randn((D, a.features), device=dev, generator=torch.Generator(device=dev).manual_seed(12345))
        return (torch.randn((N, D), device=dev, generator=g) @ basis).div_(D ** 0.5).add_(30.0)
    return torch.randn((N, a.features), device=dev, generator=g).add_(30.0)              # knnbench's data


def transform_layout(i32, eps, eps_neg, nxt0, neg0, y_train, y0, cuts, n_epochs, group):
    """The layout from fresh state through the ranges `cuts`: (positions, seconds by device events)."""
    nxt, neg, y = nxt0.clone(), neg0.clone(), y0.clone()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ops.umap_transform_layout(i32, eps, eps_neg, nxt, neg, y_train, y, lo, hi, n_epochs, 0, 0, 1.58, 0.9, 1.0, group)
    b.record()
    torch.cuda.synchronize()
    return y, a.elapsed_time(b) / 1e3


def transform_bench(a, dev):
    for N in a.rows:
        X, Q = data(N, a, dev, 0), data(a.queries, a, dev, 1)
        R = a.queries
        idx_all, dist_all = K.knn_graph(X, max(a.ks), include_self=True)
        pcs = U.pca_coordinates(X)
        for k in a.ks:
            model = U.UMAPEmbedding(n_neighbors=k)
            t0 = time.perf_counter()
            model.fit_graph(np.ascontiguousarray(idx_all[:, :k]), np.ascontiguousarray(dist_all[:, :k]), pcs, X=X)
            t_fit = time.perf_counter() - t0
            n_t = max(1, model.n_epochs_ // 3)
            K.knn_query(X, Q, k)                                                          # warm
            t0 = time.perf_counter()
            qi, qd = K.knn_query(X, Q, k)
            t_query = time.perf_counter() - t0
            i32, d = torch.from_numpy(qi.astype(np.int32)).to(dev), torch.from_numpy(qd).to(dev)
            y_train = torch.from_numpy(model.embedding_).to(dev)
            (sigma, mem, eps, eps_neg, nxt, neg, y0), t_prep = timed(lambda: ops.umap_transform_prepare(i32, d, y_train, n_t, 5))
            live = torch.isfinite(eps)
            rec = {"record": "transform", "N": N, "R": R, "k": k, "intrinsic_dim": a.intrinsic_dim, "n_epochs_t": n_t,
                   "entries": R * k, "entries_sampled": int(live.sum().item()),
                   "fired_per_epoch": float((1.0 / eps.double()).sum().item()), "s_fit_graph_wall": t_fit,
                   "s_query_graph_wall": t_query, "s_prepare": t_prep}
            ref = None
            for group in (0, 8, 64):
                ts = []
                for _ in range(4):                                                        # the first is the warm-up
                    y, t = transform_layout(i32, eps, eps_neg, nxt, neg, y_train, y0, (0, n_t), n_t, group)
                    ts.append(t)
                rec[f"s_layout_one_launch_group{group}"] = statistics.median(ts[1:])
                ref = y if ref is None else ref
                rec[f"same_bits_group{group}"] = bool(torch.equal(ref.view(torch.int32), y.view(torch.int32)))
            ts = [transform_layout(i32, eps, eps_neg, nxt, neg, y_train, y0, tuple(range(n_t + 1)), n_t, 0) for _ in range(4)]
            rec["s_layout_epoch_by_epoch"] = statistics.median(t for _, t in ts[1:])
            rec["same_bits_epoch_by_epoch"] = bool(torch.equal(ref.view(torch.int32), ts[-1][0].view(torch.int32)))
            model.transform(Q)                                                            # warm
            t0 = time.perf_counter()
            out = model.transform(Q)
            rec["s_transform_wall"] = time.perf_counter() - t0
            rec["queries_per_s"] = R / rec["s_transform_wall"]
            rec["same_bits_transform"] = bool(np.array_equal(out.view(np.uint32), ref.cpu().numpy().view(np.uint32)))
            rec["finite"] = bool(np.isfinite(out).all())
            emit(rec, a.out)
        del X, Q
        torch.cuda.empty_cache()


def wide_bench(a, dev):
    """One fit at width: shared Gram against the Gram computed twice."""
    from dynamorph_amd.pca import WidePCA
    F = a.features
    for N in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        A, B = torch.randn((N, 8), device=dev, generator=g), torch.randn((8, F), device=dev, generator=g)
        X = torch.randn((N, F), device=dev, generator=g).mul_(0.05).addmm_(A, B).add_(30.0)   # knnbench --wide's planted rows
        for k in a.ks:
            _, t_gram = timed(lambda: WidePCA().gram(X))
            model = U.UMAPEmbedding(n_neighbors=k)
            model.fit_transform(X)                                                        # warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            emb = model.fit_transform(X)
            t_shared = time.perf_counter() - t0

            def twice():
                idx, dist = K.wide_knn_graph(X, k, include_self=True)
                return U.UMAPEmbedding(n_neighbors=k).fit_graph(idx, dist, U.pca_coordinates(X)).embedding_
            twice()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            emb2 = twice()
            t_twice = time.perf_counter() - t0
            emit({"record": "wide_fit", "N": N, "F": F, "k": k, "n_epochs": model.n_epochs_, "s_fit_shared_gram_wall": t_shared,
                  "s_fit_gram_twice_wall": t_twice, "s_rowgram": t_gram, "gram_share_shared": t_gram / t_shared,
                  "gram_share_twice": 2 * t_gram / t_twice,
                  "same_bits": bool(np.array_equal(emb.view(np.uint32), emb2.view(np.uint32))),
                  "finite": bool(np.isfinite(emb).all())}, a.out)
        del X
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=None)
    ap.add_argument("--features", type=int, default=None)
    ap.add_argument("--wide", action="store_true", help="one fit of latents wider than 16384 features (F = 65536, N = 8192, n = 200)")
    ap.add_argument("--ks", type=int, nargs="+", default=None)
    ap.add_argument("--intrinsic-dim", type=int, default=0,
                    help="D > 0: data of D intrinsic dimensions, 30 + randn(N, D) @ randn(D, F) / sqrt(D), which has far shorter "
                         "hub rows than isotropic noise in F dimensions")
    ap.add_argument("--epochs-only", action="store_true", help="the graph and one layout per shape, nothing else (for counters)")
    ap.add_argument("--transform", action="store_true", help="measure the transform of --queries new rows into a model of N rows")
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("umapbench needs a GPU")
    dev = torch.device("cuda:0")
    a.rows = a.rows or ([8192] if a.wide else [20000, 100000])
    a.features = a.features or (65536 if a.wide else 4096)
    a.ks = a.ks or ([200] if a.wide else [15, 200])
    if a.wide:
        return wide_bench(a, dev)
    if a.transform:
        return transform_bench(a, dev)
    try:
        import umap as umap_learn
    except ImportError:
        umap_learn = None
        emit({"record": "umap_learn", "note": "not measured: umap-learn does not import here"}, a.out)
    for N in a.rows:
        g = torch.Generator(device=dev).manual_seed(0)
        if a.intrinsic_dim > 0:
            D = a.intrinsic_dim
            X = (torch.randn((N, D), device=dev, generator=g) @ torch.randn((D, a.features), device=dev, generator=g))
            X = X.div_(D ** 0.5).add_(30.0)
        else:
            X = torch.randn((N, a.features), device=dev, generator=g).add_(30.0)      # knnbench's data
        t0 = time.perf_counter()
        idx_all, dist_all = K.knn_graph(X, max(a.ks), include_self=True)
        emit({"record": "knn_graph", "N": N, "F": a.features, "intrinsic_dim": a.intrinsic_dim, "k": max(a.ks), "s_wall": time.perf_counter() - t0}, a.out)
        pcs, t_pca = timed(lambda: U.pca_coordinates(X), reps=1, warm=0 if a.epochs_only else 1)
        y0, t_scale = timed(lambda: U.init_layout(pcs, 0))
        n_epochs = U.default_n_epochs(N)
        for k in a.ks:
            idx = np.ascontiguousarray(idx_all[:, :k])
            dist = np.ascontiguousarray(dist_all[:, :k])
            i32 = torch.from_numpy(idx.astype(np.int32)).to(dev)
            d = torch.from_numpy(dist).to(dev)
            (rho, sigma, _, _), t_smooth = timed(lambda: ops.umap_smooth(d))
            mem, t_mem = timed(lambda: ops.umap_membership(i32, d, rho, sigma))
            (indptr, cols, w), t_sym = timed(lambda: U.symmetrize(i32, mem))
            (p_indptr, p_cols, p_w), t_prune = timed(lambda: U.prune(indptr, cols, w, n_epochs))
            (eps, eps_neg), t_sched = timed(lambda: U.schedule(p_w, 5))
            nnz = int(p_w.numel())
            fired = float((1.0 / eps.double()).sum().item())                  # entries that fire per epoch, on average
            row_len = (p_indptr[1:] - p_indptr[:-1])
            rows = torch.repeat_interleave(torch.arange(N, device=dev), row_len)
            per_row = torch.zeros(N, dtype=torch.float64, device=dev).index_add_(0, rows, 1.0 / eps.double())
            rec = {"record": "fit", "N": N, "k": k, "intrinsic_dim": a.intrinsic_dim, "n_epochs": n_epochs, "nnz_graph": int(w.numel()), "nnz_sampled": nnz,
                   "longest_row": int(row_len.max().item()), "mean_row": nnz / N, "fired_per_epoch": fired,
                   "fired_per_epoch_heaviest_row": float(per_row.max().item()),
                   "s_smooth": t_smooth, "s_membership": t_mem, "s_symmetrize": t_sym, "s_prune": t_prune,
                   "s_schedule": t_sched, "s_init_pca": t_pca, "s_init_rescale": t_scale}
            ref = None
            for group in ((0,) if a.epochs_only else (0, 1, 8, 32)):
                layout(p_indptr, p_cols, eps, eps_neg, y0, 3, group)                      # warm-up of the same shape
                y, ts = layout(p_indptr, p_cols, eps, eps_neg, y0, n_epochs, group)
                med = statistics.median(ts)
                rec[f"s_epoch_median_group{group}"] = med
                rec[f"s_layout_group{group}"] = sum(ts)
                rec[f"stored_entries_per_s_group{group}"] = nnz / med
                rec[f"fired_entries_per_s_group{group}"] = fired / med
                if ref is None:
                    ref = y
                rec[f"same_bits_group{group}"] = bool(torch.equal(ref.view(torch.int32), y.view(torch.int32)))
            if not a.epochs_only:
                emb = U.UMAPEmbedding(n_neighbors=k)
                emb.fit_graph(idx, dist, pcs)                                             # warm
                t0 = time.perf_counter()
                emb.fit_graph(idx, dist, pcs)
                rec["s_fit_graph_wall"] = time.perf_counter() - t0
                rec["finite"] = bool(np.isfinite(emb.embedding_).all())
            emit(rec, a.out)
            if umap_learn is not None and not a.epochs_only:
                Xh = X.cpu().numpy()
                t0 = time.perf_counter()
                umap_learn.UMAP(a=1.58, b=0.9, n_neighbors=k, precomputed_knn=(idx, dist)).fit(Xh)
                emit({"record": "umap_learn", "N": N, "k": k, "s_wall": time.perf_counter() - t0,
                      "threads": os.environ.get("OMP_NUM_THREADS")}, a.out)
        del X
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
