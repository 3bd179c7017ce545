#!/usr/bin/env python3
"""The EMA codebook mode on the MI355X, everything in one process, alternated, after warming every shape:
(1) the fused training step with the mode off and on -- device events around whole steps (captured forward + backward, the
exchange, Adam and the update launch) at B = 2048 on the default VQ_VAE and at bench.py's z32ex configuration -- with the
mode-off step against itself for the spread; (2) dm_vq_backward_stats beside dm_vq_backward_slabs on each of the three
routes; (3) dm_vq_ema_apply alone.

    python tools/emabench.py [--steps 30] [--launches 40] [--batch 2048] [--z32-batch 768] [--skip-steps]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dynamorph_amd  # noqa: E402
from dynamorph_amd import ops  # noqa: E402
from dynamorph_amd.train import FusedTrainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--launches", type=int, default=40)
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--z32-batch", type=int, default=768)
ap.add_argument("--skip-steps", action="store_true", help="kernels only")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("emabench: no GPU visible (times are measured on the device or not at all)")
DEV = "cuda:0"
EXAMPLE_CONFIG = dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512)      # bench.py's z32ex
record = {}


def alternate(fa, fb, n, warm=5):
    """n calls each of fa and fb, alternated, every call timed by its own pair of device events -> (median a, median b) ms."""
    for _ in range(warm):
        fa(), fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(n):
        for f, acc in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return float(np.median(ta)), float(np.median(tb))


def tm_matrix(B):
    i = torch.arange(B)
    d = (i[:, None] - i[None, :]).abs()
    same = (i[:, None] // 4) == (i[None, :] // 4)
    m = torch.zeros(B, B)
    m[same & (d == 1)] = 2.0
    m[same & (d == 2)] = 1.0
    return m.to(DEV)


def steps(label, build, B, tm):
    x = torch.randn(B, 2, 128, 128, generator=torch.Generator().manual_seed(1234)).to(DEV)
    trs = []
    for ema in (None, 0.99):
        torch.manual_seed(0)
        tr = FusedTrainer(build(ema).to(DEV), lr=1e-4)
        tr.prepare(x, None, tm)
        trs.append(tr)
    off, on = (lambda: trs[0].step(x, None, tm)), (lambda: trs[1].step(x, None, tm))
    a1, a2 = alternate(off, off, args.steps)
    o, e = alternate(off, on, args.steps)
    print(f"{label}, B = {B}, medians of {args.steps} alternated captured steps (device events around step()):")
    print(f"  mode off against itself   {a1:9.4f} ms  {a2:9.4f} ms   spread {abs(a1 - a2) / min(a1, a2) * 100:.2f} %")
    print(f"  mode off / mode on        {o:9.4f} ms  {e:9.4f} ms   on / off {e / o:.4f}   ({(e - o) * 1e3:+.1f} us)")
    record[label] = {"B": B, "off_ms": [a1, a2, o], "on_ms": e}
    del trs
    torch.cuda.empty_cache()


if not args.skip_steps:
    steps("VQ_VAE default", lambda ema: dynamorph_amd.VQ_VAE(ema_decay=ema), args.batch, None)
    steps("VQ_VAE_z32 z32ex", lambda ema: dynamorph_amd.VQ_VAE_z32(weight_matching=100., margin=1., w_a=1., w_t=0.5, w_n=-0.5,
                                                                  ema_decay=ema, **EXAMPLE_CONFIG), args.z32_batch,
          tm_matrix(args.z32_batch))

print(f"the quantiser's backward alone, medians of {args.launches} alternated launches (device events):")
for route, (B, K, D, H, W) in (("MFMA one-hot", (2048, 64, 16, 16, 16)), ("LDS window", (768, 512, 64, 32, 32)),
                               ("run-time width", (512, 40, 24, 30, 30))):
    g = torch.Generator().manual_seed(2)
    z = torch.randn(B, D, H, W, generator=g).to(DEV)
    e = torch.randn(K, D, generator=g).to(DEV)
    idx = torch.randint(0, K, (B, H, W), generator=g).to(DEV)
    go = torch.randn(B, D, H, W, generator=g).to(DEV)
    gl = torch.ones(1, device=DEV)
    grad = lambda: ops.vq_backward_slabs(z, e, idx, go, gl, 0.25)      # noqa: E731
    stat = lambda: ops.vq_backward_stats(z, e, idx, go, gl, 0.25)      # noqa: E731
    g1, g2 = alternate(grad, grad, args.launches)
    gr, st = alternate(grad, stat, args.launches)
    print(f"  {route:15s} {B} x {K} x {D} x {H}x{W}: slabs against itself {g1 * 1e3:8.1f} {g2 * 1e3:8.1f} us;  "
          f"slabs {gr * 1e3:8.1f} us  stats {st * 1e3:8.1f} us   stats / slabs {st / gr:.3f}")
    record["backward " + route] = {"shape": [B, K, D, H, W], "slabs_us": [g1 * 1e3, g2 * 1e3, gr * 1e3], "stats_us": st * 1e3}
    del z, go

print(f"dm_vq_ema_apply alone, medians of {args.launches} launches (device events):")
for K, D in ((64, 16), (512, 64), (4096, 16)):
    stats = torch.rand(K * (D + 1), device=DEV)
    N, m, e = torch.ones(K, device=DEV), torch.randn(K, D, device=DEV), torch.randn(K, D, device=DEV)
    ap1, ap2 = alternate(lambda: ops.vq_ema_apply(stats, N, m, e, 0.99, 1e-5), lambda: ops.vq_ema_apply(stats, N, m, e, 0.99, 1e-5),
                         args.launches)
    print(f"  K = {K:5d}, D = {D:3d}: {ap1 * 1e3:8.1f} us  {ap2 * 1e3:8.1f} us")
    record[f"apply {K}x{D}"] = [ap1 * 1e3, ap2 * 1e3]
print(json.dumps({"emabench": record}))
