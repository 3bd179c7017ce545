#!/usr/bin/env python3
"""Per-patch scoring on the MI355X: (1) host-to-host patches/s of score_patches beside encode_patches on the same pinned
patches (the ceiling: same pipeline, strictly less work) and beside the batch-of-one `model(sample)` loop it replaces;
(2) dm_dec_tail_score with decoded = NULL against dm_dec_tail_forward at B = 1024, alternated in one process, medians of the
launches' device-event times, and dm_dec_tail_forward against itself for the spread.

    python tools/scorebench.py [--n 8192] [--batch 1024] [--loop 256] [--launches 40]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dynamorph_amd  # noqa: E402
from dynamorph_amd import ops  # noqa: E402
from dynamorph_amd.patch_vae import encode_patches, score_patches  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--loop", type=int, default=256)
ap.add_argument("--launches", type=int, default=40)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("scorebench: no GPU visible (rates are measured on the device or not at all)")
DEV = "cuda:0"
torch.manual_seed(0)
m = dynamorph_amd.VQ_VAE().to(DEV)
x = torch.randn(args.n, 2, 128, 128).pin_memory()


def best_of(fn, reps=3):
    fn()
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


print(f"host to host, N = {args.n} pinned patches 2 x 128 x 128, batch_size {args.batch} (best of 3 after one warm-up pass)")
for name, fn in (("encode_patches", lambda: encode_patches(m, x, device=DEV, batch_size=args.batch)),
                 ("score_patches", lambda: score_patches(m, x, device=DEV, batch_size=args.batch)),
                 ("score_patches + counts", lambda: score_patches(m, x, device=DEV, batch_size=args.batch, return_code_counts=True)),
                 ("score_patches + decoded", lambda: score_patches(m, x, device=DEV, batch_size=args.batch, return_decoded=True))):
    t = best_of(fn)
    print(f"  {name:26s} {t * 1e3:8.1f} ms  {args.n / t:10.0f} patches/s")


def loop():
    out = []
    with torch.no_grad():
        for i in range(args.loop):
            _, ld = m(x[i:i + 1].to(DEV))
            out.append(float(ld["recon_loss"]))
    return out


t = best_of(loop, reps=2)
print(f"  {'model(sample) loop':26s} {t * 1e3:8.1f} ms  {args.loop / t:10.0f} patches/s   ({args.loop} patches, one at a time)")

# ---- the tail kernels alone
B = 1024
g = torch.Generator().manual_seed(1)
d2 = torch.randn(B, 4, 64, 64, generator=g).clamp(min=0).to(DEV)
w4, b4 = (torch.randn(4, 4, 4, 4, generator=g) * 0.3).to(DEV), torch.randn(4, generator=g).to(DEV)
w6, b6 = torch.randn(2, 4, generator=g).to(DEV), torch.randn(2, generator=g).to(DEV)
xs = torch.randn(B, 2, 128, 128, generator=g).to(DEV)
var = torch.tensor([0.5, 1.5], device=DEV)
lib = ops.L.load()
st = torch.cuda.current_stream().cuda_stream
dec = torch.empty(B, 2, 128, 128, device=DEV)
slabs = torch.empty(lib.dm_dec_tail_num_blocks(B, 64, 64), device=DEV, dtype=torch.float64)
wsb = lib.dm_dec_tail_score_workspace_bytes(B, 2, 64, 64)
ws = torch.empty(wsb // 8, device=DEV, dtype=torch.float64)
sums = torch.empty(B, 2, device=DEV, dtype=torch.float64)
P = lambda t: t.data_ptr()  # noqa: E731


def forward():
    assert lib.dm_dec_tail_forward(P(d2), P(w4), P(b4), P(w6), P(b6), P(xs), None, 0, P(var), P(dec), P(slabs), B, 4, 2, 64, 64, st) == 0


def score():
    assert lib.dm_dec_tail_score(P(d2), P(w4), P(b4), P(w6), P(b6), P(xs), None, 0, P(var), None, P(sums), P(ws), wsb, B, 4, 2,
                                 64, 64, st) == 0


def alternate(fa, fb, n):
    """n launches each of fa and fb, alternated, every launch timed by its own pair of device events -> (median a, median b) ms."""
    for _ in range(5):
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


f1, f2 = alternate(forward, forward, args.launches)
fw, sc = alternate(forward, score, args.launches)
print(f"decoder tail alone, B = {B}, 2 x 128 x 128, no mask, medians of {args.launches} alternated launches (device events):")
print(f"  dm_dec_tail_forward against itself      {f1 * 1e3:8.1f} us  {f2 * 1e3:8.1f} us   spread {abs(f1 - f2) / min(f1, f2) * 100:.2f} %")
print(f"  dm_dec_tail_forward / dm_dec_tail_score {fw * 1e3:8.1f} us  {sc * 1e3:8.1f} us   score / forward {sc / fw:.3f}"
      f"   (score: two launches, decoded = NULL; {B * 196608 / sc / 1e6:.0f} GB/s of 196 608 B/patch)")
