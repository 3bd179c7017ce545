#!/usr/bin/env python3
"""Per-patch input gradients on the MI355X: (1) host-to-host patches/s of patch_gradients beside score_patches on the same
pinned patches (the same pipeline; 131 KB per patch each way here) and beside the batch-of-one loop it replaces --
`model(x[i:i+1])` with requires_grad_() and total_loss.backward(), per-sample statistics off: a batch of one is its own
statistics -- passes alternated, medians, the spread of each side; (2) the 16 x 16 latent stage of the backward pass alone
(engine.latent_stage_backward on a per_sample context, data only), the one-launch kernel dm_latent_tail_backward against the
layer-by-layer chain, and the latent-tail forward that patch_gradients runs for the running-statistics replay, at B = 1024:
runs alternated, median and min .. max of each.

    python tools/gradbench.py [--n 8192] [--batch 1024] [--loop 256] [--passes 5] [--launches 40]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dynamorph_amd  # noqa: E402
from dynamorph_amd import engine as E, ops  # noqa: E402
from dynamorph_amd.patch_vae import patch_gradients, score_patches  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--loop", type=int, default=256)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--launches", type=int, default=40)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("gradbench: no GPU visible (rates are measured on the device or not at all)")
DEV = "cuda:0"
torch.manual_seed(0)
m = dynamorph_amd.VQ_VAE().to(DEV)
x = torch.randn(args.n, 2, 128, 128).pin_memory()
w = torch.randn(4096)
w /= w.norm()


def loop():
    """The only way to these numbers without patch_gradients: one patch at a time through the module and autograd."""
    out = np.empty((args.loop, 2, 128, 128), np.float32)
    for i in range(args.loop):
        xi = x[i:i + 1].to(DEV).requires_grad_(True)
        m(xi)[1]["total_loss"].backward()
        out[i] = xi.grad[0].cpu().numpy()
    m.zero_grad(set_to_none=True)
    return out


sides = (("patch_gradients", args.n, lambda: patch_gradients(m, x, device=DEV, batch_size=args.batch)),
         ("patch_gradients, cotangent", args.n, lambda: patch_gradients(m, x, of=w, device=DEV, batch_size=args.batch)),
         ("score_patches", args.n, lambda: score_patches(m, x, device=DEV, batch_size=args.batch)),
         ("batch-of-one loop", args.loop, loop))
for _, _, fn in sides:
    fn()                                    # one warm-up pass each
times = {name: [] for name, _, _ in sides}
for _ in range(args.passes):                # alternated: every pass of a side next to a pass of every other
    for name, _, fn in sides:
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
print(f"host to host, pinned patches 2 x 128 x 128, batch_size {args.batch}; {args.passes} alternated passes after one warm-up: "
      f"median, (max - min) / median")
rate = {}
for name, n, _ in sides:
    t = np.asarray(times[name])
    med = float(np.median(t))
    rate[name] = n / med
    print(f"  {name:28s} {n:6d} patches {med * 1e3:9.1f} ms  {n / med:10.0f} patches/s   spread {(t.max() - t.min()) / med * 100:5.1f} %")
print(f"  patch_gradients / loop {rate['patch_gradients'] / rate['batch-of-one loop']:.1f} x;  "
      f"patch_gradients / score_patches {rate['patch_gradients'] / rate['score_patches']:.2f}")

# ---- the latent stage of the backward pass alone
B = 1024
L = E.Layers(m)
xs = torch.randn(B, 2, 128, 128, generator=torch.Generator().manual_seed(1)).to(DEV)
g_z = torch.randn(B, 16, 16, 16, generator=torch.Generator().manual_seed(2)).to(DEV)
with torch.no_grad():
    _, cx = E.encoder_forward(L, xs, per_sample=True)


def chain():
    return E.latent_stage_backward(L, cx, g_z, None, want_param_grads=False, fused=False)


def fused():
    return E.latent_stage_backward(L, cx, g_z, None, want_param_grads=False)


lt_args = (cx.a3, cx.coef3, L.enc10.weight.detach(), L.enc10.bias.detach(), L.bn4.weight.detach(), L.bn4.bias.detach(), L.bn4.eps,
           [(ca.weight.detach(), ca.bias.detach(), bna.weight.detach(), bna.bias.detach(), bna.eps, cb.weight.detach(),
             cb.bias.detach(), bnb.weight.detach(), bnb.bias.detach(), bnb.eps) for ca, bna, cb, bnb in L.res])


def replay_forward():
    """What encoder_forward(replay_as_latents=True) adds to a batch: the one-launch latent tail, for its per-patch sums."""
    return ops.latent_tail_forward(*lt_args)


def alternate(fns, n):
    """n runs of every function, alternated, each run timed by its own pair of device events -> per function the times in ms."""
    for _ in range(5):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(n):
        for f, acc in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    return ts


print(f"B = {B}, per-patch statistics, {args.launches} alternated runs each (device events, launch overhead included): "
      f"median, min .. max")
with torch.no_grad():
    names = ("latent stage of the backward pass, chain (enc.12 .. enc.10, data only, eleven launches)",
             "latent stage of the backward pass, fused (dm_latent_tail_backward, one launch)",
             "latent tail forward, run for the running-statistics replay (one launch)")
    ts = alternate((chain, fused, replay_forward), args.launches)
    for name, t in zip(names, ts):
        print(f"  {name:92s} {np.median(t) * 1e3:8.1f} us  {min(t) * 1e3:8.1f} .. {max(t) * 1e3:8.1f} us")
    print(f"  fused / chain {np.median(ts[1]) / np.median(ts[0]):.3f}")
