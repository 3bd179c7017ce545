#!/usr/bin/env python3
"""The row-range time-matching pair (one data-parallel rank's rows against the global batch: dm_time_matching_forward_rows /
_backward_rows) against the square pair on the whole batch, on one GPU: the default model (Bg = 2048 on 8 ranks: 256 rows,
n = 4096) and the z32 example configuration (Bg = 768: 96 rows, n = 65536).  Prints one JSON line per shape.
    python tools/tmrows_bench.py"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dynamorph_amd import ops  # noqa: E402


def t_ms(fn, iters=10, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


dev = "cuda:0"
for Bg, R, n, mode in ((2048, 256, 4096, 0), (2048, 256, 4096, 1), (768, 96, 65536, 1)):
    z = torch.randn(Bg, n, device=dev)
    tm = torch.randint(0, 3, (Bg, Bg), device=dev).float()
    args = (mode, 1.1, 0.1, -0.5, 0.5)
    r0 = Bg - R                                            # the last rank's rows
    _, S = ops.time_matching_forward(z, tm, *args)
    _, Sr = ops.time_matching_forward_rows(z, tm, r0, R, *args)
    add, add_r = torch.zeros(Bg, n, device=dev), torch.zeros(R, n, device=dev)
    rec = {"Bg": Bg, "rows": R, "n": n, "mode": mode,
           "square_forward_ms": round(t_ms(lambda: ops.time_matching_forward(z, tm, *args)), 4),
           "square_backward_ms": round(t_ms(lambda: ops.time_matching_backward(z, S, None, 0.5, add=add)), 4),
           "rows_forward_ms": round(t_ms(lambda: ops.time_matching_forward_rows(z, tm, r0, R, *args)), 4),
           "rows_backward_ms": round(t_ms(lambda: ops.time_matching_backward_rows(z, Sr, None, 0.5, add=add_r)), 4)}
    print(json.dumps(rec), flush=True)
