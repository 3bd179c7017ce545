#!/usr/bin/env python3
"""Two ranks sharing one GPU over gloo take captured FusedTrainer steps with sync_batchnorm on or off: one JSON line per
(model, flag) with the wall time per step and the number of replayed segments.  Gloo on one GPU moves every payload through
host memory and says nothing about RCCL latency; the run is for kernel traces (the added launches per step and their time):
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/syncbn_rehearsal.py --steps 20
    python tools/syncbn_rehearsal.py --models VQ_VAE --flags 1"""
import argparse
import json
import os
import socket
import sys
import time

import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, args):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      DM_DIST_BACKEND="gloo")
    import dynamorph_amd
    from dynamorph_amd import dist as D
    from dynamorph_amd.train import FusedTrainer
    D.init_from_env()
    torch.cuda.set_device(0)
    for kind in args.models.split(","):
        for flag in (int(f) for f in args.flags.split(",")):
            torch.manual_seed(0)
            model = (dynamorph_amd.VQ_VAE() if kind == "VQ_VAE" else
                     dynamorph_amd.VQ_VAE_z32(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512)).to("cuda")
            tr = FusedTrainer(model, use_graph=True, sync_batchnorm=bool(flag))
            x = torch.randn(args.batch, 2, 128, 128, device="cuda") * (1 + rank) + rank
            for _ in range(3):
                tr.step(x)
            torch.cuda.synchronize()
            D.barrier()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.step(x)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            segs = len(tr._graphs[(tuple(x.shape), None, None)]["train"][0].graphs)
            if rank == 0:
                print(json.dumps({"model": kind, "sync_batchnorm": bool(flag), "world": world, "batch_per_rank": args.batch,
                                  "steps": args.steps, "segments": segs, "ms_per_step_gloo": round(ms, 3)}), flush=True)
    D.barrier()
    torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="VQ_VAE,VQ_VAE_z32")
    ap.add_argument("--flags", default="1,0")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_worker, args=(2, port, args), nprocs=2, join=True)


if __name__ == "__main__":
    main()
