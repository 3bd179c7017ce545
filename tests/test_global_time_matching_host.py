"""CPU: the host side of the global time-matching mode -- dist.all_gather_rows over gloo for ragged and empty shards, and the
refusal of the mode on the autograd route."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _gather_worker(rank, world, port, cases, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dynamorph_amd import dist as D
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    got = {}
    for n_global, tail, dtype in cases:
        full = torch.arange(n_global * max(1, int(torch.tensor(tail).prod())), dtype=torch.float64).reshape((n_global,) + tail)
        full = full.to(dtype)
        lo, hi = D.shard_range(n_global, rank, world)
        got[(n_global, tail, str(dtype))] = D.all_gather_rows(full[lo:hi].clone(), n_global)
        out = torch.full((n_global,) + tail, -1, dtype=dtype)
        D.all_gather_rows(full[lo:hi].clone(), n_global, out=out)
        got[(n_global, tail, str(dtype), "out")] = out
    torch.save(got, os.path.join(out_dir, f"gather{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3, 4])
def test_all_gather_rows_over_gloo(tmp_path, world):
    cases = [(7, (5,), torch.float32), (2, (3,), torch.float32), (8, (2, 3), torch.float64), (world, (4,), torch.float32),
             (1, (6,), torch.float32)]
    mp.spawn(_gather_worker, args=(world, _free_port(), cases, str(tmp_path)), nprocs=world, join=True)
    for rank in range(world):
        got = torch.load(os.path.join(tmp_path, f"gather{rank}.pt"))
        for n_global, tail, dtype in cases:
            full = torch.arange(n_global * max(1, int(torch.tensor(tail).prod())), dtype=torch.float64).reshape((n_global,) + tail)
            full = full.to(dtype)
            for key in ((n_global, tail, str(dtype)), (n_global, tail, str(dtype), "out")):
                t = got[key]
                assert t.shape == full.shape and t.dtype == dtype, (rank, key, t.shape, t.dtype)
                assert torch.equal(t, full), (rank, key)


def test_all_gather_rows_single_process_and_shard_check():
    from dynamorph_amd import dist as D
    x = torch.randn(5, 3)
    assert D.all_gather_rows(x, 5) is x
    out = torch.empty(5, 3)
    assert torch.equal(D.all_gather_rows(x, 5, out=out), x)
    with pytest.raises(ValueError):
        D.all_gather_rows(x, 6)


def test_global_time_matching_refused_on_the_autograd_route(tmp_path):
    import dynamorph_amd
    from dynamorph_amd.train import _make_optimizer, train
    model = dynamorph_amd.VQ_VAE(device="cpu")
    with pytest.raises(ValueError, match="global_time_matching"):
        _make_optimizer(model, 1e-3, fused=False, global_time_matching=True)
    with pytest.raises(ValueError, match="global_time_matching"):
        _make_optimizer(torch.nn.Linear(2, 2), 1e-3, fused=True, global_time_matching=True)
    data = torch.utils.data.TensorDataset(torch.randn(4, 2, 128, 128))
    with pytest.raises(ValueError, match="global_time_matching"):
        train(model, data, str(tmp_path), n_epochs=1, batch_size=2, device="cpu", fused=False, global_time_matching=True)
    # (the default stays what it was: a torch optimizer on this route)
    assert isinstance(_make_optimizer(model, 1e-3, fused=False), torch.optim.Adam)
