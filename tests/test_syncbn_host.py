"""CPU: the host side of synchronized BatchNorm -- dist.allreduce_payload_ over gloo (a zero placeholder contribution
included), the refusal of the mode off the fused step, and that one process ignores it."""
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


def _payload(rank, C):
    g = torch.Generator().manual_seed(100 + rank)
    return torch.cat([torch.randn(2 * C, generator=g, dtype=torch.float64), torch.tensor([float(4 + rank)], dtype=torch.float64)])


def _payload_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from dynamorph_amd import dist as D
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    got = []
    for C in (1, 16, 64):
        # the last rank only joins the exchange: its placeholder contribution is all zeros (weight 0)
        p = _payload(rank, C) if rank < world - 1 else torch.zeros(2 * C + 1, dtype=torch.float64)
        q = D.allreduce_payload_(p, None)
        assert q is p
        got.append(p.clone())
    torch.save(got, os.path.join(out_dir, f"payload{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world", [2, 3])
def test_allreduce_payload_over_gloo(tmp_path, world):
    mp.spawn(_payload_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    outs = [torch.load(os.path.join(tmp_path, f"payload{r}.pt")) for r in range(world)]
    for i, C in enumerate((1, 16, 64)):
        ref = sum(_payload(r, C) for r in range(world - 1))
        assert torch.allclose(outs[0][i], ref, rtol=1e-15, atol=1e-15), C
        assert float(outs[0][i][2 * C]) == sum(4 + r for r in range(world - 1))        # the global count
        for r in range(1, world):
            assert torch.equal(outs[r][i], outs[0][i]), (C, r)                            # every rank: the same sums


def test_allreduce_payload_single_process():
    from dynamorph_amd import dist as D
    p = torch.arange(5, dtype=torch.float64)
    assert D.allreduce_payload_(p) is p
    assert torch.equal(p, torch.arange(5, dtype=torch.float64))


def test_sync_batchnorm_refused_off_the_fused_step(tmp_path):
    import dynamorph_amd
    from dynamorph_amd.train import _make_optimizer, train
    model = dynamorph_amd.VQ_VAE(device="cpu")
    with pytest.raises(ValueError, match="sync_batchnorm"):
        _make_optimizer(model, 1e-3, fused=False, sync_batchnorm=True)
    with pytest.raises(ValueError, match="sync_batchnorm"):
        _make_optimizer(model, 1e-3, fused="graph", sync_batchnorm=True)
    with pytest.raises(ValueError, match="sync_batchnorm"):
        _make_optimizer(torch.nn.Linear(2, 2), 1e-3, fused=True, sync_batchnorm=True)
    z32 = dynamorph_amd.VQ_VAE_z32(extra_loss={"l": lambda labels, z: (z.sum(), 0.0)}, alpha=0.1).to("cpu")
    with pytest.raises(ValueError, match="sync_batchnorm"):
        _make_optimizer(z32, 1e-3, fused=True, sync_batchnorm=True)
    data = torch.utils.data.TensorDataset(torch.randn(4, 2, 128, 128))
    with pytest.raises(ValueError, match="sync_batchnorm"):
        train(model, data, str(tmp_path), n_epochs=1, batch_size=2, device="cpu", fused=False, sync_batchnorm=True)
    # (the default stays what it was)
    assert isinstance(_make_optimizer(model, 1e-3, fused=False), torch.optim.Adam)


def test_sync_batchnorm_accepted_in_one_process(monkeypatch):
    """One process: the fused route takes the flag without complaint (the trainer itself ignores it there: a GPU test
    holds its step bit-equal to the step without the flag)."""
    import dynamorph_amd
    from dynamorph_amd import train as T
    seen = {}

    class Recorder:
        def __init__(self, model, **kw):
            seen.update(kw)
    monkeypatch.setattr(T, "FusedTrainer", Recorder)
    opt = T._make_optimizer(dynamorph_amd.VQ_VAE(device="cpu"), 1e-3, fused=True, sync_batchnorm=True)
    assert isinstance(opt, Recorder) and seen["sync_batchnorm"] is True
