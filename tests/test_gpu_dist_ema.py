"""GPU: the EMA codebook mode under data parallelism, rehearsed as 2 ranks that share the one GPU over gloo (as
tests/test_gpu_dist.py spawns them).  The update's statistics ride the step's one all-reduce as plain sums over the ranks:
neither grad_weight nor Adam's 1 / world touches them, a rank without data adds zeros and still applies the update, and
rank 0's frozen codebook -- which is in neither the flat buffer nor model.buffers() -- reaches every rank at start."""
import os
import socket
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, DECAY = 1e-3, 0.9
EMA_KEYS = ("vq.w.weight", "vq.ema_cluster_size", "vq.ema_w")
SPAWN_LIMIT = 240          # seconds for the one spawn that runs every scenario


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _global_batch():
    return torch.randn(6, 2, 128, 128, generator=torch.Generator().manual_seed(5))


def _seeded_model(seed, dev):
    import dynamorph_amd
    torch.manual_seed(seed)
    return dynamorph_amd.VQ_VAE(ema_decay=DECAY).to(dev)


def _ema_state(model):
    sd = model.state_dict()
    return {k: sd[k].detach().cpu().clone() for k in EMA_KEYS}


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", DM_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from dynamorph_amd import dist as D
    from dynamorph_amd.train import FusedTrainer
    D.init_from_env()
    dev = "cuda:0"
    torch.cuda.set_device(0)
    out = {}

    # ---- A: different replicas, different data; one collective per step
    model = _seeded_model(900 + rank, dev)
    out["A_own_codebook"] = model.vq.w.weight.detach().cpu().clone()
    tr = FusedTrainer(model, lr=LR)
    out["A_start"] = _ema_state(model)
    calls = [0]
    orig = dist.all_reduce

    def counted(*a, **kw):
        calls[0] += 1
        return orig(*a, **kw)
    dist.all_reduce = counted
    x = torch.randn(6, 2, 128, 128, generator=torch.Generator().manual_seed(70 + rank)).to(dev)
    per_step = []
    for _ in range(2):
        before = calls[0]
        tr.step(x)
        per_step.append(calls[0] - before)
    dist.all_reduce = orig
    torch.cuda.synchronize()
    out["A_calls"] = per_step
    out["A_flat"] = tr.flat.detach().cpu().clone()
    out["A_end"] = _ema_state(model)

    # ---- B: the global batch with synchronized BatchNorm, 2 ranks x 3 samples
    model = _seeded_model(910, dev)
    tr = FusedTrainer(model, lr=LR, sync_batchnorm=True)
    xg = _global_batch()
    tr.step(xg[3 * rank:3 * rank + 3].to(dev))
    torch.cuda.synchronize()
    out["B_end"] = _ema_state(model)

    # ---- C: a ragged 3 + 0 step: rank 0 holds the whole global batch, rank 1 nothing
    model = _seeded_model(920, dev)
    tr = FusedTrainer(model, lr=LR)
    if rank == 0:
        tr.step(xg[:3].to(dev), grad_weight=3 * world / 3.0)
    else:
        tr.step_without_data()
    torch.cuda.synchronize()
    out["C_end"] = _ema_state(model)
    out["C_flat"] = tr.flat.detach().cpu().clone()

    # ---- the autograd route with more than one rank says no
    model = _seeded_model(930, dev)
    try:
        model(xg[:2].to(dev))
        out["autograd_refusal"] = None
    except ValueError as e:
        out["autograd_refusal"] = str(e)
    torch.save(out, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(tmp_path_factory):
    """Both ranks' results of the one spawn; the spawn runs under a time limit of its own."""
    out_dir = str(tmp_path_factory.mktemp("dist_ema"))
    world = 2
    ctx = mp.spawn(_worker, args=(world, _free_port(), out_dir), nprocs=world, join=False)
    deadline = time.monotonic() + SPAWN_LIMIT
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail(f"the two ranks did not finish within {SPAWN_LIMIT} s")
    return [torch.load(os.path.join(out_dir, f"rank{r}.pt")) for r in range(world)]


def test_replicas_agree(ranks):
    r0, r1 = ranks
    assert not torch.equal(r0["A_own_codebook"], r1["A_own_codebook"])          # the replicas did start apart
    for k in EMA_KEYS:
        assert torch.equal(r1["A_start"][k], r0["A_start"][k]), k                # rank 0's replica wins, codebook included
    assert torch.equal(r0["A_start"]["vq.w.weight"], r0["A_own_codebook"])
    assert torch.equal(r0["A_start"]["vq.ema_w"], r0["A_own_codebook"])
    assert torch.equal(r0["A_flat"], r1["A_flat"])
    for k in EMA_KEYS:
        assert torch.equal(r0["A_end"][k], r1["A_end"][k]), k
    assert not torch.equal(r0["A_end"]["vq.w.weight"], r0["A_start"]["vq.w.weight"])


def test_one_collective_per_step(ranks):
    for r in ranks:
        assert r["A_calls"] == [1, 1]


def test_global_batch_with_sync_batchnorm(ranks):
    """2 ranks x 3 samples against one process x 6 samples.  The two are the same sums split differently, so they agree to
    rounding: the floor of the model test's gate, 2e-4 of the tensor's scale (there is no oracle error to take 1.5 x of)."""
    from dynamorph_amd.train import FusedTrainer
    model = _seeded_model(910, "cuda:0")
    FusedTrainer(model, lr=LR, use_graph=False).step(_global_batch().to("cuda:0"))
    want = _ema_state(model)
    n_moved = 0
    for k in EMA_KEYS:
        assert torch.equal(ranks[0]["B_end"][k], ranks[1]["B_end"][k]), k
        scale = max(float(want[k].abs().max()), 1e-6)
        err = float((ranks[0]["B_end"][k].double() - want[k].double()).abs().max())
        print(f"global batch {k}: error {err:.3e}, scale {scale:.3e}")
        assert err <= 2e-4 * scale, (k, err, scale)
    # the counts are integers over the GLOBAL batch: N = decay + (1 - decay) n with sum n = 6 x 256 positions
    n = (want["vq.ema_cluster_size"].double() - DECAY) / (1.0 - DECAY)
    assert abs(float(n.sum()) - 6 * 256) < 1e-2
    n2 = (ranks[0]["B_end"]["vq.ema_cluster_size"].double() - DECAY) / (1.0 - DECAY)
    assert abs(float(n2.sum()) - 6 * 256) < 1e-2


def test_ragged_batch(ranks):
    """3 + 0: the codebook of both ranks is the one process's on the 3 samples, to the bit -- the statistics are rank 0's
    plus zeros, unscaled by grad_weight = 2 and by Adam's 1 / world."""
    from dynamorph_amd.train import FusedTrainer
    model = _seeded_model(920, "cuda:0")
    tr = FusedTrainer(model, lr=LR)
    tr.step(_global_batch()[:3].to("cuda:0"))
    want = _ema_state(model)
    for k in EMA_KEYS:
        assert torch.equal(ranks[0]["C_end"][k], ranks[1]["C_end"][k]), k
        assert torch.equal(ranks[0]["C_end"][k], want[k]), k
    assert torch.equal(ranks[0]["C_flat"], ranks[1]["C_flat"])


def test_autograd_route_refuses_more_than_one_rank(ranks):
    for r in ranks:
        assert r["autograd_refusal"] and "FusedTrainer" in r["autograd_refusal"]
