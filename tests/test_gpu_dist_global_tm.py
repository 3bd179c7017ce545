"""GPU: the global time-matching mode of the data-parallel step (FusedTrainer / train with global_time_matching=True),
rehearsed as ranks that share the one GPU of the box over gloo (the pattern of tests/test_gpu_dist.py).

  * Two ranks take the SAME patches X: their rank-local BatchNorm statistics are then those of [X; X], so BatchNorm drops
    out and one step of the two ranks on the global relation block [[A, C], [C, A]] must equal one process on [X; X] with
    that block -- the exchanged gradient bucket and the five scalars.  With the mode off the same comparison must fail.
  * Ragged and empty shards in train(): Bg = 7 over 2 ranks, Bg = 2 over 3 ranks."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3                     # samples per rank; the global batch is [X; X]
Z32_EXAMPLE = dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512)
NOISE_BIASES = ("enc.1.bias", "enc.4.bias", "enc.7.bias", "enc.10.bias", ".1.bias", ".4.bias")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      DM_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    from dynamorph_amd import dist as D
    D.init_from_env()
    torch.cuda.set_device(0)


def _model(kind):
    import dynamorph_amd
    torch.manual_seed(77)
    if kind == "VQ_VAE":
        return dynamorph_amd.VQ_VAE().to("cuda")
    if kind == "VQ_VAE_z16":
        return dynamorph_amd.VQ_VAE_z16().to("cuda")
    return dynamorph_amd.VQ_VAE_z32(**Z32_EXAMPLE).to("cuda")


def _inputs():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, 2, 128, 128, generator=g)
    a = torch.randint(0, 3, (B, B), generator=g).float()
    a = torch.triu(a, 1) + torch.triu(a, 1).T
    c = torch.randint(0, 3, (B, B), generator=g).float()
    c = torch.triu(c) + torch.triu(c, 1).T
    tm = torch.cat([torch.cat([a, c], 1), torch.cat([c, a], 1)], 0)
    return x, tm


def _step_worker(rank, world, port, kind, out_dir):
    _init(rank, world, port)
    import torch.distributed as dist
    from dynamorph_amd.train import FusedTrainer
    x, tm = _inputs()
    x, tm = x.cuda(), tm.cuda()
    res = {}
    for use_graph in (True, False):
        for flag in (True, False):
            tr = FusedTrainer(_model(kind), lr=1e-3, use_graph=use_graph, global_time_matching=flag)
            # mode off: what train() hands a rank by default -- the block of its own shard
            block = tm if flag else tm[rank * B:(rank + 1) * B, rank * B:(rank + 1) * B].contiguous()
            vals = tr.step(x, None, block)
            # captured programs: the global step is 2 segments (cut at the gather), the plain step ONE graph
            segs = len(tr._graphs[(tuple(x.shape), None, tuple(block.shape))]["train"][0].graphs) if use_graph else 0
            res[(use_graph, flag)] = (vals.cpu(), tr.grad.cpu().clone(), segs)      # the bucket after the exchange (sum)
    if rank == 0:
        torch.save(res, os.path.join(out_dir, "ranks.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _mismatch(vals, grad, ref_vals, ref_grad, names):
    """Why the two-rank step differs from the one-process step (None: it does not), under the gates of the repository's
    trainer comparisons: losses within 1e-5 (relative above 1), gradients within fp32 accumulation noise."""
    for i in range(5):
        r = float(ref_vals[i])
        if abs(float(vals[i]) - r) > 1e-5 * max(1.0, abs(r)):
            return f"scalar {i}: {float(vals[i])} vs {r}"
    for name, (lo, hi) in names.items():
        if any(name.endswith(s) for s in NOISE_BIASES):
            continue
        g, gr = grad[lo:hi], ref_grad[lo:hi]
        scale = float(gr.abs().max()) + 1e-12
        if float((g - gr).abs().max()) > 1e-3 * scale:
            return f"gradient {name}: {float((g - gr).abs().max())} vs scale {scale}"
    return None


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["VQ_VAE", "VQ_VAE_z16", "VQ_VAE_z32"])
def test_two_ranks_duplicate_shards_equal_one_process(tmp_path, kind):
    world = 2
    mp.spawn(_step_worker, args=(world, _free_port(), kind, str(tmp_path)), nprocs=world, join=True)
    got = torch.load(os.path.join(tmp_path, "ranks.pt"))
    from dynamorph_amd.train import FusedTrainer
    x, tm = _inputs()
    xx = torch.cat([x, x]).cuda()
    model = _model(kind)
    names, off = {}, 0
    for name, p in model.named_parameters():
        if p.requires_grad:
            names[name] = (off, off + p.numel())
            off += p.numel()
    ref = FusedTrainer(model, lr=1e-3, use_graph=False)
    ref_vals = ref.step(xx, None, tm.cuda()).cpu()
    ref_grad = ref.grad.cpu()
    for use_graph in (True, False):
        vals, bucket, _ = got[(use_graph, True)]
        why = _mismatch(vals, bucket / world, ref_vals, ref_grad, names)     # (Adam's load applies the 1 / world)
        assert why is None, (kind, use_graph, why)
        vals, bucket, _ = got[(use_graph, False)]
        assert _mismatch(vals, bucket / world, ref_vals, ref_grad, names) is not None, (kind, use_graph)
    for flag, segs in ((True, 2), (False, 1)):
        assert got[(True, flag)][2] == segs, (kind, flag, got[(True, flag)][2])
        # the captured step and the eager step run one body: bit-equal scalars and exchanged bucket
        assert torch.equal(got[(True, flag)][0], got[(False, flag)][0]), (kind, flag)
        assert torch.equal(got[(True, flag)][1], got[(False, flag)][1]), (kind, flag)


def _relation(n, seed):
    import scipy.sparse as sp
    g = np.random.RandomState(seed)
    t = g.randint(0, 3, size=(n, n)).astype(np.float32)
    t = np.triu(t, 1) + np.triu(t, 1).T
    return sp.csr_matrix(t)


def _train_worker(rank, world, port, n_samples, val_ratio, batch, feed, out_dir):
    _init(rank, world, port)
    import dynamorph_amd
    import torch.distributed as dist
    from dynamorph_amd import dist as D
    from dynamorph_amd import engine as E
    from dynamorph_amd.train import train
    model = _model("VQ_VAE")
    data = torch.utils.data.TensorDataset(torch.randn(n_samples, 2, 128, 128, generator=torch.Generator().manual_seed(5)))
    rel = _relation(n_samples, 9)
    seen = {}

    def probe(phase, epoch, ids, x, kw):
        # the latents this rank's step is about to act on (pre-step parameters, rank-local BatchNorm statistics)
        if phase != "train":
            return
        bufs = [b.clone() for b in model.buffers()]
        with torch.no_grad():
            z, _ = E.encoder_forward(E.Layers(model), x.contiguous())
        for b, s in zip(model.buffers(), bufs):
            b.copy_(s)
        seen["z"] = z.reshape(z.shape[0], -1).cpu().clone()
        seen["ids"] = np.asarray(ids).copy()
        seen["tm"] = kw["time_matching_mat"].cpu().clone()

    stats = {}
    np.random.seed(3)
    train(model, data, os.path.join(out_dir, "run"), relation_mat=rel, n_epochs=1, lr=1e-3, batch_size=batch, device="cuda:0",
          val_split_ratio=val_ratio, patience=None if val_ratio is None else 5, feed=feed, stats=stats, probe=probe,
          global_time_matching=True)
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters() if p.requires_grad])
    ev = D.collective_evidence(flat)
    torch.save({"ev": ev, "steps": stats["step_losses"]["train"][0], "seen": seen},
               os.path.join(out_dir, f"train{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("world,n_samples,val_ratio,batch,feed", [(2, 8, 0.125, 7, "resident"), (3, 3, 0.34, 2, "sync")])
def test_train_ragged_and_empty_shards(tmp_path, world, n_samples, val_ratio, batch, feed):
    """One train() epoch with the global term: every rank completes it (the empty shards join the collectives), replicas
    stay bit-equal, and the step's time-matching value -- what the epoch record prints -- is the one-process value of the
    global term on the gathered latents (float64 from the reference formula, mode 0: sum of sim * tm)."""
    mp.spawn(_train_worker, args=(world, _free_port(), n_samples, val_ratio, batch, feed, str(tmp_path)), nprocs=world,
             join=True)
    outs = [torch.load(os.path.join(tmp_path, f"train{r}.pt"), weights_only=False) for r in range(world)]
    assert outs[0]["ev"]["replicas_bit_equal"] and outs[0]["ev"]["world"] == world
    with_data = [o for o in outs if o["seen"]]
    assert len(with_data) == min(world, batch)
    zs = torch.cat([o["seen"]["z"] for o in with_data]).double()
    tm = with_data[0]["seen"]["tm"].double()
    assert tm.shape == (batch, batch)
    for o in with_data:
        assert torch.equal(o["seen"]["tm"], with_data[0]["seen"]["tm"])     # every rank: the global block
    diff = zs[:, None, :] - zs[None, :, :]
    ref = float(((diff * diff).mean(2) * tm).sum())
    for o in with_data:
        assert len(o["steps"]) == 1
        got = o["steps"][0]["time_matching_loss"]
        assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), (got, ref)
