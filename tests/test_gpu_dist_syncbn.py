"""GPU: synchronized BatchNorm in the data-parallel step (FusedTrainer / train with sync_batchnorm=True), rehearsed as ranks
that share the one GPU of the box over gloo (the pattern of tests/test_gpu_dist_global_tm.py).

  * Two ranks on DIFFERENT patches (rank 1's drawn with a shifted mean and scale) equal one process on their concatenation:
    the losses, the exchanged gradient bucket and every BatchNorm's running statistics -- with the flag off they do not.
  * Both flags together (global time matching as well) equal one process on the concatenation with the global block.
  * Ragged shards (4 + 3) with the trainer's gradient weights.
  * train() with ragged and empty shards: every rank finishes, replicas and all buffers stay bit-equal, model.pt holds them.
  * The new kernels alone against dm_bn_finalize / dm_bn_backward_finalize, and the flag in one process."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3                     # samples per rank in the step comparisons
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


def _samples(sizes):
    """One block of patches per rank; every block after the first drawn with a shifted mean and a larger scale, so the
    ranks' own BatchNorm statistics differ clearly from the global batch's.  Also the global relation block."""
    g = torch.Generator().manual_seed(21)
    xs = [torch.randn(n, 2, 128, 128, generator=g) * (1.0 + 1.5 * r) + 1.5 * r for r, n in enumerate(sizes)]
    n = sum(sizes)
    t = torch.randint(0, 3, (n, n), generator=g).float()
    return xs, torch.triu(t, 1) + torch.triu(t, 1).T


def _buffers(model):
    return {k: b.detach().cpu().clone() for k, b in model.named_buffers()}


def _names(model):
    names, off = {}, 0
    for name, p in model.named_parameters():
        if p.requires_grad:
            names[name] = (off, off + p.numel())
            off += p.numel()
    return names


def _mismatch(vals, grad, ref_vals, ref_grad, names, idx):
    """Why the ranks' step differs from the one-process step (None: it does not), under the gates of the repository's
    trainer comparisons: losses within 1e-5 (relative above 1), gradients within fp32 accumulation noise.  vals: the ranks'
    scalars weighted by their share of the batch (every loss is a mean over the local shard); idx: the scalars compared --
    perplexity is a statistic of the rank's own codes and has no share-weighted form."""
    for i in idx:
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


def _buffer_mismatch(bufs, ref):
    for k, r in ref.items():
        b = bufs[k]
        if k.endswith("num_batches_tracked") or not r.is_floating_point():
            if not torch.equal(b, r):
                return f"{k}: {b} vs {r}"
        elif not torch.allclose(b, r, rtol=1e-5, atol=1e-6):
            return f"{k}: {float((b - r).abs().max())}"
    return None


# ------------------------------------------------------------------------------------------------ step comparisons
def _step_worker(rank, world, port, kind, sizes, modes, out_dir):
    _init(rank, world, port)
    import torch.distributed as dist
    from dynamorph_amd import dist as D
    from dynamorph_amd.train import FusedTrainer
    xs, tm = _samples(sizes)
    x, tm = xs[rank].cuda(), tm.cuda()
    n = sum(sizes)
    w = D.shard_weight(n, rank, world)
    res = {}
    for use_graph in (True, False):
        for mode in modes:
            tr = FusedTrainer(_model(kind), lr=1e-3, use_graph=use_graph, sync_batchnorm=mode != "off",
                              global_time_matching=mode == "both")
            block = tm if mode == "both" else None
            vals = tr.step(x, None, block, grad_weight=w)
            key = (tuple(x.shape), None, None if block is None else tuple(block.shape))
            segs = len(tr._graphs[key]["train"][0].graphs) if use_graph else 0
            res[(use_graph, mode)] = (vals.cpu(), tr.grad.cpu().clone(), _buffers(tr.model), segs)
    torch.save(res, os.path.join(out_dir, f"ranks{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _run_steps(tmp_path, kind, sizes, modes):
    world = len(sizes)
    mp.spawn(_step_worker, args=(world, _free_port(), kind, sizes, modes, str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(os.path.join(tmp_path, f"ranks{r}.pt")) for r in range(world)]
    from dynamorph_amd.train import FusedTrainer
    xs, tm = _samples(sizes)
    xx = torch.cat(xs).cuda()
    refs = {}
    for with_tm in (False, True):
        if with_tm and "both" not in modes:
            continue
        ref = FusedTrainer(_model(kind), lr=1e-3, use_graph=False)
        vals = ref.step(xx, None, tm.cuda() if with_tm else None)
        refs[with_tm] = (vals.cpu(), ref.grad.cpu(), _buffers(ref.model))
    share = [n / sum(sizes) for n in sizes]

    def compare(use_graph, mode):
        ref_vals, ref_grad, ref_bufs = refs[mode == "both"]
        vals = sum(s * got[r][(use_graph, mode)][0] for r, s in enumerate(share))
        bucket = got[0][(use_graph, mode)][1]
        idx = (0, 1, 2, 4) if mode == "both" else (0, 1, 2)
        why = _mismatch(vals, bucket / world, ref_vals, ref_grad, _names(_model(kind)), idx)
        return why or _buffer_mismatch(got[0][(use_graph, mode)][2], ref_bufs)

    # captured segments: cut at each BatchNorm exchange (16 for VQ_VAE / VQ_VAE_z16, 22 for VQ_VAE_z32) and at the gather
    exchanges = 22 if kind == "VQ_VAE_z32" else 16
    for mode in modes:
        segs = {"off": 1, "sync": exchanges + 1, "both": exchanges + 2}[mode]
        for r in range(world):
            assert got[r][(True, mode)][3] == segs, (kind, mode, r, got[r][(True, mode)][3])
            # the captured step and the eager step run one body: bit-equal scalars, bucket and BatchNorm buffers
            ge, gg = got[r][(False, mode)], got[r][(True, mode)]
            assert torch.equal(gg[0], ge[0]) and torch.equal(gg[1], ge[1]), (kind, mode, r)
            for k, b in ge[2].items():
                assert torch.equal(gg[2][k], b), (kind, mode, r, k)
    for use_graph in (True, False):
        for mode in modes:
            if mode == "off":
                assert compare(use_graph, mode) is not None, (kind, use_graph)
                continue
            why = compare(use_graph, mode)
            assert why is None, (kind, use_graph, mode, why)
            for r in range(1, world):                                   # the replicas' buffers: bit-equal
                for k, b in got[0][(use_graph, mode)][2].items():
                    assert torch.equal(got[r][(use_graph, mode)][2][k], b), (kind, use_graph, mode, r, k)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["VQ_VAE", "VQ_VAE_z16", "VQ_VAE_z32"])
def test_distinct_shards_equal_one_process(tmp_path, kind):
    """Tests 1 and 2 of the feature: sync_batchnorm alone (and off: the comparison must fail), and together with
    global_time_matching against one process on the concatenation with the global relation block."""
    _run_steps(tmp_path, kind, (B, B), ("sync", "off", "both"))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["VQ_VAE", "VQ_VAE_z32"])
def test_ragged_shards_equal_one_process(tmp_path, kind):
    """Shards of 4 and 3, each rank stepping with grad_weight = shard_weight(7, rank, 2): the batch terms of the BatchNorm
    backward divide by w_r * N, so the exchanged bucket is the one-process gradient on the 7 samples."""
    _run_steps(tmp_path, kind, (4, 3), ("sync",))


# ------------------------------------------------------------------------------------------------ train()
def _relation(n, seed):
    import scipy.sparse as sp
    g = np.random.RandomState(seed)
    t = g.randint(0, 3, size=(n, n)).astype(np.float32)
    t = np.triu(t, 1) + np.triu(t, 1).T
    return sp.csr_matrix(t)


def _train_worker(rank, world, port, n_samples, val_ratio, batch, feed, global_tm, out_dir):
    _init(rank, world, port)
    import torch.distributed as dist
    from dynamorph_amd.train import train
    model = _model("VQ_VAE")
    g = torch.Generator().manual_seed(5)
    data = torch.utils.data.TensorDataset(torch.randn(n_samples, 2, 128, 128, generator=g) * 2.0 + 0.5)
    np.random.seed(3)
    train(model, data, os.path.join(out_dir, "run"), relation_mat=_relation(n_samples, 9), n_epochs=1, lr=1e-3,
          batch_size=batch, device="cuda:0", val_split_ratio=val_ratio, patience=5, feed=feed,
          global_time_matching=global_tm, sync_batchnorm=True)
    flat = torch.cat([p.detach().reshape(-1) for p in model.parameters() if p.requires_grad]).cpu()
    torch.save({"flat": flat, "bufs": _buffers(model)}, os.path.join(out_dir, f"train{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("global_tm", [False, True])
@pytest.mark.parametrize("world,n_samples,val_ratio,batch,feed", [(2, 8, 0.125, 7, "resident"), (3, 3, 0.34, 2, "sync")])
def test_train_ragged_and_empty_shards(tmp_path, world, n_samples, val_ratio, batch, feed, global_tm):
    """One train() epoch: ragged shards (4 + 3) and empty ones (a rank without data in training or validation joins every
    exchange on a zero-weight placeholder).  Every rank finishes; parameters and ALL buffers are bit-equal across ranks;
    rank 0's model.pt holds the same buffers."""
    mp.spawn(_train_worker, args=(world, _free_port(), n_samples, val_ratio, batch, feed, global_tm, str(tmp_path)),
             nprocs=world, join=True)
    outs = [torch.load(os.path.join(tmp_path, f"train{r}.pt")) for r in range(world)]
    ckpt = torch.load(os.path.join(tmp_path, "run", "model.pt"), map_location="cpu")
    for r in range(world):
        assert torch.equal(outs[r]["flat"], outs[0]["flat"]), r
        for k, b in outs[0]["bufs"].items():
            assert torch.equal(outs[r]["bufs"][k], b), (r, k)
            assert torch.equal(ckpt[k].cpu(), outs[r]["bufs"][k]), (r, k)
    assert int(outs[0]["bufs"]["enc.2.num_batches_tracked"]) == 2          # one training step + one validation pass


# ------------------------------------------------------------------------------------------------ kernels alone
def _ulps(a, b):
    a, b = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    return int((a - b).abs().max())


@pytest.mark.parametrize("C,nslabs", [(16, 37), (300, 5)])
def test_payload_kernels_against_the_batch_finalize(C, nslabs):
    from dynamorph_amd import ops
    dev = "cuda"
    g = torch.Generator().manual_seed(C)
    count = nslabs * 64
    x = torch.randn(nslabs, C, 64, generator=g, dtype=torch.float64) * 1.7 + 0.3
    stats = torch.stack([x.sum(2), (x * x).sum(2)], 2).to(dev)
    other = (torch.randn(nslabs, C, 2, generator=g, dtype=torch.float64) * 50).to(dev)
    gamma = (torch.rand(C, generator=g) + 0.5).to(dev)
    beta = torch.randn(C, generator=g).to(dev)
    rm0 = torch.randn(C, generator=g).to(dev)
    rv0 = (torch.rand(C, generator=g) + 0.5).to(dev)
    one = torch.ones(1, dtype=torch.float64, device=dev)
    zero = torch.zeros(1, dtype=torch.float64, device=dev)

    def state():
        return rm0.clone(), rv0.clone(), torch.zeros(1, dtype=torch.int64, device=dev)

    rm1, rv1, nbt1 = state()
    coef1, saved1 = ops.bn_finalize(stats, count, gamma, beta, rm1, rv1, nbt1, 0.1, 1e-5)
    # weight 1, plus a placeholder's zero contribution (weight 0) added as the all-reduce would
    p0 = ops.bn_sync_pack(other, 5, zero)
    assert p0.shape == (2 * C + 1,) and not p0.any()
    payload = ops.bn_sync_pack(stats, count, one) + p0
    rm2, rv2, nbt2 = state()
    coef2, saved2 = ops.bn_finalize_payload(payload, gamma, beta, rm2, rv2, nbt2, 0.1, 1e-5)
    torch.cuda.synchronize()
    assert float(payload[2 * C]) == count
    assert _ulps(coef2, coef1) <= 1 and _ulps(saved2, saved1) <= 1
    assert torch.equal(rm2, rm1) and torch.equal(rv2, rv1) and int(nbt2) == int(nbt1) == 1

    # backward: (sum dy, sum dy * a) slabs
    dy = torch.randn(nslabs, C, 64, generator=g, dtype=torch.float64)
    bstats = torch.stack([dy.sum(2), (dy * x).sum(2)], 2).to(dev)
    dg1, db1 = torch.empty(C, device=dev), torch.empty(C, device=dev)
    cb1 = ops.bn_backward_finalize(bstats, count, gamma, saved1, dg1, db1)
    dg2, db2 = torch.empty(C, device=dev), torch.empty(C, device=dev)
    bp = ops.bn_backward_pack(bstats, saved1, one, dg2, db2)
    cb2 = ops.bn_backward_payload(bp, payload, gamma, saved1, one)
    torch.cuda.synchronize()
    assert torch.equal(dg2, dg1) and torch.equal(db2, db1)
    assert _ulps(cb2, cb1) <= 1

    # a ragged gradient weight w: the payload carries w * sums and the batch terms divide by w * N -- the same coefficients
    w = torch.full((1,), 6.0 / 7.0, dtype=torch.float64, device=dev)
    bpw = ops.bn_backward_pack(bstats, saved1, w, dg2, db2)
    cbw = ops.bn_backward_payload(bpw, payload, gamma, saved1, w)
    torch.cuda.synchronize()
    assert torch.allclose(bpw, bp * (6.0 / 7.0), rtol=1e-15, atol=0)
    assert torch.equal(dg2, dg1) and torch.equal(db2, db1)           # dgamma / dbeta: the local sums, unweighted
    assert torch.allclose(cbw, cb1, rtol=1e-6, atol=1e-7)
    # weight 0 (a rank without data): zero payload, and da = scale * dy
    bp0 = ops.bn_backward_pack(bstats, saved1, zero, dg2, db2)
    cb0 = ops.bn_backward_payload(bp0, payload, gamma, saved1, zero)
    torch.cuda.synchronize()
    assert not bp0.any()
    assert torch.equal(cb0[:, 0], cb1[:, 0]) and not cb0[:, 1:].any()

    # two contributions summed: the global count's statistics and the N / (N - 1) factor of the running variance
    both = ops.bn_sync_pack(stats, count, one) + ops.bn_sync_pack(stats[:2].contiguous(), 128, one)
    rm3, rv3, nbt3 = state()
    ops.bn_finalize_payload(both, gamma, beta, rm3, rv3, nbt3, 0.1, 1e-5)
    allx = torch.cat([x.permute(1, 0, 2).reshape(C, -1), x[:2].permute(1, 0, 2).reshape(C, -1)], 1)
    n = allx.shape[1]
    assert float(both[2 * C]) == n
    mean, var = allx.mean(1), allx.var(1, unbiased=True)
    torch.cuda.synchronize()
    assert torch.allclose(rm3.cpu().double(), 0.1 * mean + 0.9 * rm0.cpu().double(), rtol=1e-5, atol=1e-6)
    assert torch.allclose(rv3.cpu().double(), 0.1 * var + 0.9 * rv0.cpu().double(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("use_graph", [True, False])
def test_sync_batchnorm_in_one_process_changes_nothing(use_graph):
    from dynamorph_amd.train import FusedTrainer
    xs, _ = _samples((4,))
    x = xs[0].cuda()
    out = []
    for flag in (False, True):
        tr = FusedTrainer(_model("VQ_VAE"), lr=1e-3, use_graph=use_graph, sync_batchnorm=flag)
        assert not tr.sync_bn
        vals = [tr.step(x).cpu() for _ in range(2)]
        out.append((vals, tr.flat.cpu(), _buffers(tr.model)))
    (v0, f0, b0), (v1, f1, b1) = out
    assert all(torch.equal(a, b) for a, b in zip(v0, v1))
    assert torch.equal(f0, f1)
    assert all(torch.equal(b0[k], b1[k]) for k in b0)
