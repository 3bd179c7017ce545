"""train() / run_one_batch / get_mask / get_relation_tensor against what the REFERENCE's own functions did.

tests/golden/g11_train_loop.npz was written by tests/golden/make_golden_train_loop.py, which lifts get_relation_tensor,
get_mask, run_one_batch and train out of the reference's run_training.py (335-417, 455-551) and runs them with the
reference's models on the CPU.  Here dynamorph_amd.train.train has to walk the same sample ids, hand its model the same
augmented batches, masks and relation blocks (bit for bit), log the same scalars and leave numpy's generator where the
reference leaves it.  No restated loop: the checker is the fixture."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.usefixtures("golden_threads")

from conftest import NOISE, NOISE_MEAN
W = torch.arange(1, 2 * 128 * 128 + 1, dtype=torch.float64).reshape(1, 2, 128, 128) / (2 * 128 * 128)


def _run(g, tag):
    pre = tag + "/"
    return {k[len(pre):]: v for k, v in g.items() if k.startswith(pre)}


def _inputs(g):
    from scipy.sparse import csr_matrix
    data = torch.from_numpy(g["data_f16"].astype(np.float32))
    masks = torch.from_numpy(g["masks_i8"].astype(np.float32))
    rel = csr_matrix(g["relation_dense_i8"].astype(np.float64))
    return data, masks, rel


class _Rows:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, float(value), int(step)))


class _Probe:
    """Keeps, per step, what train() hands the step: ids, batch checksum (the fixture's), mask checksum, relation block;
    the first batch in full."""

    def __init__(self):
        self.ids, self.sums, self.msums, self.tms, self.first_x, self.masks = [], [], [], [], None, {}

    def __call__(self, phase, epoch, ids, x, kw):
        self.ids.append(np.asarray(ids, dtype=np.int64).copy())
        xc = x.detach().cpu()
        if self.first_x is None:
            self.first_x = xc.clone()
        self.sums.append((xc.double() * W).sum(dim=(1, 2, 3)).numpy())
        m, tm = kw.get("batch_mask"), kw.get("time_matching_mat")
        if m is not None:
            mc = m.detach().cpu()
            self.masks[len(self.ids) - 1] = mc.clone()
            self.msums.append((mc.double() * (W[:, :1] * 2)).sum(dim=(1, 2, 3)).numpy())
        if tm is not None:
            self.tms.append(tm.detach().cpu().numpy().reshape(-1))


def _train_like_the_fixture(r, g, model, device, tmp_path, **kw):
    from torch.utils.data import TensorDataset
    from dynamorph_amd.train import train
    data, masks, rel = _inputs(g)
    rows, probe, stats = _Rows(), _Probe(), {}
    np.random.seed(int(r["seed"]))
    train(model, TensorDataset(data), str(tmp_path), relation_mat=rel if int(r["use_rel"]) else None,
          mask=TensorDataset(masks) if int(r["use_mask"]) else None, n_epochs=int(r["n_epochs"]), lr=float(r["lr"]),
          batch_size=int(g["batch_size"]), device=device, shuffle_data=bool(r["shuffle"]),
          transform=True if int(r["transform"]) else None, val_split_ratio=float(r["val_split_ratio"]), patience=20,
          writer=rows, probe=probe, stats=stats, **kw)
    after = np.random.randint(0, 2 ** 31, size=4)
    # every step's loss dict in the order the steps ran: epoch by epoch, training batches then validation batches
    rows.steps = [d for e in range(len(stats["step_losses"]["train"])) for ph in ("train", "val")
                  for d in stats["step_losses"][ph][e]]
    return rows, probe, after


def _check_walk(r, probe, after):
    """Everything discrete: ids, batches, masks, relation blocks, generator position -- bit for bit."""
    assert [len(i) for i in probe.ids] == r["step_len"].tolist()
    assert np.array_equal(np.concatenate(probe.ids), r["step_ids"]), "sample ids per step"
    assert np.array_equal(np.concatenate(probe.sums), r["step_checksum"]), "(augmented) batches, every step"
    if "first_train_x_f16" in r:
        assert torch.equal(probe.first_x, torch.from_numpy(r["first_train_x_f16"].astype(np.float32)))
    if int(r["use_mask"]):
        assert np.array_equal(np.concatenate(probe.msums), r["step_mask_checksum"])
        for name in ("first_train", "first_val"):
            want = torch.from_numpy(r[name + "_mask_u8"].astype(np.float32))
            assert torch.equal(probe.masks[int(r[name + "_step"])], want), name
    if int(r["use_rel"]):
        assert np.array_equal(np.concatenate(probe.tms).astype(np.int8), r["step_tm"])
    assert np.array_equal(after, r["after"]), "numpy's generator is left where the reference leaves it"


def _check_rows(r, rows, tol, tol_perplexity=None, after_flip=1.0):
    """Every step's loss dict and every epoch scalar against the reference's: |got - ref| <= tol * max(1, |ref|) for the
    losses (north_star: 1e-5).  On the GPU two things are looser, both for the reason codes_gate states: the HIP encoder
    sums in another order than oneDNN, so a position whose two best codes are a near-tie may take the other code.
      * perplexity = exp(entropy of the code counts) moves by ~1e-3 of its value when ONE of a batch's 512-2048 positions
        does (tol_perplexity);
      * such a position changes one of the 512-2048 terms of that step's commitment / codebook gradient, so the weights of
        all LATER steps differ at lr / positions -- a discrete event no fp32 implementation can follow bit for bit.  Steps
        up to and including the first one whose perplexity departs from the reference's by more than 1e-5 keep `tol`; the
        steps and epoch scalars after it get after_flip * tol.  The step-0 row (identical weights) is always at `tol`."""
    tol_perplexity = tol if tol_perplexity is None else tol_perplexity
    keys = r["loss_keys"].tolist()
    assert len(rows.steps) == len(r["step_losses"])
    worst = {"step": 0.0, "epoch": 0.0, "perplexity": 0.0}
    flipped_at = None
    n_epochs = int(r["n_epochs"])
    per_epoch = len(rows.steps) // n_epochs
    for i, (mine, want) in enumerate(zip(rows.steps, r["step_losses"])):
        assert list(mine.keys()) == keys, (i, list(mine.keys()))              # the model's own key order (vq_vae.py:333-338)
        bound = tol if flipped_at is None else after_flip * tol
        for k, w_ in zip(keys, want):
            err = abs(float(mine[k]) - w_) / max(1.0, abs(w_))
            kind = "perplexity" if k == "perplexity" else "step"
            worst[kind] = max(worst[kind], err)
            assert err <= (tol_perplexity if k == "perplexity" else bound), ("step", i, k, float(mine[k]), w_, err, flipped_at)
            if k == "perplexity" and err > 1e-5 and flipped_at is None:
                flipped_at = i
    assert [t for t, _, _ in rows.rows] == r["rows_tag"].tolist()             # same scalars in the same order
    assert [e for _, _, e in rows.rows] == r["rows_epoch"].tolist()
    for (tag, v, e), want in zip(rows.rows, r["rows_value"]):
        err = abs(v - want) / max(1.0, abs(want))
        kind = "perplexity" if tag.endswith("perplexity") else "epoch"
        worst[kind] = max(worst[kind], err)
        clean = flipped_at is None or flipped_at >= (e + 1) * per_epoch       # no code had flipped by the end of this epoch
        assert err <= (tol_perplexity if kind == "perplexity" else (tol if clean else after_flip * tol)), (tag, e, v, want, err)
    print(f"{len(rows.steps)} steps, {len(rows.rows)} epoch scalars; worst error of max(1, |ref|): losses per step "
          f"{worst['step']:.2e}, per epoch {worst['epoch']:.2e}, perplexity {worst['perplexity']:.2e}; "
          f"first step with another code than the reference's: {flipped_at}")


def _check_states(r, model, ckpt_path, lr, steps, atol, adam_noise=0.0):
    """model.pt (the best epoch's state dict) and the final state dict against the reference's.  atol: every element of
    every tensor; adam_noise > 0 (GPU): Adam's first steps move an element by ~lr * sign(gradient), so the few elements
    whose gradient is smaller than its own rounding noise take the other sign in another summation order -- they may
    differ by up to 2.5 * lr * steps, but at most a fraction adam_noise of a tensor's elements may leave atol."""
    ck = torch.load(ckpt_path, map_location="cpu")
    final = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    worst_frac = 0.0
    for tag, sd in (("ckpt", ck), ("final", final)):
        want = {k[len(tag) + 1:]: v for k, v in r.items() if k.startswith(tag + "/")}
        assert list(sd.keys()) == list(want.keys())
        for k, v in sd.items():
            w_ = torch.from_numpy(np.asarray(want[k]))
            assert v.shape == w_.shape and v.dtype == w_.dtype, (tag, k)
            if k.endswith("num_batches_tracked"):
                assert torch.equal(v, w_), (tag, k)
                continue
            diff = (v - w_).abs()
            if k.endswith(NOISE + NOISE_MEAN) and "enc" in k:
                assert diff.max() <= 2.5 * lr * steps, (tag, k)
            elif adam_noise > 0 and "running" not in k:
                off = float((diff > atol).float().mean())
                worst_frac = max(worst_frac, off)
                assert diff.max() <= 2.5 * lr * steps and off <= max(adam_noise, 1.0 / diff.numel()), (tag, k, float(diff.max()), off)
            else:
                assert diff.max() <= atol, (tag, k, float(diff.max()))
    if adam_noise > 0:
        print(f"state dicts: at most {worst_frac:.2%} of a tensor's elements beyond {atol:g}")


def _train_steps(r):
    n_val = int(np.floor(float(r["val_split_ratio"]) * 24))
    return int(np.ceil((24 - n_val) / 8)) * int(r["n_epochs"])


# ------------------------------------------------------------------------------------------------ host functions
def test_get_mask_and_get_relation_tensor_against_the_reference(golden):
    """run_training.py:335-374: the blocks the reference's own functions handed its model at every step of run a."""
    from torch.utils.data import TensorDataset
    from dynamorph_amd.train import get_mask, get_relation_tensor
    g = golden("g11_train_loop.npz")
    r = _run(g, "a")
    _, masks, rel = _inputs(g)
    at, tms = 0, []
    for i, n in enumerate(r["step_len"].tolist()):
        ids = r["step_ids"][at:at + n].tolist()
        at += n
        tm = get_relation_tensor(rel, ids, device="cpu")
        assert tm.dtype == torch.float32 and tm.shape == (n, n)
        tms.append(tm.numpy().astype(np.int8).reshape(-1))
        m = get_mask(TensorDataset(masks), ids, device="cpu")
        assert m.shape == (n, 1, 128, 128) and m.dtype == torch.float32
        if i == int(r["first_train_step"]):
            assert torch.equal(m, torch.from_numpy(r["first_train_mask_u8"].astype(np.float32)))
            assert np.array_equal(tm.numpy(), r["first_train_tm"])
        if i == int(r["first_val_step"]):
            assert torch.equal(m, torch.from_numpy(r["first_val_mask_u8"].astype(np.float32)))
            assert np.array_equal(tm.numpy(), r["first_val_tm"])
    assert np.array_equal(np.concatenate(tms), r["step_tm"])
    assert get_relation_tensor(None, [0]) is None and get_mask(None, [0]) is None


def test_train_loop_on_the_cpu_walks_the_reference_batches(golden, tmp_path):
    """Run c (no augmentation: nothing needs the GPU) with the CPU oracle as the model: split, shuffles, ragged batches,
    masks, per-epoch scalars, checkpoint and generator position of the reference's train()."""
    from oracle import vqvae_oracle as O
    g = golden("g11_train_loop.npz")
    r = _run(g, "c")
    model = O.OracleVQVAE()
    model.load_state_dict({k[4:]: torch.from_numpy(np.asarray(v)) for k, v in r.items() if k.startswith("sd0/")})
    rows, probe, after = _train_like_the_fixture(r, g, model, "cpu", tmp_path, fused=False)
    _check_walk(r, probe, after)
    _check_rows(r, rows, tol=2e-6)
    _check_states(r, model, os.path.join(tmp_path, "model.pt"), float(r["lr"]), _train_steps(r), atol=2e-6)


# ------------------------------------------------------------------------------------------------ the HIP path
@pytest.mark.gpu
@pytest.mark.parametrize("tag,feed,fused", [("a", "resident", True), ("a", "sync", False), ("a", "stream", True),
                                            ("b", "resident", True), ("b", "sync", True), ("c", "resident", True)])
def test_train_loop_reproduces_the_reference_run(golden, tmp_path, tag, feed, fused):
    """dynamorph_amd.train.train on the GPU (resident feed + FusedTrainer = the product default; the streaming feed; the
    reference-shaped synchronous loop on the autograd path) against the reference's run: ids, augmented batches, masks
    and relation blocks bit for bit, every epoch scalar within 1e-5, weights after the run."""
    import dynamorph_amd
    g = golden("g11_train_loop.npz")
    r = _run(g, tag)
    cls = dynamorph_amd.VQ_VAE_z16 if tag == "a" else dynamorph_amd.VQ_VAE
    model = cls().to("cuda:0")
    model.load_state_dict({k[4:]: torch.from_numpy(np.asarray(v)) for k, v in r.items() if k.startswith("sd0/")})
    rows, probe, after = _train_like_the_fixture(r, g, model, "cuda:0", tmp_path, fused=fused, feed=feed)
    for i, (mine, want) in enumerate(zip(rows.steps, r["step_losses"])):
        print(f"step {i:2d} n={int(r['step_len'][i])}: " + "  ".join(f"{float(a):.7f}/{b:.7f}" for a, b in zip(mine.values(), want)))
    _check_walk(r, probe, after)
    _check_rows(r, rows, tol=1e-5, tol_perplexity=3e-3, after_flip=10.0)
    _check_states(r, model, os.path.join(tmp_path, "model.pt"), float(r["lr"]), _train_steps(r), atol=0.5 * float(r["lr"]), adam_noise=0.05)
