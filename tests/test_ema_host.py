"""`not gpu`: the EMA codebook mode's definition (tests/helpers/ema_reference.py) against an independent Lloyd step, and
the module surface -- keywords, parameters, buffers, state-dict keys, loading a reference-format checkpoint -- on the CPU
(constructing the modules needs no device; nothing here computes with them)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ema_reference as R  # noqa: E402

K, D = 12, 5


def _case(seed=0, used=8):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((3, D, 4, 4))
    idx = rng.integers(0, used, size=(3, 4, 4))          # codes used .. K - 1 are never assigned
    e = rng.standard_normal((K, D))
    return z, idx, e


def test_decay_zero_is_one_lloyd_step():
    """gamma = 0, epsilon = 0: N = n, m = s, sum N = P, so a used code becomes the mean of its assigned z."""
    z, idx, e = _case()
    n, s, N2, m2, e2 = R.ema_update_f64(z, idx, np.ones(K), e.copy(), e, 0.0, 0.0)
    zf = np.transpose(z, (0, 2, 3, 1)).reshape(-1, D)
    cnt = np.zeros(K)
    tot = np.zeros((K, D))
    np.add.at(cnt, idx.reshape(-1), 1.0)
    np.add.at(tot, idx.reshape(-1), zf)
    assert np.array_equal(n, cnt) and np.array_equal(N2, cnt)
    used = cnt > 0
    assert used.sum() >= 2 and (~used).sum() >= 4
    mean = tot[used] / cnt[used, None]
    # (n / P * P may differ from n in the last bit, and the one-hot product sums in another order than np.add.at)
    assert np.allclose(e2[used], mean, rtol=1e-13, atol=0)
    assert np.allclose(s, tot, rtol=1e-13, atol=1e-15)


def test_unused_code_keeps_its_vector():
    """gamma > 0, epsilon = 0: for a code that is never used N and m shrink by the same factor."""
    z, idx, e = _case(1)
    for decay in (0.5, 0.99):
        n, s, N2, m2, e2 = R.ema_update_f64(z, idx, np.ones(K), e.copy(), e, decay, 0.0)
        unused = n == 0
        assert unused.sum() >= 4
        assert np.allclose(e2[unused], e[unused], rtol=1e-14, atol=0)
        assert np.array_equal(N2[unused], np.full(unused.sum(), decay))


@pytest.mark.parametrize("k", [64, 49, 1000])
def test_initial_state_reproduces_the_codebook(k):
    """N = 1, m = e: e = m / N~ holds -- for epsilon = 0 to the last bit of the fp32 codebook (N~ = 1 / K * K is within an ulp
    of 1 in double, far below half an fp32 ulp); for epsilon > 0 N~ is still 1 up to rounding."""
    e = torch.randn(k, 7, generator=torch.Generator().manual_seed(k)).numpy()
    N, m = np.ones(k), e.astype(np.float64)
    for eps in (0.0, 1e-5):
        tot = N.sum()
        Nt = (N + eps) / (tot + k * eps) * tot              # steps 4 and 5 of the definition on the initial state
        got = (m / Nt[:, None]).astype(np.float32)
        if eps == 0.0:
            assert np.array_equal(got, e)
        else:
            assert np.allclose(got, e, rtol=2e-7, atol=0)


def _keys(m):
    return list(m.state_dict().keys())


@pytest.mark.parametrize("name", ["VQ_VAE", "VQ_VAE_z16", "VQ_VAE_z32"])
def test_state_dict_keys_with_and_without_the_mode(name):
    import dynamorph_amd
    cls = getattr(dynamorph_amd, name)
    plain, off, on = cls(), cls(ema_decay=None), cls(ema_decay=0.99, ema_epsilon=1e-5)
    # ema_decay=None is today's module: the same parameters, buffers and keys, in the same order
    assert _keys(off) == _keys(plain)
    assert [k for k, _ in off.named_parameters()] == [k for k, _ in plain.named_parameters()]
    assert [k for k, _ in off.named_buffers()] == [k for k, _ in plain.named_buffers()]
    assert [p.requires_grad for p in off.parameters()] == [p.requires_grad for p in plain.parameters()]
    assert "vq.ema_w" not in _keys(off) and not off.vq.ema
    # the mode adds the two buffers and nothing else; the codebook keeps its name and is frozen
    assert sorted(set(_keys(on)) - set(_keys(plain))) == ["vq.ema_cluster_size", "vq.ema_w"]
    assert [k for k in _keys(on) if not k.startswith("vq.ema_")] == _keys(plain)
    assert on.vq.ema and on.vq.ema_decay == 0.99 and on.vq.ema_epsilon == 1e-5
    assert "vq.w.weight" in dict(on.named_parameters()) and not on.vq.w.weight.requires_grad
    assert plain.vq.w.weight.requires_grad
    assert torch.equal(on.vq.ema_cluster_size, torch.ones(on.vq.num_embeddings))
    assert torch.equal(on.vq.ema_w, on.vq.w.weight.detach())
    # trainable elements: K * D fewer
    count = lambda m: sum(p.numel() for p in m.parameters() if p.requires_grad)   # noqa: E731
    assert count(plain) - count(on) == on.vq.w.weight.numel()


def test_quantizer_keywords_are_checked():
    from dynamorph_amd.vq_vae import VectorQuantizer
    q = VectorQuantizer(8, 16, ema_decay=0.0)
    assert q.ema and sorted(k for k, _ in q.named_buffers()) == ["ema_cluster_size", "ema_w"]
    assert not VectorQuantizer(8, 16).ema and list(VectorQuantizer(8, 16).named_buffers()) == []
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            VectorQuantizer(8, 16, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_epsilon"):
        VectorQuantizer(8, 16, ema_decay=0.9, ema_epsilon=-1.0)


@pytest.mark.parametrize("name", ["VQ_VAE", "VQ_VAE_z32"])
def test_reference_format_checkpoint_loads_into_an_ema_model(name):
    """A checkpoint without the two buffers: load_state_dict (strict) succeeds and the buffers take the initial state of the
    LOADED codebook; a checkpoint with them is loaded as it is."""
    import dynamorph_amd
    from oracle import vqvae_oracle as O
    torch.manual_seed(3)
    ref = O.OracleVQVAEz32() if name == "VQ_VAE_z32" else O.OracleVQVAE()
    sd = ref.state_dict()
    assert "vq.ema_w" not in sd
    m = getattr(dynamorph_amd, name)(ema_decay=0.9)
    m.vq.ema_cluster_size.fill_(7.0)                       # (stale state that the load must replace)
    res = m.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.vq.w.weight.detach(), sd["vq.w.weight"]) and not m.vq.w.weight.requires_grad
    assert torch.equal(m.vq.ema_w, sd["vq.w.weight"]) and torch.equal(m.vq.ema_cluster_size, torch.ones(64))
    assert "vq.ema_w" not in sd                            # the caller's mapping is left alone
    full = m.state_dict()
    full["vq.ema_cluster_size"] = torch.full((64,), 2.5)
    full["vq.ema_w"] = full["vq.ema_w"] * 2.5
    m2 = getattr(dynamorph_amd, name)(ema_decay=0.9)
    m2.load_state_dict(full)
    assert torch.equal(m2.vq.ema_cluster_size, torch.full((64,), 2.5)) and torch.equal(m2.vq.ema_w, full["vq.ema_w"])
    # and an EMA checkpoint does not load into a gradient-trained model by accident
    with pytest.raises(RuntimeError, match="ema_"):
        getattr(dynamorph_amd, name)().load_state_dict(full)


def test_routes_that_do_not_take_the_mode_say_so(monkeypatch):
    """fused='graph', and the autograd route with more than one rank, refuse an EMA model before anything touches a device."""
    import dynamorph_amd
    from dynamorph_amd import dist as D
    from dynamorph_amd.train import GraphedTrainer, _make_optimizer
    m = dynamorph_amd.VQ_VAE(ema_decay=0.9)
    with pytest.raises(ValueError, match="EMA"):
        _make_optimizer(m, 1e-3, "graph")
    with pytest.raises(ValueError, match="EMA"):
        GraphedTrainer(m)
    assert isinstance(_make_optimizer(m, 1e-3, False), torch.optim.Adam)      # one process: the eager autograd route
    monkeypatch.setattr(D, "world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="EMA codebook update with more than one rank"):
        _make_optimizer(m, 1e-3, False)


def test_oracle_wrapper_matches_the_float64_restatement():
    """OracleEMA (torch, model dtype) and the numpy restatement agree on one step of the float64 oracle; the codebook gets no
    gradient and the loss is cc * mse."""
    ref, x = R.build_oracle("VQ_VAE", R.ONE_STEP_SEEDS["VQ_VAE"])
    o = R.OracleEMA(ref, 0.9, 1e-5).double()
    e0, N0, m0 = o.codebook.clone().numpy(), o.N.numpy().copy(), o.m.numpy().copy()
    losses, z, idx = o.train_step(None, x.double())
    assert o.model.vq.w.weight.grad is None
    q = e0[idx.numpy()].transpose(0, 3, 1, 2)
    assert abs(float(losses["commitment_loss"]) - 0.25 * np.mean((q - z.numpy()) ** 2)) < 1e-14
    n, s, N2, m2, e2 = R.ema_update_f64(z.numpy(), idx.numpy(), N0, m0, e0, 0.9, 1e-5)
    assert n.sum() == idx.numel()
    assert np.allclose(o.N.numpy(), N2, rtol=1e-13) and np.allclose(o.m.numpy(), m2, rtol=1e-12, atol=1e-14)
    assert np.allclose(o.codebook.numpy(), e2, rtol=1e-12, atol=1e-14)


def test_committed_seeds_are_clean():
    """The one-step test's seeds satisfy the criterion they were chosen by (fp32 and float64 oracle codes equal, no near-tie
    at rel = 1e-4)."""
    for name, seed in R.ONE_STEP_SEEDS.items():
        assert R.seed_is_clean(name, seed), (name, seed)
