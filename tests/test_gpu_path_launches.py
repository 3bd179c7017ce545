"""The launch sequence of the package's PUBLIC paths, pinned: `model(x, ...)` + `.backward()`, one eager FusedTrainer step,
encode_patches / score_patches / patch_gradients -- every C entry point of libdynamorph_hip.so each reaches, in order, with
its plain-integer arguments (test_gpu_engine_launches.Recorder).  test_gpu_engine_launches.py pins dynamorph_amd.engine
function by function; this file pins what the callers of the engine assemble from it, so a caller rewritten against another
set of engine functions must still reach the same kernels on the same data in the same order.

tests/golden/g16_path_launches.json holds every distinct call once ("calls") and each case as the list of its calls' positions
in that table ("cases"); the lists are compared whole.  `python tests/test_gpu_path_launches.py` rewrites the file from the
code as it stands (on the GPU).
"""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_engine_launches import DEV, FUSED, WIDE, Recorder  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_path_launches.json")
B, N, SIZE = 2, 3, 128          # N = 3 with batch_size 2: a batch of 2 and one of 1; three patches are two power-of-two runs


def _model(family, seed=16, eval_mode=False, **kw):
    import torch
    import dynamorph_amd
    torch.manual_seed(seed)
    m = getattr(dynamorph_amd, family)(num_inputs=2, **kw).to(DEV)
    return m.eval() if eval_mode else m


def _batch(n=B, mask=False, matrix=False):
    import torch
    g = torch.Generator().manual_seed(61)
    x = torch.randn(n, 2, SIZE, SIZE, generator=g)
    m = (torch.rand(n, 1, SIZE, SIZE, generator=g) > 0.4).float() if mask else None
    tm = torch.randint(0, 3, (n, n), generator=g).float() if matrix else None
    return x, m, tm


def _to(t):
    return None if t is None else t.to(DEV)


# ------------------------------------------------------------------------------------ cases
def _autograd(family, mask=False, want_dx=False, **kw):
    m = _model(family, **kw)
    x, msk, tm = (_to(t) for t in _batch(mask=mask, matrix=True))
    if want_dx:
        x.requires_grad_()
    with Recorder() as calls:
        _, ld = m(x, time_matching_mat=tm, batch_mask=msk)
        ld["total_loss"].backward()
    return calls


def _halves():
    """model.enc(x) and model.dec(z) of VQ_VAE_z32 on their own, each with its backward."""
    import torch
    m = _model("VQ_VAE_z32")
    x = _to(_batch()[0])
    with Recorder() as calls:
        z = m.enc(x)
        z.backward(torch.ones_like(z))
        dec = m.dec(z.detach())
        dec.backward(torch.ones_like(dec))
    return calls


def _trainer(family, matrix=False, mask=False, forward_only=False, **kw):
    from dynamorph_amd.train import FusedTrainer
    m = _model(family, **kw)
    tr = FusedTrainer(m, use_graph=False)
    x, msk, tm = (_to(t) for t in _batch(mask=mask, matrix=matrix))
    with Recorder() as calls:
        if forward_only:
            tr.forward_only(x, msk, tm)
        else:
            tr.step(x, msk, tm)
    return calls


def _encode(family):
    from dynamorph_amd.patch_vae import encode_patches
    m = _model(family)
    with Recorder() as calls:
        encode_patches(m, _batch(N)[0], device=DEV, batch_size=2)
    return calls


def _score(family, eval_mode):
    from dynamorph_amd.patch_vae import score_patches
    m = _model(family, eval_mode=eval_mode)
    x, msk, _ = _batch(N, mask=True)
    with Recorder() as calls:
        score_patches(m, x, masks=msk, device=DEV, batch_size=2, return_decoded=True)
    return calls


def _gradients(family, of):
    import torch
    from dynamorph_amd.patch_vae import patch_gradients
    m = _model(family)
    x, msk, _ = _batch(N, mask=True)
    if of == "cotangent":        # (N, D*h*w): one cotangent on z_before per patch
        of = torch.randn(N, 16 * (SIZE // 4) ** 2, generator=torch.Generator().manual_seed(62))
    with Recorder() as calls:
        patch_gradients(m, x, masks=msk, of=of, device=DEV, batch_size=2)
    return calls


CASES = {
    # model(x, ...) followed by .backward(), B = 2
    "autograd-default": lambda: _autograd("VQ_VAE", mask=True, **FUSED),
    "autograd-z32": lambda: _autograd("VQ_VAE_z32"),
    "autograd-z32-wide": lambda: _autograd("VQ_VAE_z32", **WIDE),
    "autograd-z32-want_dx": lambda: _autograd("VQ_VAE_z32", mask=True, want_dx=True),
    "autograd-z32-enc_and_dec_alone": _halves,
    # FusedTrainer(model, use_graph=False): one step, or one forward_only
    "trainer-default": lambda: _trainer("VQ_VAE", matrix=True, mask=True, **FUSED),
    "trainer-default-forward_only": lambda: _trainer("VQ_VAE", matrix=True, forward_only=True, **FUSED),
    "trainer-z32": lambda: _trainer("VQ_VAE_z32"),
    "trainer-z32-matrix": lambda: _trainer("VQ_VAE_z32", matrix=True, mask=True),
    "trainer-z32-wide": lambda: _trainer("VQ_VAE_z32", **WIDE),
    "trainer-z32-wide-matrix": lambda: _trainer("VQ_VAE_z32", matrix=True, **WIDE),
    "trainer-z32-ema": lambda: _trainer("VQ_VAE_z32", ema_decay=0.99),
    "trainer-z32-forward_only": lambda: _trainer("VQ_VAE_z32", matrix=True, forward_only=True),
    # the inference drivers, N = 3 with batch_size 2
    "encode-z32": lambda: _encode("VQ_VAE_z32"),
    "score-default-train": lambda: _score("VQ_VAE", False),
    "score-default-eval": lambda: _score("VQ_VAE", True),
    "score-z32-train": lambda: _score("VQ_VAE_z32", False),
    "score-z32-eval": lambda: _score("VQ_VAE_z32", True),
    "gradients-default-total_loss": lambda: _gradients("VQ_VAE", "total_loss"),
    "gradients-default-recon_loss": lambda: _gradients("VQ_VAE", "recon_loss"),
    "gradients-default-commitment_loss": lambda: _gradients("VQ_VAE", "commitment_loss"),
    "gradients-z32-total_loss": lambda: _gradients("VQ_VAE_z32", "total_loss"),
    "gradients-z32-recon_loss": lambda: _gradients("VQ_VAE_z32", "recon_loss"),
    "gradients-z32-commitment_loss": lambda: _gradients("VQ_VAE_z32", "commitment_loss"),
    "gradients-z32-cotangent": lambda: _gradients("VQ_VAE_z32", "cotangent"),
}


def _run(case):
    import torch
    got = json.loads(json.dumps(CASES[case]()))
    torch.cuda.synchronize()
    return got


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {name: [g["calls"][i] for i in seq] for name, seq in g["cases"].items()}


def test_golden_covers_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_sequence_is_the_recorded_one(recorded, case):
    got, want = _run(case), recorded[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: call {i} is {g}, recorded {w}"
    assert len(got) == len(want), f"{case}: {len(got)} calls, recorded {len(want)}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    table, cases = {}, {}
    for name in sorted(CASES):
        keys = [json.dumps(c, separators=(",", ":")) for c in _run(name)]
        cases[name] = [table.setdefault(k, len(table)) for k in keys]
        print(f"{name}: {len(keys)} calls")
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        f.write('{"calls": [\n' + ",\n".join("  " + k for k in table) + '\n],\n"cases": {\n'
                + ",\n".join("  " + json.dumps(k) + ": " + json.dumps(v, separators=(",", ":")) for k, v in cases.items())
                + "\n}}\n")
