import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    """GPU tests are skipped (not failed) when no device is visible, e.g. `pytest tests/` here."""
    import torch
    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU visible")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name)) as f:
        return {k: f[k] for k in f.files}


# (biases of convolutions that feed a train-mode BatchNorm have an identically zero gradient: rounding noise there becomes
# +-lr Adam steps whose signs depend on the summation order; they do not reach any output)
NOISE = ("enc.1.bias", "enc.4.bias", "enc.7.bias", "enc.10.bias", ".1.bias", ".4.bias")
# (... except the running mean of the BatchNorm behind them, which tracks the mean of conv + bias)
NOISE_MEAN = ("enc.2.running_mean", "enc.5.running_mean", "enc.8.running_mean", "enc.11.running_mean", ".2.running_mean",
              ".5.running_mean")

GOLDEN_THREADS = 8      # tests/golden/make_golden*.py: torch.set_num_threads(8)


@pytest.fixture
def golden_threads():
    """The CPU oracle with the thread count the golden vectors were captured with: oneDNN splits fp32 reductions (weight
    gradients, BatchNorm statistics) by thread, so another count sums in another order and the bit-for-bit / 1e-5
    comparisons against the vectors would measure the host instead of the oracle."""
    import torch
    saved = torch.get_num_threads()
    torch.set_num_threads(GOLDEN_THREADS)
    yield
    torch.set_num_threads(saved)


@pytest.fixture(scope="session")
def golden():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = load_golden(name)
        return cache[name]
    return get


def codes_gate(flips, z_ref, codebook, what="codes", rel=1e-4):
    """The end-to-end index gate of DESIGN.md section 3: the HIP encoder accumulates in another order than oneDNN, so a
    code may differ from the reference's ONLY where the reference's own two best distances are within `rel` of each other.
    flips: bool (B, H, W), True where the code (or the quantised vector) differs; z_ref: the REFERENCE latents
    (B, D, H, W); codebook (K, D).  Asserts zero flips away from such near-ties and at most 1e-5 * P + 1 flips in all;
    prints the counts."""
    import torch
    flips = torch.as_tensor(flips).bool().cpu()
    z_ref, codebook = torch.as_tensor(z_ref).double().cpu(), torch.as_tensor(codebook).double().cpu()
    B, D, H, W = z_ref.shape
    d = torch.cdist(z_ref.permute(0, 2, 3, 1).reshape(-1, D), codebook).pow(2)            # (P, K)
    top2 = torch.topk(d, 2, dim=1, largest=False).values
    near = ((top2[:, 1] - top2[:, 0]) <= rel * top2[:, 0]).reshape(B, H, W)
    nflip, nnear, P = int(flips.sum()), int(near.sum()), flips.numel()
    print(f"{what}: {nflip} of {P} codes differ, {nnear} reference near-ties (relative gap <= {rel})")
    assert not bool((flips & ~near).any()), f"{what}: {int((flips & ~near).sum())} codes differ away from near-ties"
    assert nflip <= 1e-5 * P + 1, f"{what}: {nflip} flips in {P} positions"


def oracle_truth(ref, x, **kw):
    """Runs the fp32 oracle `ref` AND a float64 copy of it on the same input (forward + backward of total_loss).
    Returns (loss dict of the fp32 run, {name: fp32 grad}, {name: float64 grad}).  The float64 run is the yardstick of
    grad_gate: what the fp32 reference itself misses it by is the accumulation noise no fp32 implementation can undercut."""
    import copy
    import torch
    ref64 = copy.deepcopy(ref).double()
    _, ld = ref(x, **kw)
    ld["total_loss"].backward()
    kw64 = {k: (v.double() if torch.is_tensor(v) else v) for k, v in kw.items()}
    _, ld64 = ref64(x.double(), **kw64)
    ld64["total_loss"].backward()
    g32 = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    g64 = {k: p.grad for k, p in ref64.named_parameters() if p.grad is not None}
    return ld, g32, g64


def grad_gate(model, g32, g64, keys=None, skip=(), factor=1.5, floor=2e-4, what="", factor_for=None, enforce=True):
    """Every gradient of the HIP `model` (p.grad) is as close to the float64 truth as the reference's own fp32 CPU path is
    (x factor), or within floor x the tensor's scale -- the yardstick of test_oracle_parity_fresh_seed_larger_batch, in
    place of the flat 2 % of scale the shape sweeps used until round 2 (a dropped tile row or a missing tap at B = 2..7
    hid under that).  factor_for: {tensor name: its own factor} for documented outliers; enforce=False only prints the table
    of ratios (hip error / reference fp32 error), for comparisons that are recorded but not gated."""
    worst = ("", 0.0)
    checked = 0
    ratios = []
    for k, p in model.named_parameters():
        if not p.requires_grad or k in skip or (keys is not None and k not in keys) or k not in g64:
            continue
        assert p.grad is not None, k
        truth = g64[k]
        scale = max(truth.abs().max().item(), 1e-6)
        e_ref = (g32[k].double() - truth).abs().max().item()
        e_hip = (p.grad.detach().cpu().double() - truth).abs().max().item()
        f = (factor_for or {}).get(k, factor)
        ratios.append((e_hip / max(e_ref, 1e-30), k, e_hip, e_ref, scale))
        if enforce:
            assert e_hip <= max(f * e_ref, floor * scale) + 1e-9, (what, k, "hip", e_hip, "fp32 reference", e_ref, "scale", scale)
        checked += 1
        if e_hip / scale > worst[1]:
            worst = (k, e_hip / scale)
    assert checked > 0
    if not enforce:
        print(f"{what} (recorded, not gated): hip error / reference fp32 error per tensor, largest first")
        for r, k, eh, er, sc in sorted(ratios, reverse=True)[:12]:
            print(f"    {k:32s} ratio {r:8.2f}   hip {eh:.2e}  reference {er:.2e}  scale {sc:.2e}")
        return checked
    top = max(ratios)
    print(f"{what}: {checked} gradients within the float64 yardstick; worst {worst[0]} {worst[1]:.2e} of scale; "
          f"largest hip / reference error ratio {top[0]:.2f} ({top[1]})")
    return checked


LOSS_GATE_WORST = {}


def loss_gate(got, ref, what, tol=1e-5):
    """north_star: recon / commitment loss within 1e-5 (fp32) of the reference.  |got - ref| <= tol * max(1, |ref|); the
    measured error of every call is kept (printed with -s, worst per label in LOSS_GATE_WORST) so that a gate can be read
    against what the kernels actually deliver."""
    got, ref = float(got), float(ref)
    err = abs(got - ref) / max(1.0, abs(ref))
    LOSS_GATE_WORST[what] = max(LOSS_GATE_WORST.get(what, 0.0), err)
    print(f"loss gate {what}: {got:.8f} vs {ref:.8f}, error {err:.2e} of max(1, |ref|)")
    assert err <= tol, (what, got, ref, err)
