"""Reference side of dynamorph_amd.patch_vae.patch_gradients and of the per-patch backward of the 16 x 16 latent stage.

oracle_patch_gradients: the reference's batch-of-one loop on the CPU oracle -- x = patches[i:i+1].requires_grad_();
model(x, batch_mask=masks[i:i+1])[1][of].backward(); x.grad -- in fp32 or float64, with the forward hooks of
tests/test_gpu_model.py::test_gradient_with_respect_to_the_input_patches counting the ReLU inputs that fp32 rounding can flip.
yardstick: that test's gate, per patch.  latent_stage_reference: enc.10 .. enc.12 as functional torch (batch_norm per patch),
differentiated by autograd -- nothing here calls the library.  Pure CPU; tests/test_patch_gradients_host.py holds the loop to
plain autograd on the oracle.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

FRAGILE_REL = 4e-7          # a ReLU input the float64 run decides by less than this x the tensor's largest value


def oracle_patch_gradients(ref, x, mask=None, of="total_loss", dtype=torch.float32, force_idx=None, count_fragile=False):
    """ref: an oracle model in the mode to evaluate (left untouched: the loop runs on a copy, cast to `dtype`).
    of: a key of the loss dict, or a cotangent on z_before -- (D*h*w,) shared or (N, D*h*w) -- for which the differentiated
    scalar is (of_i * enc(x_i).reshape(-1)).sum(), the encoder alone.
    force_idx: {patch index: codes (1, h, w)} the quantiser uses instead of its argmin for those patches.
    Returns (gradients (N, C, H, W) in `dtype`, per-patch count of fragile ReLU inputs (zeros unless count_fragile))."""
    model = copy.deepcopy(ref).to(dtype)
    N = x.shape[0]
    cot = None if isinstance(of, str) else torch.as_tensor(of).to(dtype)
    grads, fragile = [], np.zeros(N, np.int64)
    near = []
    hooks = []
    if count_fragile:
        hooks = [mod.register_forward_hook(lambda _m, a, _o: near.append(int((a[0].abs() < FRAGILE_REL * a[0].abs().max()).sum())))
                 for mod in model.modules() if isinstance(mod, torch.nn.ReLU)]
    for i in range(N):
        xi = x[i:i + 1].detach().clone().to(dtype).requires_grad_(True)
        del near[:]
        if cot is not None:
            w = cot if cot.dim() == 1 else cot[i]
            (w * model.enc(xi).reshape(-1)).sum().backward()
        else:
            model.vq.force_idx = None if force_idx is None or i not in force_idx else force_idx[i]
            m = None if mask is None else mask[i:i + 1].to(dtype)
            model(xi, batch_mask=m)[1][of].backward()
        fragile[i] = sum(near)
        grads.append(xi.grad)
    for h in hooks:
        h.remove()
    return torch.cat(grads, 0), fragile


def yardstick(got, g32, g64, fragile, what=""):
    """The gate of test_gradient_with_respect_to_the_input_patches on one patch (or one tensor): with e_ref the fp32 oracle's
    error against float64 and scale the float64 gradient's largest magnitude, every element within max(1.5 e_ref, 2e-4 scale)
    -- except around `fragile` ReLU inputs, where at most 8192 elements per fragile input may exceed it and none 5e-2 scale.
    Prints the figures, then asserts."""
    truth = torch.as_tensor(g64).double()
    got = torch.as_tensor(got).double()
    scale = truth.abs().max().item()
    e_ref = (torch.as_tensor(g32).double() - truth).abs().max().item()
    err = (got - truth).abs()
    e_hip = err.max().item()
    tight = max(1.5 * e_ref, 2e-4 * scale) + 1e-12
    off = int((err > tight).sum())
    print(f"{what}: scale {scale:.2e}, error {e_hip:.2e}, of the fp32 reference {e_ref:.2e}; {off} of {err.numel()} elements "
          f"beyond {tight:.1e}, {int(fragile)} fragile ReLU inputs")
    assert scale > 0 and off <= 8192 * fragile and e_hip <= (5e-2 * scale if fragile else tight), \
        (what, e_hip, e_ref, scale, off, int(fragile))


def latent_stage_reference(a3, gamma3, beta3, eps3, w10, b10, gamma4, beta4, eps4, res, g_z, dtype=torch.float64):
    """enc.8 (BatchNorm + ReLU on a3) .. enc.12 of every patch with that patch's own statistics, and its backward.
    a3, g_z (B, C, H, W); res: per residual layer (wa, ba, gamma_a, beta_a, eps_a, wb, bb, gamma_b, beta_b, eps_b).
    Returns (z, dy3, slab, fragile): dy3 = d<g_z, z> / d relu(BN3(a3)) masked by that ReLU, i.e. the gradient at enc.8's output before
    its BatchNorm backward; slab (B, C, 2) = (sum dy3, sum dy3 * a3) per patch; fragile (B,): the ReLU
    inputs of the patch within FRAGILE_REL of zero."""
    c = lambda t: None if t is None else torch.as_tensor(t).detach().to(dtype)       # noqa: E731
    B = a3.shape[0]
    zs, dys, slabs, fragile = [], [], [], []
    near = []

    def relu(t):
        near.append(int((t.abs() < FRAGILE_REL * t.abs().max()).sum()))
        return F.relu(t)
    for b in range(B):
        a = c(a3[b:b + 1])
        del near[:]
        y3 = F.batch_norm(a, None, None, c(gamma3), c(beta3), True, 0.0, eps3).requires_grad_(True)
        h = F.conv2d(relu(y3), c(w10), c(b10), padding=1)
        h = F.batch_norm(h, None, None, c(gamma4), c(beta4), True, 0.0, eps4)
        for wa, ba, ga, bea, epsa, wb, bb, gb, beb, epsb in res:
            r = F.batch_norm(F.conv2d(relu(h), c(wa), c(ba), padding=1), None, None, c(ga), c(bea), True, 0.0, epsa)
            wb_ = c(wb)
            r = F.batch_norm(F.conv2d(relu(r), wb_.reshape(wb_.shape[0], -1, 1, 1), c(bb)), None, None, c(gb), c(beb), True, 0.0, epsb)
            h = h + r
        (h * c(g_z[b:b + 1])).sum().backward()
        dy = y3.grad
        zs.append(h.detach())
        dys.append(dy)
        slabs.append(torch.stack([dy.sum((0, 2, 3)), (dy * a).sum((0, 2, 3))], 1))
        fragile.append(sum(near))
    return torch.cat(zs, 0), torch.cat(dys, 0), torch.stack(slabs, 0), np.asarray(fragile)
