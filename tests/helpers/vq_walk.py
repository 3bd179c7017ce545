"""The quantiser's forward kernels where a workgroup walks several rounds of positions: one table of cases and the pure
functions the host test (tests/test_vq_walk_host.py) and the GPU test (tests/test_gpu_vq_walk.py) share.

vq_forward_mfma_kernel and vq_cells_kernel (csrc/vq.hip, csrc/vq_cells.h) are persistent: a workgroup takes 4 chunks of 64
positions (the cell kernel: 4 passes of 128) per round and comes back for more, `grid` workgroups further on.  The next
round's latents are requested during the current one, the (sample, chunk) cursor advances with one carry, the streamed
codebook's two LDS buffers keep their parity from round to round, the cell kernel's operand ring and group minima live on
from pass to pass.  Every case below makes the grid walk between two and three rounds; dm_vq_forward_plan -- the function
the launch sizes its grid with -- says so, and both tests assert it (conditions()).

Latent grids are 8 x 24 unless a case needs another: 192 positions = 3 chunks per sample, so the cursor's carry fires, and
192 % 128 != 0 keeps embedding_dim 16 on the streamed kernel.  Batch sizes follow from the grids the launch uses:
  streamed, embedding_dim 8 / 16   768 workgroups, 196608 positions per round      B = 2459 (P / 64 = 7377 = 4 * 1844 + 1)
  streamed, embedding_dim 32       512 workgroups, 131072                          B = 1639
  streamed, embedding_dim 64       256 (at most 64 codes) / 512 workgroups         B = 819 / 1639
  cell kernel                      512 workgroups of 4 waves, 262144               4096 < passes < 6144
"""
import collections
import ctypes

DM_VQ_AUTO, DM_VQ_EXACT, DM_VQ_MFMA, DM_VQ_BF16 = range(4)
KERNEL_EXACT, KERNEL_ANY, KERNEL_MFMA, KERNEL_CELLS = range(4)          # dm_vq_forward_plan's `kind`

SLICE_POSITIONS = 65536     # a batch slice of at most this many positions is ONE round on every route (asserted per case)

Case = collections.namedtuple("Case", "section filt D K H W B")
# section: "streamed" (vq_forward_mfma_kernel), "cells" (vq_cells_kernel), "join" (dm_vq_forward_join)
# filt: "auto" = DM_VQ_AUTO (the bf16-split filter wherever embedding_dim is a multiple of 16), "f32" = DM_VQ_MFMA


def _streamed():
    out = []
    for filt in ("auto", "f32"):
        # one-launch form; codebook that stays in the two LDS buffers (f32 filter); odd / even buffer count per round
        out += [Case("streamed", filt, 16, K, 8, 24, 2459) for K in (40, 300, 1100, 1500)]
        # 600 / 700 codes: odd / even buffer counts, the other way round for the other filter
        out += [Case("streamed", filt, 32, K, 8, 24, 1639) for K in (40, 100, 600, 700)]
        out += [Case("streamed", filt, 64, 64, 8, 24, 819)]
        out += [Case("streamed", filt, 64, K, 8, 24, 1639) for K in (128, 512, 576)]
        # the example configuration (VQ_VAE_z32: 512 codes x 64 dimensions, 32 x 32 latents)
        out += [Case("streamed", filt, 64, 512, 32, 32, 300)]
    out += [Case("streamed", "f32", 8, K, 8, 24, 2459) for K in (40, 300, 1100)]      # (no bf16 split at embedding_dim 8)
    # one chunk per sample (8 x 8 latents): the cursor's carry fires every round
    out += [Case("streamed", "f32", 8, 300, 8, 8, 7001), Case("streamed", "auto", 16, 1100, 8, 8, 7001),
            Case("streamed", "auto", 32, 600, 8, 8, 4801), Case("streamed", "auto", 64, 512, 8, 8, 4801)]
    return out


# The cell kernel's grid is capped at 512 workgroups (2048 waves), and its start-up stagger is on exactly when every wave
# has two full rounds (passes >= 8 * grid): no launch walks more than two rounds with the stagger off, so all three cases
# have it on.  130 codes: 4097 passes, the third round is ONE wave's; 777 codes: 5001 passes; 4096 codes on 32 x 32 latents
# (the 256-pixel workload's shape): 4168 passes.
CASES = _streamed() + [Case("cells", "auto", 16, 130, 8, 16, 4097), Case("cells", "auto", 16, 777, 16, 24, 1667),
                       Case("cells", "auto", 16, 4096, 32, 32, 521),
                       Case("join", "auto", 16, 64, 16, 16, 1850)]


def case_id(c):
    return f"{c.section}-{c.filt}-D{c.D}-K{c.K}-{c.H}x{c.W}-B{c.B}"


def variant(c):
    return DM_VQ_MFMA if c.filt == "f32" else DM_VQ_AUTO


def positions(c, B=None):
    return (c.B if B is None else B) * c.H * c.W


def plan(lib, c, B=None):
    """(kind, grid, positions_per_round) of the case's launch (of a batch of B samples of it) from dm_vq_forward_plan."""
    kind, grid, ppr = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.dm_vq_forward_plan(variant(c), c.D, c.K, c.H, c.W, positions(c, B), 1 if c.section == "join" else 0,
                                ctypes.byref(kind), ctypes.byref(grid), ctypes.byref(ppr))
    assert rc == 0, (case_id(c), rc, lib.dm_last_error())
    return kind.value, grid.value, ppr.value


def conditions(c, kind, grid, ppr):
    """What makes a case a case: the named kernel, between two and three rounds of its grid, and -- for the cases of the
    streamed kernel on latents smaller than 32 x 32 -- a last group of four chunks that is not full."""
    P = positions(c)
    assert kind == (KERNEL_CELLS if c.section == "cells" else KERNEL_MFMA), (case_id(c), kind)
    assert ppr == (512 if kind == KERNEL_CELLS else 256) * grid, (case_id(c), grid, ppr)
    assert 2 * ppr < P < 3 * ppr, (case_id(c), P, ppr)
    if c.section == "streamed" and (c.H, c.W) != (32, 32):
        assert (P // 64) % 4 != 0, (case_id(c), P)


def slices(B, HW, limit=SLICE_POSITIONS):
    """Consecutive batch slices [b0, b1) of at most `limit` positions each, covering [0, B)."""
    per = max(1, limit // HW)
    return [(b0, min(B, b0 + per)) for b0 in range(0, B, per)]


def oracle_samples(c, ppr):
    """The samples held to the C oracle: the first, the one workgroup 0's second round starts in (round r covers positions
    [r * ppr, (r + 1) * ppr) in workgroup order), the last."""
    return sorted({0, ppr // (c.H * c.W), c.B - 1})


def stream_buffers(D, K, bf):
    """Buffers' worth of code chunks vq_forward_mfma_kernel streams per round of positions (its PCH / nhp arithmetic): the
    parity of the LDS buffer a round starts on flips from round to round when this is odd.  At most 2: the codebook is
    staged once and stays."""
    aq = 2 * (D // 16) if bf else (D // 4 + 3) // 4
    pch = max(1, 1024 // (4 * aq * 64))
    return -(-(-(-K // 64)) // pch)


def draw(c, B=None):
    """Seeded randn latents (B, D, H, W) and codebook (K, D), as tests/test_gpu_kernels.py draws them."""
    import torch
    B = c.B if B is None else B
    z = torch.randn(B, c.D, c.H, c.W, generator=torch.Generator().manual_seed(c.B + c.D + c.K))
    cb = torch.randn(c.K, c.D, generator=torch.Generator().manual_seed(c.K))
    return z, cb


def gather(cb, idx):
    """codebook[idx] as (B, D, H, W)."""
    return cb[idx].permute(0, 3, 1, 2)


def straight_through(z, cb, idx):
    """The straight-through value z + (codebook[idx] - z) in fp32 (vq_vae.py:76), two rounded operations."""
    return z + (gather(cb, idx) - z)


def squared_error(z, cb, idx):
    """sum (codebook[idx] - z)^2 in float64."""
    return float((gather(cb, idx).double() - z.double()).pow(2).sum())


def nearest_codes(z, cb):
    """argmin_k |z - e_k|^2 in float64, first minimum (host stand-in for the kernels' codes on well-separated data)."""
    import torch
    B, D, H, W = z.shape
    d = torch.cdist(z.double().permute(0, 2, 3, 1).reshape(-1, D), cb.double()).pow(2)
    return d.argmin(1).reshape(B, H, W)
