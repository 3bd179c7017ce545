"""engine.view_strides -- (sn, sc, sky, skx, off) of a weight view from the weight's shape and the order of its two channel
dimensions -- against the tuples written out by hand for every weight shape of the two model families' example widths.  No
GPU and no library: the function is pure."""
import pytest

from dynamorph_amd.engine import view_strides

# shape (A, Bc, k, k) -> (stored: the output index is dim 0, swapped: the output index is dim 1; 3x3 taps flipped there)
EXPECTED = {
    (8, 3, 4, 4): ((48, 16, 4, 1, 0), (16, 48, 4, 1, 0)),               # the composite enc.0 o enc.1 weight at NIN = 2
    (16, 8, 4, 4): ((128, 16, 4, 1, 0), (16, 128, 4, 1, 0)),
    (16, 16, 4, 4): ((256, 16, 4, 1, 0), (16, 256, 4, 1, 0)),
    (16, 16, 3, 3): ((144, 9, 3, 1, 0), (9, 144, -3, -1, 8)),
    (32, 16, 3, 3): ((144, 9, 3, 1, 0), (9, 144, -3, -1, 8)),
    (16, 32, 1, 1): ((32, 1, 0, 0, 0), (1, 32, 0, 0, 0)),
    (2, 4, 1, 1): ((4, 1, 0, 0, 0), (1, 4, 0, 0, 0)),
    (64, 32, 4, 4): ((512, 16, 4, 1, 0), (16, 512, 4, 1, 0)),           # the wide family
    (64, 64, 3, 3): ((576, 9, 3, 1, 0), (9, 576, -3, -1, 8)),
}


@pytest.mark.parametrize("shape", sorted(EXPECTED))
def test_view_strides_are_the_literal_tuples(shape):
    stored, swapped = EXPECTED[shape]
    assert view_strides(shape, False) == stored
    assert view_strides(shape, True) == swapped


@pytest.mark.parametrize("shape", sorted(EXPECTED))
def test_views_address_the_weight_and_its_transpose(shape):
    """What the strides mean: element (n, c, ky, kx) of the view is w[n, c, ky, kx] in the stored order and, in the swapped
    order, w[c, n, ky, kx] -- for 3x3 with both tap axes reversed; every address stays inside the tensor."""
    import torch
    w = torch.arange(shape[0] * shape[1] * shape[2] * shape[3]).reshape(shape)
    flat, k = w.reshape(-1), shape[2]
    for swapped in (False, True):
        sn, sc, sky, skx, off = view_strides(shape, swapped)
        want = w.transpose(0, 1) if swapped else w
        if swapped and k == 3:
            want = want.flip(2, 3)
        n, c, ky, kx = torch.meshgrid(*[torch.arange(s) for s in want.shape], indexing="ij")
        addr = off + n * sn + c * sc + ky * sky + kx * skx
        assert int(addr.min()) >= 0 and int(addr.max()) < flat.numel()
        assert torch.equal(flat[addr], want)
