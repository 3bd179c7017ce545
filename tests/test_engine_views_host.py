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


# ------------------------------------------------------------------ the Layers objects of the two families (CPU modules)
def _resolves(L, m):
    """L holds the very modules of m (a VQ_VAE_z32), by the child indices of the reference's two nn.Sequentials."""
    enc, dec = m.enc, m.dec
    assert (L.conv0, L.bn0, L.conv1, L.bn1, L.enc_block) == (enc[0], enc[1], enc[3], enc[4], enc[5])
    assert L.conv0 is enc[0] and L.bn0 is enc[1] and L.conv1 is enc[3] and L.bn1 is enc[4] and L.enc_block is enc[5]
    assert L.dec_block is dec[0] and L.up0 is dec[1] and L.bn_up is dec[2] and L.up1 is dec[4]
    for handles, block in ((L.enc_res, enc[5]), (L.dec_res, dec[0])):
        assert len(handles) == len(block.layers) == 2
        for (ca, bna, cb, bnb), l in zip(handles, block.layers):
            assert ca is l[1] and bna is l[2] and cb is l[4] and bnb is l[5]
    assert L.codebook is m.vq.w and L.channel_var is m.channel_var and (L.nin, L.nh) == (2, 16)
    assert [id(p) for p in L.stem_params()] == [id(p) for i in (0, 1, 3, 4) for p in (enc[i].weight, enc[i].bias)]
    assert [id(p) for p in L.tail_params()] == [id(p) for i in (1, 2, 4) for p in (dec[i].weight, dec[i].bias)]


def test_z32_layers_hold_the_models_own_modules():
    import dynamorph_amd
    from dynamorph_amd.engine import Z32Layers
    m = dynamorph_amd.VQ_VAE_z32()
    _resolves(Z32Layers(m), m)
    Le, Ld = Z32Layers(enc=m.enc), Z32Layers(dec=m.dec)              # the halves on their own: no parent, no loss
    assert Le.conv1 is m.enc[3] and Le.enc_res[1][3] is m.enc[5].layers[1][5] and not hasattr(Le, "up0")
    assert Ld.up1 is m.dec[4] and Ld.dec_res[0][0] is m.dec[0].layers[0][1] and not hasattr(Ld, "conv0")
    assert Le.channel_var is None and Ld.channel_var is None and Le.codebook is None and Ld.codebook is None
    assert (Le.nin, Le.nh) == (Ld.nin, Ld.nh) == (2, 16)
    assert not any(v is m for L in (Z32Layers(m), Le, Ld) for v in vars(L).values())     # no back-reference to the parent


def test_z32_layers_resolve_on_a_copy_and_after_pickling():
    import copy
    import pickle
    import dynamorph_amd
    from dynamorph_amd.engine import Z32Layers
    m = dynamorph_amd.VQ_VAE_z32()
    for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        _resolves(Z32Layers(other), other)
        assert Z32Layers(other).conv0 is not m.enc[0]
        assert list(other.state_dict()) == list(m.state_dict())


def test_layers_of_names_the_family():
    import torch
    import dynamorph_amd
    from dynamorph_amd.engine import Layers, Z32Layers, layers_of
    for cls, want in ((dynamorph_amd.VQ_VAE, Layers), (dynamorph_amd.VQ_VAE_z16, Layers), (dynamorph_amd.VQ_VAE_z32, Z32Layers)):
        assert type(layers_of(cls(), "caller")) is want and type(layers_of(cls())) is want
    d, z = layers_of(dynamorph_amd.VQ_VAE(weight_recon=2.0, weight_commitment=0.5)), layers_of(dynamorph_amd.VQ_VAE_z32())
    assert (d.latent_stride, d.latent_after_vq, d.loss_weights) == (8, False, (2.0, 0.5))
    assert (z.latent_stride, z.latent_after_vq, z.loss_weights) == (4, True, (1.0, 1.0))
    with pytest.raises(TypeError, match=r"caller: Linear is not built on the HIP path \(VQ_VAE, VQ_VAE_z16, VQ_VAE_z32\)"):
        layers_of(torch.nn.Linear(2, 2), "caller")
    assert layers_of(torch.nn.Linear(2, 2)) is None
