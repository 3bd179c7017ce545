"""The launch sequence of dynamorph_amd.engine, pinned: every C entry point of libdynamorph_hip.so that a call reaches, in
order, with its plain-integer arguments (the integer fields of the structs it is handed included: load modes, weight-view
strides and offsets, segment shapes of the slab reduction) -- no pointers, no floats.  The recorded lists of
tests/golden/g15_engine_launches.json are compared whole, so a launch that is added, dropped, reordered, routed to another
kernel or given another weight view fails here whatever the numbers come out as.

`python tests/test_gpu_engine_launches.py` rewrites the golden file from the code as it stands (on the GPU).
"""
import ctypes as C
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_engine_launches.json")


# --------------------------------------------------------------------------------- recorder
def _is_int(t):
    return isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ in "bBhHiIlLqQ"


def _ints(v):
    """The plain-integer content of a ctypes struct (a dict, nested structs and arrays included) or array (a list)."""
    if isinstance(v, C.Structure):
        out = {}
        for name, t in v._fields_:
            if _is_int(t):
                out[name] = int(getattr(v, name))
            elif issubclass(t, (C.Structure, C.Array)):
                sub = _ints(getattr(v, name))
                if sub and any(sub):
                    out[name] = sub
        return out
    if _is_int(v._type_):
        return [int(e) for e in v]
    if issubclass(v._type_, (C.Structure, C.Array)):
        return [_ints(e) for e in v]
    return None


class Recorder:
    """with Recorder() as calls: the bound entry points of _lib.load() are wrapped for the duration of the block."""

    def __enter__(self):
        from dynamorph_amd import _lib
        self.lib, self.saved, calls = _lib.load(), {}, []
        for name, (_, argtypes) in _lib.SIGNATURES.items():
            self.saved[name] = fn = getattr(self.lib, name)
            setattr(self.lib, name, self._wrap(name, fn, argtypes, calls))
        return calls

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)

    @staticmethod
    def _wrap(name, fn, argtypes, calls):
        def call(*args):
            rec = []
            for a, t in zip(args, argtypes):
                if _is_int(t):
                    rec.append(int(a))
                elif hasattr(t, "_type_") and isinstance(t._type_, type) and issubclass(t._type_, C.Structure):
                    rec.append(None if a is None else _ints(getattr(a, "_obj", a)))      # byref(struct) or an array of them
            calls.append([name, rec])
            return fn(*args)
        return call


# ------------------------------------------------------------------------------------ cases
class Grads(dict):
    """G(param) -> the tensor a backward kernel writes that parameter's gradient into."""

    def __call__(self, p):
        if id(p) not in self:
            import torch
            self[id(p)] = torch.zeros_like(p)
        return self[id(p)]


def _vqvae(seed=5, B=2, size=128, eval_mode=False, **kw):
    import torch
    import dynamorph_amd
    from dynamorph_amd import engine as E
    torch.manual_seed(seed)
    m = dynamorph_amd.VQ_VAE(num_inputs=2, **kw).to(DEV)
    if eval_mode:
        m.eval()
    x = torch.randn(B, 2, size, size, device=DEV)
    return m, E.Layers(m), x


FUSED = dict(num_hiddens=16, num_residual_hiddens=32, num_residual_layers=2)      # 16 x 16 latents: every fused backward
NARROW = dict(num_hiddens=8, num_residual_hiddens=32, num_residual_layers=2)      # no fused kernel is built for this width


def _encoder(kw, size, want_dx=False, zero_fed_biases=True, defer_last_join=0, eval_mode=False):
    import torch
    from dynamorph_amd import engine as E
    m, L, x = _vqvae(size=size, eval_mode=eval_mode, **kw)
    with Recorder() as calls:
        z, cx = E.encoder_forward(L, x, defer_last_join=defer_last_join)
        if defer_last_join:
            assert z is None and cx.pending_join is not None
            z, _, _, _ = E.vq_forward_joined(L.codebook.weight, cx.pending_join, 0.25)
        E.encoder_backward(L, cx, torch.randn_like(z), Grads(), zero_fed_biases=zero_fed_biases, want_dx=want_dx)
    return calls


def _decoder(kw, size, form, want_gz=True, own_pending=True):
    """form: 'deferred' (dec_tail_train), 'fused' (dec_tail_backward where built), 'ext' (gdec_ext beside the loss),
    'ext_only' (no loss term)."""
    import torch
    from dynamorph_amd import engine as E, ops
    m, L, x = _vqvae(size=size, **kw)
    zq = torch.randn(2, kw["num_hiddens"], size // 8, size // 8, device=DEV)
    gscale = torch.ones(1, device=DEV)
    with Recorder() as calls:
        dec, cx = E.decoder_forward(L, zq, x, None, defer_tail=form == "deferred")
        assert cx.deferred == (form == "deferred")
        gext = torch.randn_like(x) if form in ("ext", "ext_only") else None
        pending = None if own_pending else []
        E.decoder_backward(L, cx, None if form == "ext_only" else gscale, gext, Grads(), want_gz=want_gz, pending=pending)
        if pending is not None:
            ops.reduce_slabs_multi(pending)
    return calls


def _per_sample(latents_only):
    from dynamorph_amd import engine as E
    m, L, x = _vqvae(**FUSED)
    with Recorder() as calls:
        E.encoder_forward(L, x, per_sample=True, latents_only=latents_only)
    return calls


def _quantiser(form):
    import torch
    from dynamorph_amd import engine as E
    m, L, x = _vqvae(**FUSED)
    z = torch.randn(2, 16, 16, 16, device=DEV)
    kw = dict(plain={}, deferred=dict(defer_scalars=True), latents=dict(want_scalars=False))[form]
    with Recorder() as calls:
        E.vq_forward(L.codebook.weight, z, 0.25, **kw)
    return calls


def _z32(form, want_dx=False, want_gr=True, **kw):
    """The two conv stems of VQ_VAE_z32 around its residual stacks, as FusedTrainer and the autograd functions call them:
    form 'shared' -- one pending list and one slab reduction for the whole pass; 'own' -- every function reduces its own."""
    import torch
    import dynamorph_amd
    from dynamorph_amd import engine as E, ops
    torch.manual_seed(6)
    m = dynamorph_amd.VQ_VAE_z32(**kw).to(DEV)
    L = E.Z32Layers(m)
    x = torch.randn(2, 2, 128, 128, device=DEV)
    er, dr = L.enc_res, L.dec_res
    G = Grads()
    gscale = torch.ones(1, device=DEV)
    shared = form == "shared"
    with Recorder() as calls:
        h, scx = E.z32_stem_forward(L, x)
        z, esaved = E.residual_forward(er, h)
        r, dsaved = E.residual_forward(dr, z)
        _, cx = E.z32_tail_forward(L, r, x, None)
        pending = [] if shared else None
        gext = None if shared else torch.randn_like(x)
        g_r = E.z32_tail_backward(L, cx, gscale if want_gr else None, gext, G, want_gr=want_gr,
                                  pending=pending, zero_fed_biases=not shared)
        if want_gr:
            rp = pending if shared else []
            g_z, _ = E.residual_backward(dr, dsaved, g_r, G, None, pending=rp, zero_fed_biases=not shared)
            g_h, stats = E.residual_backward(er, esaved, g_z, G, scx.a2 if shared else None, pending=rp,
                                             zero_fed_biases=not shared)
            E.z32_stem_backward(L, scx, g_h, G, stats=stats, pending=pending,
                                zero_fed_biases=not shared, want_dx=want_dx)
            ops.reduce_slabs_multi(rp)
    return calls


WIDE = dict(num_hiddens=64, num_residual_hiddens=64, num_embeddings=512)           # the reference's config_example.yml

CASES = {
    # VQ_VAE at the reference's width, B = 2, 128 x 128
    "encoder": lambda: _encoder(FUSED, 128),
    "encoder-want_dx": lambda: _encoder(FUSED, 128, want_dx=True),
    "encoder-biases_not_zeroed": lambda: _encoder(FUSED, 128, zero_fed_biases=False),
    "encoder-want_dx-biases_not_zeroed": lambda: _encoder(FUSED, 128, want_dx=True, zero_fed_biases=False),
    "encoder-join_in_quantiser": lambda: _encoder(FUSED, 128, defer_last_join=64),
    "encoder-eval": lambda: _encoder(FUSED, 128, eval_mode=True),
    "decoder-deferred_tail": lambda: _decoder(FUSED, 128, "deferred"),
    "decoder-fused_tail": lambda: _decoder(FUSED, 128, "fused"),
    "decoder-gdec_ext": lambda: _decoder(FUSED, 128, "ext"),
    "decoder-gdec_ext_only": lambda: _decoder(FUSED, 128, "ext_only"),
    "decoder-no_gz": lambda: _decoder(FUSED, 128, "fused", want_gz=False),
    "decoder-callers_pending": lambda: _decoder(FUSED, 128, "deferred", own_pending=False),
    "per_sample-latents_only": lambda: _per_sample(True),
    "per_sample-all_layers": lambda: _per_sample(False),
    "quantiser-plain": lambda: _quantiser("plain"),
    "quantiser-deferred_scalars": lambda: _quantiser("deferred"),
    "quantiser-latents": lambda: _quantiser("latents"),
    # a width no fused kernel is built for, B = 2, 64 x 64: every two-launch fallback and _head_backward_unfused
    "narrow-encoder": lambda: _encoder(NARROW, 64, want_dx=True),
    "narrow-encoder-eval": lambda: _encoder(NARROW, 64, eval_mode=True),
    "narrow-decoder": lambda: _decoder(NARROW, 64, "fused"),
    "narrow-decoder-gdec_ext": lambda: _decoder(NARROW, 64, "ext"),
    "narrow-decoder-gdec_ext_only": lambda: _decoder(NARROW, 64, "ext_only", want_gz=False),
    # VQ_VAE_z32, B = 2, 128 x 128: the example widths (64 / 64 / 512) and the default ones (16 / 32 / 64)
    "z32-wide-shared_pending": lambda: _z32("shared", **WIDE),
    "z32-wide-own_pending-want_dx": lambda: _z32("own", want_dx=True, **WIDE),
    "z32-wide-no_gr": lambda: _z32("own", want_gr=False, **WIDE),
    "z32-default-shared_pending": lambda: _z32("shared"),
    "z32-default-own_pending-want_dx": lambda: _z32("own", want_dx=True),
}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_covers_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_launch_sequence_is_the_recorded_one(recorded, case):
    import torch
    got = json.loads(json.dumps(CASES[case]()))
    torch.cuda.synchronize()
    want = recorded[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: call {i} is {g}, recorded {w}"
    assert len(got) == len(want), f"{case}: {len(got)} calls, recorded {len(want)}"


if __name__ == "__main__":
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {}
    for name in sorted(CASES):
        out[name] = CASES[name]()
        torch.cuda.synchronize()
        print(f"{name}: {len(out[name])} calls")
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ": [\n" + ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in v) + "\n]"
                                    for k, v in out.items()) + "\n}\n")
