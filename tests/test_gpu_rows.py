"""dynamorph_amd/rows.py::device_chunks on the device: every kind of source assembled back to fp32(X) bit for bit while a
second kernel reads each chunk (N = 70 rows of F = 37 in chunks of 16: five chunks, a ragged tail of 6, each of the two device
buffers used again twice), the chunk-size rules, a pinned source through PCA.moments / knn_query / KMeans.predict, and a loop
left early."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, F, CR = 70, 37, 16
X64 = np.random.default_rng(70).standard_normal((N, F)) * 3.0 + 10.0
X32 = X64.astype(np.float32)

SOURCES = ("pageable_f32", "pageable_f64", "pinned_f32", "strided_cpu", "cuda")


def source(kind):
    """(X as that kind of source, the fp32 matrix its chunks must hold)."""
    if kind == "pageable_f32":
        return X32.copy(), X32
    if kind == "pageable_f64":
        return X64.copy(), X32
    if kind == "pinned_f32":
        return torch.from_numpy(X32).pin_memory(), X32
    if kind == "strided_cpu":
        wide = torch.from_numpy(np.concatenate([X32 + 1, X32, X32 - 1], axis=1))
        x = wide[:, F:2 * F]
        assert not x.is_contiguous()
        return x, X32
    if kind == "cuda":
        return torch.from_numpy(X32).to(DEV), X32
    raise KeyError(kind)


def assemble(X, chunk_rows, stop_after=None, **kw):
    """Walks device_chunks as a consumer does: per chunk a copy into `out` and a second kernel that reads the chunk (float64
    row sums).  Returns (out, row sums, [(lo, rows)]) as numpy."""
    from dynamorph_amd.rows import device_chunks
    with torch.no_grad(), torch.cuda.device(DEV):
        out = torch.full((N, F), float("nan"), device=DEV)
        sums = torch.zeros(N, dtype=torch.float64, device=DEV)
        seen = []
        for lo, chunk in device_chunks(X, chunk_rows, DEV, **kw):
            m = chunk.shape[0]
            assert chunk.is_cuda and chunk.dtype == torch.float32 and chunk.shape[1] == F and chunk.stride(1) == 1
            out[lo:lo + m].copy_(chunk)
            sums[lo:lo + m] = chunk.double().sum(1)
            seen.append((lo, m))
            if stop_after is not None and len(seen) == stop_after:
                break
        return out.cpu().numpy(), sums.cpu().numpy(), seen


def check(out, sums, want):
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    # a float64 sum of F fp32 numbers, in any order, is within F 2^-53 sum |x| of the exact one
    w = want.astype(np.float64)
    assert (np.abs(sums - w.sum(1)) <= F * 2.0 ** -53 * np.abs(w).sum(1)).all()


@pytest.mark.parametrize("kind", SOURCES)
def test_chunks_assemble_to_fp32_x(kind):
    X, want = source(kind)
    out, sums, seen = assemble(X, CR)
    assert seen == [(0, 16), (16, 16), (32, 16), (48, 16), (64, 6)]
    check(out, sums, want)
    for cr, n_chunks in ((N, 1), (N + 30, 1), (1, N)):
        out, sums, seen = assemble(X, cr)
        assert len(seen) == n_chunks and seen[0] == (0, min(cr, N))
        check(out, sums, want)


@pytest.mark.parametrize("kind", ("pageable_f64", "pinned_f32", "cuda"))
def test_max_chunk_bytes_caps_the_rows_but_not_below_one(kind):
    X, want = source(kind)
    out, sums, seen = assemble(X, CR, max_chunk_bytes=5 * 4 * F + 4 * F - 1)         # five rows and most of a sixth
    assert [m for _, m in seen] == [5] * 14
    check(out, sums, want)
    out, sums, seen = assemble(X, CR, max_chunk_bytes=1 << 20)                       # the cap does not bind
    assert [m for _, m in seen] == [16, 16, 16, 16, 6]
    out, sums, seen = assemble(X, CR, max_chunk_bytes=4 * F - 1)                     # less than one row: one row
    assert [m for _, m in seen] == [1] * N
    check(out, sums, want)


def test_pinned_rows_through_the_public_calls():
    from dynamorph_amd.kmeans import KMeans
    from dynamorph_amd.knn import knn_query
    from dynamorph_amd.pca import PCA
    pinned, _ = source("pinned_f32")
    assert pinned.is_pinned() and pinned.is_contiguous()
    n0, mean0, C0 = PCA(0.5, chunk_rows=CR).moments(X32.copy())
    n1, mean1, C1 = PCA(0.5, chunk_rows=CR).moments(pinned)
    assert n0 == n1 == N and torch.equal(mean0, mean1) and torch.equal(C0, C1)
    xd = torch.from_numpy(X32).to(DEV)
    i0, d0 = knn_query(xd, xd.clone(), 15, chunk_rows=CR)
    i1, d1 = knn_query(xd, pinned, 15, chunk_rows=CR)
    assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    km = KMeans(4, n_init=2, seed=3).fit(xd)
    assert np.array_equal(km.predict(pinned, chunk_rows=CR), km.labels_)


@pytest.mark.parametrize("kind", ("pageable_f32", "pinned_f32", "cuda"))
def test_a_loop_left_early_leaves_nothing_behind(kind):
    X, want = source(kind)
    out, _, seen = assemble(X, CR, stop_after=2)
    assert seen == [(0, 16), (16, 16)]
    assert np.array_equal(out[:32].view(np.uint32), want[:32].view(np.uint32)) and np.isnan(out[32:]).all()
    out, sums, seen = assemble(X, CR)
    assert len(seen) == 5
    check(out, sums, want)
    torch.cuda.synchronize()
