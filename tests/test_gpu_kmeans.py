"""The k-means of the latents on the GPU (csrc/kmeans.hip, dynamorph_amd/kmeans.py) against the float64
reference of tests/helpers/kmeans_reference.py: one labelling pass against the complete criterion and, to the bit, against
knn_query(C, X, 1); invariance to the shift, the chunking, the row stride and the launch; the per-cluster sums; whole fits
from a given init (labels and n_iter_ equal, centres within one fp32 ulp); the stops; the seeding; the pipeline drop-ins."""
import ctypes
import functools
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kmeans_reference as MR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def assign(X, C, shift="mean"):
    """(labels int32, dist fp32, rechecked) of one labelling pass; shift: "mean" (the fp32 column mean), None or an array."""
    from dynamorph_amd import knn, ops
    x = X if torch.is_tensor(X) else dev(X)
    s = knn.column_shift(x) if isinstance(shift, str) else (None if shift is None else dev(shift))
    labels, dist, n = ops.kmeans_assign(x, dev(C), s)
    return labels.cpu().numpy(), dist.cpu().numpy(), int(n.item())


@functools.lru_cache(maxsize=None)
def assign_case(name):
    if name == "ragged_1000x37_k7":
        X = MR.randn(202, (1000, 37))
        C = MR.init_rows(300, X, 7)
    elif name == "wide_300x4096_k4":
        X = MR.randn(207, (300, 4096))
        C = MR.init_rows(300, X, 4)
    elif name == "tiles_5000x32_k200":
        X = MR.blobs(204, 5000, 32, 200, sep=1.)
        C = MR.init_rows(300, X, 200)
    elif name in ("2000x16_k129", "2000x16_k1024"):
        X = MR.randn(208, (2000, 16))
        C = MR.init_rows(300, X, int(name.split("_k")[1]))
    elif name == "1000x37_k1":
        X = MR.randn(202, (1000, 37))
        C = MR.init_rows(300, X, 1)
    elif name == "2x1_k2":
        X = np.array([[0.25], [-1.5]], np.float32)
        C = np.array([[-0.75], [0.5]], np.float32)
    elif name == "offset_600x64_k4":
        X = MR.blobs(433, 600, 64, 4, off=10., scale=1e-2, sep=.6)
        C = MR.init_rows(1433, X, 4)
    else:
        raise KeyError(name)
    return X, C


ASSIGN_CASES = ("ragged_1000x37_k7", "wide_300x4096_k4", "tiles_5000x32_k200", "2000x16_k129", "2000x16_k1024", "1000x37_k1",
                "2x1_k2", "offset_600x64_k4")


# ------------------------------------------------------------------------------------------- one labelling pass
@pytest.mark.parametrize("name", ASSIGN_CASES)
def test_assign_meets_the_criterion_and_knn_query_bits(name):
    from dynamorph_amd import knn
    X, C = assign_case(name)
    labels, dist, n = assign(X, C)
    print(f"{name}: {n} of {len(X)} rows rechecked")
    MR.assert_assign(labels, dist, X, C, name)
    idx, d = knn.knn_query(C, X, 1)
    assert np.array_equal(labels, idx[:, 0].astype(np.int32))
    assert np.array_equal(dist.view(np.uint32), d[:, 0].view(np.uint32))


def test_assign_without_shift_takes_the_exact_route_to_the_same_bits():
    """Data at offset 10 with spread 1e-2: without the shift the filter's error bound exceeds every distance, no row can be
    certified, and every row is redone exactly -- to the same labels and distance bits."""
    X, C = assign_case("offset_600x64_k4")
    l0, d0, n0 = assign(X, C)
    l1, d1, n1 = assign(X, C, shift=None)
    print(f"offset_600x64_k4: {n0} rows rechecked with the shift, {n1} without")
    assert n1 == len(X)
    assert np.array_equal(l0, l1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    MR.assert_assign(l1, d1, X, C, "offset_600x64_k4 without shift")


def test_equal_centres_and_rows_that_are_centres():
    X = MR.randn(202, (1000, 37))
    C = MR.init_rows(300, X, 7)
    rows = np.sort(np.random.default_rng(300).choice(1000, 7, replace=False))      # (the rows init_rows took)
    assert np.array_equal(X[rows], C)
    C[5] = C[2]                                      # two equal centres: the higher index is never a label
    labels, dist, n = assign(X, C)
    assert not (labels == 5).any() and (labels == 2).any()
    bad, _ = MR.failing_rows(labels, dist, X, C)
    assert not bad, sorted(bad.items())[:5]
    keep = [i for i in range(7) if i != 5]           # a row that IS a centre: distance exactly 0, its own label
    assert (dist[rows[keep]] == 0).all() and np.array_equal(labels[rows[keep]], np.array(keep))
    assert (dist[np.setdiff1d(np.arange(1000), rows)] > 0).all()


# ---------------------------------------------------------------------------------------------------- invariance
def test_results_do_not_depend_on_shift_stride_chunking_or_launch():
    from dynamorph_amd import KMeans
    X = MR.randn(202, (1000, 37))
    C0 = MR.init_rows(300, X, 7)
    a = KMeans(7, init=C0).fit(X)
    b = KMeans(7, init=C0).fit(X)                    # two repeated launches
    wide = torch.zeros((1000, 48), device=DEV)
    wide[:, :37] = dev(X)
    c = KMeans(7, init=C0).fit(wide[:, :37])         # a row-strided X (ldx = 48 > F)
    for other in (b, c):
        assert np.array_equal(a.labels_, other.labels_) and a.n_iter_ == other.n_iter_ and a.inertia_ == other.inertia_
        assert np.array_equal(a.cluster_centers_.view(np.uint32), other.cluster_centers_.view(np.uint32))
    assert a.labels_.dtype == np.int32 and a.cluster_centers_.dtype == np.float32 and a.n_features_in_ == 37
    for kw in (dict(), dict(chunk_rows=333), dict(chunk_rows=64), dict(shift=None),
               dict(shift=dev(np.full(37, 0.5, np.float32)), chunk_rows=500)):
        assert np.array_equal(a.predict(X, **kw), a.labels_), kw
    assert np.array_equal(a.predict(dev(X), chunk_rows=300), a.labels_)
    assert np.array_equal(a.predict(wide[:, :37]), a.labels_)
    assert np.array_equal(a.predict(X[:3]), a.labels_[:3])          # fewer rows than clusters
    l0, d0, _ = assign(X, a.cluster_centers_)
    for shift in (None, np.full(37, -2.0, np.float32)):
        l1, d1, _ = assign(X, a.cluster_centers_, shift=shift)
        assert np.array_equal(l0, l1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
    l2, d2, _ = assign(wide[:, :37], a.cluster_centers_)
    assert np.array_equal(l0, l2) and np.array_equal(d0.view(np.uint32), d2.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("shape", [(1000, 37), (700, 256), (3, 5)])
def test_sums_are_exact_counts_and_float64_means(shape):
    from dynamorph_amd import ops
    N, F = shape
    K = 6
    X = MR.randn(210, shape) + np.float32(3)
    labels = np.random.default_rng(211).integers(0, K - 1, N).astype(np.int32)
    labels[labels == 3] = 5                          # cluster 3 has no rows
    x, lab = dev(X), dev(labels)
    sums, counts = ops.kmeans_sums(x, lab, K)
    sums2, counts2 = ops.kmeans_sums(x, lab, K)
    wide = torch.zeros((N, F + 11), device=DEV)
    wide[:, :F] = x
    sums3, _ = ops.kmeans_sums(wide[:, :F], lab, K)
    assert torch.equal(sums, sums2) and torch.equal(counts, counts2) and torch.equal(sums, sums3)
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    assert counts.dtype == np.int64 and sums.dtype == np.float64
    assert np.array_equal(counts, np.bincount(labels, minlength=K))
    assert counts[3] == 0 and not sums[3].any()
    ref, _ = MR.cluster_sums(X, labels, K)
    live = counts > 0
    mean64 = ref[live] / counts[live, None]
    got = (sums[live] / counts[live, None]).astype(np.float32)
    assert (np.abs(got.astype(np.float64) - mean64) <= np.spacing(np.abs(mean64).astype(np.float32))).all()
    assert np.abs(sums[live] - ref[live]).max() <= 1e-12 * np.abs(ref[live]).max()
    d2 = ops.kmeans_row_d2(x, dev(got), dev(np.flatnonzero(live).searchsorted(labels).astype(np.int32))).cpu().numpy()
    want = MR.d2_float64(X, got)[np.arange(N), np.flatnonzero(live).searchsorted(labels)]
    assert d2.dtype == np.float64 and np.abs(d2 - want).max() <= MR.TAU * want.max()


# ----------------------------------------------------------------------------------------------------- whole fit
def ulp_close(got, ref):
    return (np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref).astype(np.float32))).all()


@pytest.mark.parametrize("name", MR.FIT_FIXTURES)
def test_fit_from_a_given_init_equals_the_reference(name):
    from dynamorph_amd import KMeans
    X, C0 = MR.fit_fixture(name)
    ref = MR.fit_reference(name)
    m = KMeans(C0.shape[0], init=C0).fit(X)
    print(f"{name}: n_iter {m.n_iter_} (reference {ref['n_iter']}), {m.rechecked_} rows rechecked, "
          f"inertia {m.inertia_!r} (reference {ref['inertia']!r})")
    assert m.n_iter_ == ref["n_iter"]
    assert np.array_equal(m.labels_, ref["labels"])
    assert ulp_close(m.cluster_centers_, ref["centres"])
    assert abs(m.inertia_ - ref["inertia"]) <= 1e-6 * ref["inertia"]
    if name == "empty_cluster":
        assert ref["relocations"] == 1
        try:                                         # (without scikit-learn: tests/test_kmeans_host.py holds the reference to it)
            import sklearn.cluster as skc
        except ImportError:
            return
        sk = skc.KMeans(n_clusters=4, init=C0.astype(np.float64), n_init=1, algorithm="lloyd").fit(X.astype(np.float64))
        assert np.array_equal(m.labels_, sk.labels_)
        assert np.array_equal(m.fit_predict(X), sk.labels_)


def test_stops_at_max_iter_and_on_the_shift():
    from dynamorph_amd import KMeans
    X, C0 = MR.fit_fixture("blobs_1000x37")
    one = MR.fit_reference("blobs_1000x37", max_iter=1)
    m = KMeans(5, init=C0, max_iter=1).fit(X)
    assert m.n_iter_ == 1 == one["n_iter"] and not one["strict"]
    assert np.array_equal(m.labels_, one["labels"])                 # (the extra labelling pass: labels of the NEW centres)
    assert not np.array_equal(one["labels"], np.argmin(MR.d2_float64(X, C0), axis=1))
    assert ulp_close(m.cluster_centers_, one["centres"])
    loose = MR.fit_reference("blobs_1000x37", tol=0.1)
    assert not loose["strict"] and loose["n_iter"] == 5 < MR.fit_reference("blobs_1000x37")["n_iter"]
    m = KMeans(5, init=C0, tol=0.1).fit(X)
    assert m.n_iter_ == 5 and np.array_equal(m.labels_, loose["labels"]) and ulp_close(m.cluster_centers_, loose["centres"])


# ------------------------------------------------------------------------------------------------------- seeding
def test_kmeans_plus_plus_rows_runs_and_repeats():
    from dynamorph_amd import KMeans
    X, _ = MR.fit_fixture("blobs_1000x37")
    x = dev(X)
    for seed in (0, 1):
        got = KMeans(5, seed=seed)._seed_rows(x, 0).cpu().numpy()
        assert np.array_equal(got, MR.seed_rows(X, 5, seed, 0)), seed
    runs = [KMeans(5, init=X[MR.seed_rows(X, 5, 0, r)]).fit(X) for r in range(3)]
    inertias = [r.inertia_ for r in runs]
    best = runs[int(np.argmin(inertias))]            # (argmin: the lowest run of equal inertias)
    print("inertia per run:", inertias)
    m = KMeans(5, n_init=3, seed=0).fit(X)
    assert m.inertia_ == min(inertias) and np.array_equal(m.labels_, best.labels_) and m.n_iter_ == best.n_iter_
    assert np.array_equal(m.cluster_centers_.view(np.uint32), best.cluster_centers_.view(np.uint32))
    again = KMeans(5, n_init=3, seed=0).fit(X)
    assert again.inertia_ == m.inertia_ and np.array_equal(again.labels_, m.labels_)
    assert np.array_equal(again.cluster_centers_.view(np.uint32), m.cluster_centers_.view(np.uint32))


# ------------------------------------------------------------------------------------------------------ pipeline
def test_fit_kmeans_process_kmeans_and_short_trajectories(tmp_path):
    from dynamorph_amd import dim_reduction as DR
    X, C0 = MR.fit_fixture("blobs_1000x37")
    ref = MR.fit_reference("blobs_1000x37")
    model = DR.fit_kmeans(X, str(tmp_path / "w"), n_clusters=5, init=C0)
    assert os.listdir(tmp_path / "w") == ["kmeans_model.pkl"] and np.array_equal(model.labels_, ref["labels"])
    raw = open(tmp_path / "w" / "kmeans_model.pkl", "rb").read()
    assert raw[:2] == b"\x80\x04"
    os.makedirs(tmp_path / "in")
    with open(tmp_path / "in" / "A_latent_space_after_PCAed.pkl", "wb") as f:
        pickle.dump(X[:300], f, protocol=4)
    out = DR.process_kmeans(str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "w"), "A")
    assert os.listdir(tmp_path / "out") == ["A_latent_space_after_PCAed_clusters.pkl"]
    got = pickle.load(open(tmp_path / "out" / "A_latent_space_after_PCAed_clusters.pkl", "rb"))
    assert got.dtype == np.int32 and got.shape == (300,) and np.array_equal(got, out)
    assert np.array_equal(got, model.predict(X[:300])) and np.array_equal(got, ref["labels"][:300])

    vs = MR.blobs(440, 60, 6, 3)                     # 6 short trajectories over 60 frames of 6 descriptors
    trajs = {"w/0": list(range(0, 9)), "w/1": list(range(9, 16)), "w/2": [20, 21], "w/3": list(range(30, 36)),
             "w/4": list(range(40, 45)), "w/5": list(range(50, 60))}
    for diffs in (False, True):
        windows, owners = DR.trajectory_windows(vs, trajs, length=5, diffs=diffs)
        W0 = MR.init_rows(441, windows, 3)
        want = MR.lloyd(windows, W0)
        assert want["min_gap"] > MR.GAP
        res = DR.kmeans_on_short_trajs(vs, trajs, length=5, n_clusters=3, diffs=diffs, init=W0)
        assert list(res) == list(trajs)
        for o, t in enumerate(trajs):
            assert res[t].dtype == np.int32 and np.array_equal(res[t], want["labels"][owners == o]), (diffs, t)
        assert len(res["w/2"]) == 0 and len(res["w/0"]) == 5


# ----------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_are_reported_before_any_launch():
    from dynamorph_amd import _lib, ops
    lib = _lib.load()
    x, C = dev(MR.randn(1, (100, 64))), dev(MR.randn(2, (4, 64)))
    labels = torch.full((100,), -7, dtype=torch.int32, device=DEV)
    n = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ws = ops.kmeans_workspace(100, 64, 4, x)
    sums = torch.zeros((4, 64), dtype=torch.float64, device=DEV)
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    need = lib.dm_kmeans_workspace_bytes(100, 64, 4)
    for args, text in (
        ((None, 100, 64, 64, p(C), 4, None, p(labels), None, p(n), p(ws), ws.numel(), stream), b"NULL"),
        ((p(x), 100, 64, 64, None, 4, None, p(labels), None, p(n), p(ws), ws.numel(), stream), b"NULL"),
        ((p(x), 100, 64, 64, p(C), 4, None, None, None, p(n), p(ws), ws.numel(), stream), b"NULL"),
        ((p(x), 100, 64, 63, p(C), 4, None, p(labels), None, p(n), p(ws), ws.numel(), stream), b"leading dimension"),
        ((p(x), 100, 64, 64, p(C), 4, None, p(labels), None, p(n), p(ws), need - 1, stream), b"workspace"),
        ((p(x), 100, 64, 64, p(C), 4, None, p(labels), None, p(n), None, need, stream), b"NULL"),
    ):
        assert lib.dm_kmeans_assign(*args) == -1 and text in lib.dm_last_error(), (text, lib.dm_last_error())
    assert lib.dm_kmeans_sums(p(x), 100, 64, 63, p(labels), 4, p(sums), p(counts), p(ws), ws.numel(), stream) == -1
    assert lib.dm_kmeans_sums(p(x), 100, 64, 64, p(labels), 4, None, p(counts), p(ws), ws.numel(), stream) == -1
    assert lib.dm_kmeans_sums(p(x), 100, 64, 64, p(labels), 4, p(sums), p(counts), p(ws), need - 1, stream) == -1
    assert lib.dm_kmeans_row_d2(p(x), 100, 64, 63, p(C), 4, None, p(sums), stream) == -1
    torch.cuda.synchronize()
    assert (labels == -7).all() and int(n.item()) == -7 and not sums.any() and not counts.any()     # nothing ran
    with pytest.raises(ValueError, match="shift"):
        ops.kmeans_assign(x, C, torch.zeros(63, device=DEV))
    with pytest.raises(ValueError, match="need"):
        ops.kmeans_assign(x, dev(MR.randn(2, (4, 63))))
