"""`not gpu`: the host half of the k-means of the latents -- the reference loop of tests/helpers/kmeans_reference.py against
scikit-learn, the gaps of the whole-fit fixtures, trajectory_windows against the reference's loops, the errors raised before
any device call, dm_kmeans_*'s argument errors before any launch, and the scikit-learn interchange."""
import ctypes
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import kmeans_reference as MR  # noqa: E402


# ------------------------------------------------------------------------------------ the reference loop itself
@pytest.mark.parametrize("name", MR.FIT_FIXTURES)
def test_reference_lloyd_agrees_with_scikit_learn(name):
    """The helper with float64 centres against sklearn.cluster.KMeans(init=C0, n_init=1, algorithm='lloyd') on the float64
    copy of the fixture: labels and n_iter_ equal, centres within 1e-12, inertia within 1e-12 relative."""
    skc = pytest.importorskip("sklearn.cluster")
    X, C0 = MR.fit_fixture(name)
    ref = MR.lloyd(X, C0.astype(np.float64), centre_dtype=np.float64)
    sk = skc.KMeans(n_clusters=C0.shape[0], init=C0.astype(np.float64), n_init=1, algorithm="lloyd").fit(X.astype(np.float64))
    assert np.array_equal(sk.labels_, ref["labels"])
    assert sk.n_iter_ == ref["n_iter"]
    assert np.abs(sk.cluster_centers_ - ref["centres"]).max() <= 1e-12
    assert abs(sk.inertia_ - ref["inertia"]) <= 1e-12 * ref["inertia"]
    assert ref["relocations"] == (1 if name == "empty_cluster" else 0)


@pytest.mark.parametrize("name,iterations", [("blobs_1000x37", 7), ("offset_600x64", 4), ("wide_300x4096", 2)])
def test_whole_fit_fixtures_keep_clear_of_ties(name, iterations):
    """The fp32-centre reference of every whole-fit fixture: the smallest relative top-2 gap over all rows and iterations is
    at least 1e-4, ten times the threshold below which the GPU test does not hold a label to the float64 argmin."""
    ref = MR.fit_reference(name)
    print(f"{name}: n_iter {ref['n_iter']}, smallest top-2 gap {ref['min_gap']:.3e}")
    assert ref["min_gap"] >= 1e-4
    assert ref["n_iter"] == iterations and ref["relocations"] == 0


def test_empty_cluster_fixture_relocates_once():
    ref = MR.fit_reference("empty_cluster")
    print(f"empty_cluster: n_iter {ref['n_iter']}, smallest top-2 gap {ref['min_gap']:.3e}")
    assert ref["relocations"] == 1 and ref["min_gap"] >= 1e-4
    assert np.bincount(ref["labels"], minlength=4).min() >= 1


def test_criterion_catches_each_defect():
    X, C = MR.randn(202, (300, 12)), MR.init_rows(300, MR.randn(202, (300, 12)), 7)
    d2 = MR.d2_float64(X, C)
    labels = np.argmin(d2, axis=1).astype(np.int32)
    dist = np.sqrt(d2[np.arange(300), labels]).astype(np.float32)
    assert MR.failing_rows(labels, dist, X, C)[0] == {}
    l2 = labels.copy()
    l2[3] = np.argmax(d2[3])
    assert 3 in MR.failing_rows(l2, dist, X, C)[0]
    d_2 = dist.copy()
    d_2[7] *= np.float32(1 + 1e-5)
    assert 7 in MR.failing_rows(labels, d_2, X, C)[0]
    l2 = labels.copy()
    l2[9] = 7
    assert 9 in MR.failing_rows(l2, dist, X, C)[0]
    Ceq = C.copy()
    Ceq[5] = Ceq[2]                                  # equal centres: the rows nearest to them have no gap
    with pytest.raises(AssertionError, match="top-2 gap"):
        lab = np.argmin(MR.d2_float64(X, Ceq), axis=1)
        MR.assert_assign(lab, None, X, Ceq, "equal centres")


def test_seed_rows_follow_the_rule():
    X, _ = MR.fit_fixture("blobs_1000x37")
    a, b = MR.seed_rows(X, 5, 0, 0), MR.seed_rows(X, 5, 0, 1)
    assert a.shape == (5,) and len(set(a.tolist())) == 5 and not np.array_equal(a, b)
    assert np.array_equal(a, MR.seed_rows(X, 5, 0, 0))
    from dynamorph_amd.kmeans import seed_uniforms
    u = seed_uniforms(0, 0, 5)
    assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all() and a[0] == int(np.floor(u[0] * 1000))
    assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53))          # 53 bits


# ------------------------------------------------------------------------------------------------ trajectory windows
def _reference_windows(vs, traj_list, length):
    """generate_short_traj_morphorlogy, restated literally."""
    short_trajs = []
    for t in traj_list:
        n_sub_trajs = len(t) - (length - 1)
        for i in range(n_sub_trajs):
            sub_traj = t[i:(i + length)]
            sub_v = vs[np.array(sub_traj)]
            short_trajs.append(sub_v)
    short_trajs = np.stack(short_trajs, 0).reshape((len(short_trajs), -1))
    return short_trajs


@pytest.mark.parametrize("length", [5, 2])
def test_trajectory_windows_match_the_reference(length):
    from dynamorph_amd.dim_reduction import trajectory_windows
    rng = np.random.default_rng(3)
    vs = rng.standard_normal((40, 3)).astype(np.float32)
    trajs = {"a/1": [0, 1, 2, 3, 4, 5, 6], "a/2": [10, 11, 12], "b/1": [20, 22, 21, 23, 24], "b/2": [30],
             "c/1": list(range(31, 40))}
    w, own = trajectory_windows(vs, trajs, length=length)
    ref = _reference_windows(vs, list(trajs.values()), length)
    assert w.dtype == np.float32 and w.shape == ref.shape == (len(own), length * 3) and np.array_equal(w, ref)
    names = list(trajs)
    for o, t in enumerate(names):
        n = max(len(trajs[t]) - (length - 1), 0)
        assert (own == o).sum() == n                 # a trajectory shorter than `length` contributes nothing
        if n:
            assert np.array_equal(w[own == o], _reference_windows(vs, [trajs[t]], length))
    wd, ownd = trajectory_windows(vs, trajs, length=length, diffs=True)
    st = ref.reshape(len(ref), length, 3)
    refd = (st[:, 1:] - st[:, :-1]).reshape((len(ref), -1))       # Kmean_on_short_traj_diffs on the (n, length, F) windows
    assert wd.shape == (len(ref), (length - 1) * 3) and np.array_equal(wd, refd) and np.array_equal(ownd, own)
    e, eo = trajectory_windows(vs, {"x": [1, 2]}, length=5)
    assert e.shape == (0, 15) and eo.shape == (0,)
    with pytest.raises(ValueError):
        trajectory_windows(vs[0], trajs)
    with pytest.raises(ValueError):
        trajectory_windows(vs, trajs, length=1, diffs=True)


# ------------------------------------------------------------------------------- errors before any device call
def test_constructor_and_shape_errors(monkeypatch):
    import torch
    from dynamorph_amd import KMeans
    from dynamorph_amd import kmeans as KM

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(KM._knn, "_resident", no_device)
    for bad in (0, -1, 1025):
        with pytest.raises(ValueError, match="n_clusters"):
            KMeans(bad)
    with pytest.raises(ValueError, match="init"):
        KMeans(3, init="random")
    with pytest.raises(ValueError, match="init has shape"):
        KMeans(3, init=np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="init has shape"):
        KMeans(3, init=np.zeros(5, np.float32))
    with pytest.raises(ValueError, match="init has shape"):
        KMeans(3, init=np.zeros((3, 5), np.float32)).fit(np.zeros((10, 6), np.float32))
    with pytest.raises(ValueError, match="exceeds"):
        KMeans(11).fit(np.zeros((10, 4), np.float32))
    with pytest.raises(ValueError, match="PCA"):
        KMeans(2).fit(torch.zeros((10, 16385)))
    with pytest.raises(ValueError, match="2-D"):
        KMeans(2).fit(np.zeros(10, np.float32))
    with pytest.raises(ValueError, match="not fitted"):
        KMeans(2).predict(np.zeros((3, 4), np.float32))
    assert KMeans(1024).n_clusters == 1024 and KMeans(4).n_init == 10 and KMeans(4).max_iter == 300


# ------------------------------------------------------------------------------------- the C ABI, without a device
@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    return _lib.load()


def test_dm_kmeans_workspace_bytes(lib):
    w = [lib.dm_kmeans_workspace_bytes(N, 256, 64) for N in (1, 100, 1000, 20000, 100000)]
    assert all(b > 0 for b in w) and all(a <= b for a, b in zip(w, w[1:])) and w[0] < w[-1]
    assert lib.dm_kmeans_workspace_bytes(1, 1, 1) > 0 and lib.dm_kmeans_workspace_bytes(100000, 16384, 1024) > 0
    for bad in ((0, 4, 1), (-5, 4, 1), (1 << 31, 4, 1), (10, 0, 1), (10, 16385, 1), (10, 4, 0), (10, 4, 1025), (10, 4, -1)):
        assert lib.dm_kmeans_workspace_bytes(*bad) == -1, bad


def test_dm_kmeans_argument_errors_before_any_launch(lib):
    """Every refusal is made on the host (negative return, dm_last_error text); the pointers are never dereferenced."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255        # a 256-byte aligned host address standing in for device memory
    big = 1 << 40

    def assign(X=p, N=100, F=64, ldx=64, C=p, K=4, labels=p, nre=p, ws=p, ws_bytes=big):
        return lib.dm_kmeans_assign(X, N, F, ldx, C, K, None, labels, None, nre, ws, ws_bytes, None)

    def sums(X=p, N=100, F=64, ldx=64, labels=p, K=4, out=p, counts=p, ws=p, ws_bytes=big):
        return lib.dm_kmeans_sums(X, N, F, ldx, labels, K, out, counts, ws, ws_bytes, None)

    def row_d2(X=p, N=100, F=64, ldx=64, C=p, K=4, d2=p):
        return lib.dm_kmeans_row_d2(X, N, F, ldx, C, K, None, d2, None)

    need = lib.dm_kmeans_workspace_bytes(100, 64, 4)
    for call, who in ((assign, b"dm_kmeans_assign"), (sums, b"dm_kmeans_sums")):
        for kw, text in ((dict(X=None), b"NULL"), (dict(labels=None), b"NULL"), (dict(ws=None), b"NULL"),
                         (dict(ldx=63), b"leading dimension"), (dict(N=0), b"N outside"), (dict(F=0), b"F outside"),
                         (dict(F=16385, ldx=16385), b"F outside"), (dict(K=0), b"K outside"), (dict(K=1025), b"K outside"),
                         (dict(ws_bytes=need - 1), b"workspace"), (dict(ws=p + 4), b"aligned")):
            rc = call(**kw)
            assert rc == -1 and text in lib.dm_last_error() and who in lib.dm_last_error(), (kw, rc, lib.dm_last_error())
    assert assign(C=None) == -1 and assign(nre=None) == -1 and sums(out=None) == -1 and sums(counts=None) == -1
    for kw, text in ((dict(X=None), b"NULL"), (dict(C=None), b"NULL"), (dict(d2=None), b"NULL"), (dict(ldx=63), b"leading"),
                     (dict(K=0), b"K outside"), (dict(N=0), b"N outside")):
        rc = row_d2(**kw)
        assert rc == -1 and text in lib.dm_last_error(), (kw, rc, lib.dm_last_error())
    from dynamorph_amd import _lib
    with pytest.raises(ValueError, match="dm_kmeans_assign"):
        _lib.check(assign(K=0), "dm_kmeans_assign")


# --------------------------------------------------------------------------------------- scikit-learn interchange
def _fitted_host_model():
    """A KMeans with the reference's result as its state: what fit leaves on the host."""
    from dynamorph_amd import KMeans
    X, C0 = MR.fit_fixture("blobs_1000x37")
    ref = MR.fit_reference("blobs_1000x37")
    m = KMeans(5, init=C0)
    m.cluster_centers_, m.labels_, m.inertia_, m.n_iter_ = ref["centres"], ref["labels"], ref["inertia"], ref["n_iter"]
    m.n_features_in_, m.rechecked_ = 37, 0
    return m, X, ref


def test_to_sklearn_round_trip_predicts():
    pytest.importorskip("sklearn.cluster")
    m, X, ref = _fitted_host_model()
    sk = m.to_sklearn()
    raw = pickle.dumps(sk, protocol=4)
    assert raw[:2] == b"\x80\x04"
    sk2 = pickle.loads(raw)
    assert sk2.algorithm == "lloyd" and sk2.n_clusters == 5 and sk2.n_iter_ == ref["n_iter"] and sk2.n_features_in_ == 37
    assert sk2.cluster_centers_.dtype == np.float32 and sk2.labels_.dtype == np.int32
    assert np.array_equal(sk2.predict(X), ref["labels"])
    from dynamorph_amd import KMeans
    back = KMeans.from_sklearn(sk2)
    assert np.array_equal(back.cluster_centers_, ref["centres"]) and back.n_features_in_ == 37 and back.n_clusters == 5
    assert np.array_equal(back.labels_, ref["labels"]) and back.inertia_ == ref["inertia"]
    m2 = pickle.loads(pickle.dumps(m, protocol=4))                 # this package's own object pickles as well
    assert np.array_equal(m2.cluster_centers_, ref["centres"])


def test_fit_kmeans_and_process_kmeans_files(tmp_path, monkeypatch):
    """The drop-ins around a stand-in fit / predict (the reference loop): file names, protocol, dtypes."""
    pytest.importorskip("sklearn.cluster")
    from dynamorph_amd import dim_reduction as DR
    from dynamorph_amd import kmeans as KM
    X, C0 = MR.fit_fixture("blobs_1000x37")
    ref = MR.fit_reference("blobs_1000x37")

    def fit(self, data):
        assert np.array_equal(np.asarray(data), X)
        self.cluster_centers_, self.labels_, self.inertia_, self.n_iter_ = (ref["centres"], ref["labels"], ref["inertia"],
                                                                              ref["n_iter"])
        self.n_features_in_, self.rechecked_ = X.shape[1], 0
        return self

    def predict(self, data, **kw):
        return np.argmin(MR.d2_float64(np.asarray(data, np.float32), self.cluster_centers_), axis=1).astype(np.int32)

    monkeypatch.setattr(KM.KMeans, "fit", fit)
    monkeypatch.setattr(KM.KMeans, "predict", predict)
    model = DR.fit_kmeans(X, str(tmp_path / "w"), n_clusters=5, init=C0)
    assert os.listdir(tmp_path / "w") == ["kmeans_model.pkl"] and model.n_clusters == 5
    raw = open(tmp_path / "w" / "kmeans_model.pkl", "rb").read()
    assert raw[:2] == b"\x80\x04" and type(pickle.loads(raw)).__module__.startswith("sklearn.")
    os.makedirs(tmp_path / "in")
    with open(tmp_path / "in" / "A_latent_space_after_PCAed.pkl", "wb") as f:
        pickle.dump(X[:100], f, protocol=4)
    out = DR.process_kmeans(str(tmp_path / "in"), str(tmp_path / "out"), str(tmp_path / "w"), "A")
    assert os.listdir(tmp_path / "out") == ["A_latent_space_after_PCAed_clusters.pkl"]
    got = pickle.load(open(tmp_path / "out" / "A_latent_space_after_PCAed_clusters.pkl", "rb"))
    assert got.dtype == np.int32 and np.array_equal(got, out) and np.array_equal(got, ref["labels"][:100])
