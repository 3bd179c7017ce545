"""`not gpu`: the host half of the UMAP transform -- the fixture of the GPU tests and what it
exercises, the restatement's own search, argument refusal before any device call, C-ABI argument errors before any launch,
the pickle round trip of a model's host state, and the file names of the pipeline wrappers."""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import umap_reference as UR  # noqa: E402
import umap_transform_reference as TR  # noqa: E402

from dynamorph_amd import umap_layout as U  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    X, Q, y_train = TR.fixture()
    idx, dist = TR.query_knn_float64(X, Q, 256)
    return X, Q, y_train, idx, dist


# floored rows, searches out of steps, pruned entries, rows with a pruned entry: what the definition gives on the fixture
COUNTS = {2: (0, 1, 1, 1), 15: (1, 1, 10, 1), 200: (0, 0, 7014, 70), 256: (0, 0, 10928, 70)}


@pytest.mark.parametrize("k", TR.KS)
def test_fixture_exercises_floor_pruning_and_submaximal_rows(fx, k):
    X, Q, y_train, idx, dist = fx
    assert X.shape == (300, 32) and Q.shape == (70, 32) and y_train.shape == (300, 2) and y_train.dtype == np.float32
    assert (X[1:5] == X[0]).all() and (Q[0] == X[0]).all() and (Q[1] == X[7]).all() and (Q[3] == Q[2]).all()
    assert y_train.min() >= 0 and y_train.max() <= 10
    p = TR.prepare(idx[:, :k], dist[:, :k], y_train, TR.N_EPOCHS_T)
    got = (int(p["floored"].sum()), int(p["out_of_steps"].sum()), int(p["pruned"].sum()), int(p["pruned"].any(1).sum()))
    print(f"k={k}: floored, out of steps, pruned, rows with pruned = {got}")
    assert got == COUNTS[k]
    assert int((p["a"].max(1) < 1).sum()) == 68                      # the row maximum is not 1: eps = m / a needs m
    assert np.isinf(p["eps"][p["pruned"]]).all() and np.isfinite(p["eps"][~p["pruned"]]).all()
    assert (p["eps"][~p["pruned"]] >= 1).all() and (p["eps"].min(1) == 1).all()
    if k == 2:
        assert not dist[0, :2].any() and p["out_of_steps"][0]         # Q[0]: both distances 0
    if k == 15:
        assert p["floored"][0] and (dist[0, :5] == 0).all() and dist[0, 5] > 0
        assert p["pruned"][0].sum() == 10 and (p["a"][0, 5:] == 0).all()           # underflow behind the floor
    # the pruned entries are the far end of a sorted row
    assert (np.diff(p["pruned"].astype(np.int8), axis=1) >= 0).all()
    assert np.isfinite(p["y0"]).all() and p["y0"].min() >= 0 and p["y0"].max() <= 10


@pytest.mark.parametrize("k", TR.KS)
def test_helper_sigma_solves_its_equation(fx, k):
    dist = fx[4][:, :k]
    sigma, floored, out_of_steps, sigma64 = TR.smooth(dist, full=True)
    exempt = floored | out_of_steps
    err64 = np.abs(TR.S(dist, sigma64) - np.log2(k))
    err32 = np.abs(TR.S(dist, sigma.astype(np.float64)) - np.log2(k))
    print(f"k={k}: |S - log2 k| <= {err64[~exempt].max():.2e} (float64 sigma), {err32[~exempt].max():.2e} (float32 sigma)")
    assert err64[~exempt].max() <= 1e-5 and err32[~exempt].max() <= 2e-5
    assert np.array_equal(sigma[floored], TR.floors(dist)[floored].astype(np.float32))


def test_schedule_state_advances_as_the_epoch_does(fx):
    """advance (vectorised, state only) and epoch (the whole definition) keep the same float32 state."""
    X, Q, y_train, idx, dist = fx
    p = TR.prepare(idx[:, :15], dist[:, :15], y_train)
    nxt, nxt_neg = TR.state_at(p["eps"], p["eps_neg"], 7)
    _, n1, q1, counts = TR.epoch(idx[:, :15], p["eps"], p["eps_neg"], nxt, nxt_neg, y_train, p["y0"].astype(np.float32), 7,
                                 TR.N_EPOCHS_T, 1.58, 0.9, 1.0, 3, dtype=np.float32)
    n2, q2 = TR.advance(p["eps"], p["eps_neg"], nxt, nxt_neg, 7)
    assert counts["fired"] > 0 and counts["negatives"] > 0
    assert np.array_equal(n1.view(np.uint32), n2.view(np.uint32)) and np.array_equal(q1.view(np.uint32), q2.view(np.uint32))


def _fitted_model(X, y_train, k=15, with_data=True):
    m = U.UMAPEmbedding(n_neighbors=k, seed=9)
    m.embedding_, m.n_epochs_ = y_train, 200
    m._X = X if with_data else None
    return m


def test_refused_arguments_raise_before_any_device_call(monkeypatch, fx):
    from dynamorph_amd import knn, ops
    X, Q, y_train, idx, dist = fx

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    for name in ("umap_transform_prepare", "umap_transform_layout", "knn", "pca_colsum"):
        monkeypatch.setattr(ops, name, no_device)
    for name in ("knn_query", "_resident", "column_shift"):
        monkeypatch.setattr(knn, name, no_device)
    with pytest.raises(ValueError, match="no training data"):
        _fitted_model(X, y_train, with_data=False).transform(Q)
    with pytest.raises(ValueError, match="no embedding"):
        U.UMAPEmbedding().transform(Q)
    with pytest.raises(ValueError, match="no embedding"):
        U.UMAPEmbedding().transform_graph(idx[:, :15], dist[:, :15])
    with pytest.raises(ValueError, match="exceeds"):
        _fitted_model(X[:10], y_train[:10]).transform(Q)                         # k = 15 > M = 10
    with pytest.raises(ValueError, match="exceeds"):
        _fitted_model(X[:10], y_train[:10]).transform_graph(idx[:, :15] % 10, dist[:, :15])
    with pytest.raises(ValueError, match="expected"):
        _fitted_model(X, y_train).transform(Q[:, :31])                           # the wrong width
    with pytest.raises(ValueError, match="expected"):
        _fitted_model(X, y_train).transform(Q.reshape(70, 4, 8))                 # 3-D
    with pytest.raises(ValueError, match="one shape"):
        _fitted_model(X, y_train).transform_graph(idx[:, :15].reshape(70, 3, 5), dist[:, :15].reshape(70, 3, 5))
    bad = idx[:, :15].copy()
    bad[4, 6] = 300
    with pytest.raises(ValueError, match="outside 0"):
        _fitted_model(X, y_train).transform_graph(bad, dist[:, :15])
    bad[4, 6] = -1
    with pytest.raises(ValueError, match="outside 0"):
        U.check_query_graph(bad, dist[:, :15], 300)
    with pytest.raises(ValueError, match="outside 2"):
        _fitted_model(X, y_train).transform_graph(idx[:, :1], dist[:, :1])
    with pytest.raises(ValueError, match="n_epochs"):
        _fitted_model(X, y_train).transform_graph(idx[:, :15], dist[:, :15], n_epochs=0)
    with pytest.raises(ValueError, match="row_offset"):
        _fitted_model(X, y_train).transform(Q, row_offset=-1)
    with pytest.raises(ValueError, match="rows"):
        U.UMAPEmbedding().fit_graph(*UR.knn_float64(X, 15), np.zeros((300, 2), np.float32), X=X[:299])
    i64, d32 = U.check_query_graph(idx[:, :15].astype(np.int32), dist[:, :15].astype(np.float64), 300)
    assert i64.dtype == np.int64 and d32.dtype == np.float32 and i64.shape == (70, 15)


def test_cabi_transform_argument_errors_are_reported_before_any_launch():
    import ctypes
    import subprocess
    from conftest import ROOT
    subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "dynamorph_amd", "csrc")])
    from dynamorph_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)                        # never dereferenced: every call below fails its host checks

    def prepare(**kw):
        args = dict(indices=fake, dists=fake, R=10, k=5, M=20, y_train=fake, n_epochs=66, rate=5, sigma=fake, membership=fake,
                    eps=fake, eps_neg=fake, nxt=fake, nxt_neg=fake, y0=fake)
        args.update(kw)
        return lib.dm_umap_transform_prepare(*args.values(), None)
    assert prepare(dists=None) == -1 and b"NULL" in lib.dm_last_error()
    assert prepare(y0=None) == -1 and b"NULL" in lib.dm_last_error()
    assert prepare(R=0) == -1 and b"R =" in lib.dm_last_error()
    assert prepare(k=1) == -1 and b"k outside" in lib.dm_last_error()
    assert prepare(k=257, M=300) == -1 and b"k outside" in lib.dm_last_error()
    assert prepare(k=5, M=4) == -1 and b"exceeds" in lib.dm_last_error()
    assert prepare(M=2 ** 31) == -1
    assert prepare(n_epochs=0) == -1 and b"n_epochs" in lib.dm_last_error()
    assert prepare(rate=0) == -1 and b"negative_sample_rate" in lib.dm_last_error()
    assert prepare(rate=1001) == -1 and b"negative_sample_rate" in lib.dm_last_error()

    def layout(**kw):
        args = dict(indices=fake, eps=fake, eps_neg=fake, nxt=fake, nxt_neg=fake, R=10, k=5, M=20, y_train=fake, y=fake,
                    epoch_begin=0, epoch_end=66, n_epochs=66, row_offset=0, a=1.58, b=0.9, gamma=1.0, seed=0, group=0)
        args.update(kw)
        return lib.dm_umap_transform_layout(*args.values(), None)
    assert layout(y=None) == -1 and b"NULL" in lib.dm_last_error()
    assert layout(nxt_neg=None) == -1 and b"NULL" in lib.dm_last_error()
    assert layout(R=0) == -1 and b"R =" in lib.dm_last_error()
    assert layout(k=1) == -1 and b"k outside" in lib.dm_last_error()
    assert layout(k=257, M=300) == -1
    assert layout(M=4) == -1 and b"exceeds" in lib.dm_last_error()
    assert layout(M=2 ** 31) == -1
    assert layout(epoch_end=67) == -1 and b"epochs" in lib.dm_last_error()
    assert layout(epoch_begin=-1) == -1 and b"epochs" in lib.dm_last_error()
    assert layout(epoch_begin=30, epoch_end=20) == -1 and b"epochs" in lib.dm_last_error()
    assert layout(row_offset=-1) == -1 and b"row_offset" in lib.dm_last_error()
    assert layout(a=0.0) == -1 and b"positive" in lib.dm_last_error()
    assert layout(b=-1.0) == -1 and b"positive" in lib.dm_last_error()
    assert layout(group=16) == -1 and b"group" in lib.dm_last_error()
    assert layout(group=32) == -1 and b"group" in lib.dm_last_error()


def test_pickle_round_trip_of_the_host_state(fx):
    import torch
    X, Q, y_train, idx, dist = fx
    m = _fitted_model(torch.from_numpy(X.astype(np.float64)), y_train)          # a tensor, and not fp32: the state is fp32 numpy
    m._graph = (np.arange(4, dtype=np.int64), np.arange(3, dtype=np.int32), np.ones(3, np.float32), 3)
    m.rho_, m.sigma_, m.init_ = np.zeros(3, np.float32), np.ones(3, np.float32), y_train[:3]
    m.device = torch.device("cpu")
    state = m.__getstate__()
    assert isinstance(state["_X"], np.ndarray) and state["_X"].dtype == np.float32 and state["device"] == "cpu"
    assert not any(torch.is_tensor(v) for v in state.values())
    r = pickle.loads(pickle.dumps(m, protocol=4))
    assert isinstance(r, U.UMAPEmbedding) and isinstance(r._X, np.ndarray) and np.array_equal(r._X, X)
    assert np.array_equal(r.embedding_, y_train) and r.embedding_.dtype == np.float32
    assert (r.n_neighbors, r.a, r.b, r.gamma, r.negative_sample_rate, r.seed, r.n_epochs_) == (15, 1.58, 0.9, 1.0, 5, 9, 200)
    assert all(np.array_equal(x, y) for x, y in zip(r._graph[:3], m._graph[:3])) and r._graph[3] == 3
    assert r.graph().shape == (3, 3) and np.array_equal(r.sigma_, m.sigma_)
    old = dict(state)
    old.pop("_X"), old.pop("transform_group")                                   # a model pickled before this feature
    e = U.UMAPEmbedding.__new__(U.UMAPEmbedding)
    e.__setstate__(old)
    with pytest.raises(ValueError, match="no training data"):
        e.transform(Q)


def _host_pipeline(monkeypatch):
    """fit_umap_embedding with the device stages replaced: the wrapper is what runs."""
    import torch
    from dynamorph_amd import knn
    monkeypatch.setattr(knn, "_resident", lambda x, device=None: x)
    monkeypatch.setattr(knn, "knn_graph", lambda x, k, include_self=True, **kw: UR.knn_float64(x, k))
    monkeypatch.setattr(U, "pca_coordinates", lambda x, device=None: torch.from_numpy(np.asarray(x)[:, :2].copy()))

    def fit_graph(self, idx, dist, init=None, X=None):
        self.embedding_ = np.full((idx.shape[0], 2), self.n_neighbors, np.float32)
        self.n_epochs_, self._X = 500, X
        return self
    monkeypatch.setattr(U.UMAPEmbedding, "fit_graph", fit_graph)


def test_save_models_false_writes_exactly_the_files_of_before(monkeypatch, tmp_path):
    from dynamorph_amd import dim_reduction as DR
    _host_pipeline(monkeypatch)
    DR.fit_umap_embedding(UR.fixture(60, 8), str(tmp_path), labels=list(range(60)), n_nbrs=(5, 20), a_s=(1.58,), b_s=(0.9,))
    assert sorted(os.listdir(tmp_path)) == ["embedding_umap_nbr20_a1.58_b0.9.pkl", "embedding_umap_nbr5_a1.58_b0.9.pkl",
                                            "knn_nbr20.pkl", "knn_nbr5.pkl"]


def test_pipeline_file_names_with_transform_patched_out(monkeypatch, tmp_path):
    from dynamorph_amd import dim_reduction as DR
    _host_pipeline(monkeypatch)
    X = UR.fixture(60, 8)
    weights = tmp_path / "weights"
    DR.fit_umap_embedding(X, str(weights), labels=list(range(60)), n_nbrs=(5, 20), a_s=(1.58,), b_s=(0.9,), save_models=True)
    names = sorted(os.listdir(weights))
    assert names == ["embedding_umap_nbr20_a1.58_b0.9.pkl", "embedding_umap_nbr5_a1.58_b0.9.pkl", "knn_nbr20.pkl", "knn_nbr5.pkl",
                     "umap_model_nbr20_a1.58_b0.9.pkl", "umap_model_nbr5_a1.58_b0.9.pkl"]
    with open(weights / "umap_model_nbr5_a1.58_b0.9.pkl", "rb") as f:
        model = pickle.load(f)
    assert isinstance(model, U.UMAPEmbedding) and model.n_neighbors == 5 and np.array_equal(model._X, X)
    assert model._X.dtype == np.float32 and model.embedding_.shape == (60, 2)

    seen = []

    def transform(self, Q, **kw):
        seen.append((self.n_neighbors, np.asarray(Q).shape))
        return np.full((len(Q), 2), self.n_neighbors, np.float64)
    monkeypatch.setattr(U.UMAPEmbedding, "transform", transform)
    wells = [tmp_path / "B4", tmp_path / "C5"]
    outs = [tmp_path / "B4_out", tmp_path / "C5_out"]
    for w in wells:
        os.makedirs(w)
        for prefix in ("a", "b"):
            with open(w / f"{prefix}_latent_space_after.pkl", "wb") as f:
                pickle.dump(UR.fixture(7, 8, seed=1), f)
    res = DR.umap_transform(str(wells[0]), str(outs[0]), str(weights), "a")
    assert sorted(os.listdir(outs[0])) == ["a_latent_space_after_umap_model_nbr20_a1.58_b0.9.pkl",
                                           "a_latent_space_after_umap_model_nbr5_a1.58_b0.9.pkl"]
    assert sorted(res) == ["umap_model_nbr20_a1.58_b0.9", "umap_model_nbr5_a1.58_b0.9"]
    with open(outs[0] / "a_latent_space_after_umap_model_nbr5_a1.58_b0.9.pkl", "rb") as f:
        arr = pickle.load(f)
    assert arr.shape == (7, 2) and arr.dtype == np.float32 and (arr == 5).all()
    seen.clear()
    res = DR.dim_reduction_umap_transform([str(w) for w in wells], [str(o) for o in outs], str(weights), ["a", "b"])
    assert len(res) == 4 and len(seen) == 8 and all(s[1] == (7, 8) for s in seen)
    assert len(os.listdir(outs[1])) == 4 and "b_latent_space_after_umap_model_nbr20_a1.58_b0.9.pkl" in os.listdir(outs[1])
    # a umap*.pkl that is no model (the reference's own [embedding, labels] pickle under such a name): the reference's error
    with open(weights / "umap_nbr5.pkl", "wb") as f:
        pickle.dump([np.zeros((3, 2)), [0, 1, 2]], f)
    with pytest.raises(ValueError, match="Error in loading pre-saved PCA weights"):
        DR.umap_transform(str(wells[0]), str(outs[0]), str(weights), "a")
    with open(weights / "umap_nbr5.pkl", "wb") as f:
        f.write(b"not a pickle")
    with pytest.raises(ValueError, match="Error in loading pre-saved PCA weights"):
        DR.dim_reduction_umap_transform([str(wells[0])], [str(outs[0])], str(weights), "a")
