"""`gpu`: the UMAP transform of new points (dm_umap_transform_prepare, dm_umap_transform_layout, UMAPEmbedding.transform)
against the restatement of DESIGN.md section 3.5d in tests/helpers/umap_transform_reference.py, on its fixture (300 training
rows, 70 queries, k = 2, 15, 200, 256, 66 epochs): the prepare stage, single epochs teacher-forced, whole runs cut and resumed
and at every lane count, the independence of a row from the rest of the call, the quality of held-out blobs, the pipeline."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import umap_reference as UR  # noqa: E402
import umap_transform_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu

NE = TR.N_EPOCHS_T
A, B, GAMMA, SEED = 1.58, 0.9, 1.0, 9
_cache = {}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def fixture():
    """(X, Q, y_train) and the device's exact query graph at k = 256, once.  y_train is the helper's with rows 200-259 drawn
    onto a grid of spacing 0.02 at (5, 5): a fifth of all negatives lands there, and a query inside it is repelled at the
    clip."""
    from dynamorph_amd import knn as K
    if "fx" not in _cache:
        X, Q, y_train = TR.fixture()
        y_train = y_train.copy()
        y_train[200:260] = np.float32(5) + np.array([[0.02 * (t % 8), 0.02 * (t // 8)] for t in range(60)], np.float32)
        idx, dist = K.knn_query(torch.from_numpy(X).cuda(), torch.from_numpy(Q).cuda(), 256)
        _cache["fx"] = (X, Q, y_train, idx, dist)
    return _cache["fx"]


def prepared(k):
    """The device's prepare stage at k (numpy host copies and the device tensors), once per k."""
    from dynamorph_amd import ops
    if ("p", k) not in _cache:
        X, Q, y_train, idx, dist = fixture()
        idx, dist = np.ascontiguousarray(idx[:, :k]), np.ascontiguousarray(dist[:, :k])
        dev = (torch.from_numpy(idx.astype(np.int32)).cuda(), torch.from_numpy(dist).cuda(), torch.from_numpy(y_train).cuda())
        out = ops.umap_transform_prepare(dev[0], dev[1], dev[2], NE, 5)
        torch.cuda.synchronize()
        names = ("sigma", "a", "eps", "eps_neg", "next", "next_neg", "y0")
        _cache[("p", k)] = (idx, dist, dev, dict(zip(names, out)), {n: t.cpu().numpy() for n, t in zip(names, out)})
    return _cache[("p", k)]


def state_before(k, n):
    """The float32 restatement's schedule state before epoch n from the device's eps / eps_neg (test_prepare holds those to
    the float32 evaluation), advanced once per k and kept."""
    if ("s", k) not in _cache:
        h = prepared(k)[4]
        states, (nxt, nxt_neg) = {0: (h["eps"].copy(), h["eps_neg"].copy())}, (h["eps"], h["eps_neg"])
        for e in range(NE):
            nxt, nxt_neg = TR.advance(h["eps"], h["eps_neg"], nxt, nxt_neg, e)
            states[e + 1] = (nxt, nxt_neg)
        _cache[("s", k)] = states
    return _cache[("s", k)][n]


# --------------------------------------------------------------------------------------------------------------- prepare
@pytest.mark.parametrize("k", TR.KS)
def test_prepare(k):
    idx, dist, _, _, h = prepared(k)
    y_train = fixture()[2]
    sigma = h["sigma"]
    assert all(v.dtype == np.float32 for v in h.values())
    _, floored_ref, out_ref = TR.smooth(dist)
    fl = TR.floors(dist)
    assert np.array_equal(bits(sigma[floored_ref]), bits(fl[floored_ref].astype(np.float32))), "a floored row does not carry the floor"
    free = ~(floored_ref | out_ref)
    err = np.abs(TR.S(dist, sigma.astype(np.float64)) - np.log2(k))
    print(f"k={k}: {floored_ref.sum()} rows floored, {out_ref.sum()} out of steps; |S - log2 k| <= {err[free].max():.2e} on the others")
    assert free.sum() >= 68 and err[free].max() <= 2e-5
    want = TR.membership(dist, sigma)
    aerr = np.abs(h["a"].astype(np.float64) - want).max()
    print(f"k={k}: membership within {aerr:.2e} of the float64 closed form")
    assert aerr <= 1e-6
    pruned, eps, eps_neg = TR.schedule(h["a"], NE, 5)
    print(f"k={k}: {pruned.sum()} of {pruned.size} entries pruned, in {pruned.any(1).sum()} rows; {(h['a'].max(1) < 1).sum()} row maxima below 1")
    for name, ref in (("eps", eps), ("eps_neg", eps_neg), ("next", eps), ("next_neg", eps_neg)):
        assert np.array_equal(bits(h[name]), bits(ref)), f"{name} differs from the float32 evaluation of the device's memberships"
        assert np.array_equal(np.isposinf(h[name]), pruned), f"{name} is not +inf at exactly the pruned entries"
    if k >= 15:
        assert pruned.any() and not pruned.all(1).any()
    y0_64 = TR.init(idx, h["a"], y_train)
    yerr = np.abs(h["y0"].astype(np.float64) - y0_64)
    print(f"k={k}: y0 within {(yerr / np.spacing(np.abs(y0_64).astype(np.float32))).max():.2f} fp32 spacings of the float64 mean")
    assert (yerr <= np.spacing(np.abs(y0_64).astype(np.float32))).all()
    if k >= 5:
        assert not dist[0, :5].any() and (h["a"][0, :5] == 1).all()     # Q[0] = X[0] and its four copies: zero distances


# ------------------------------------------------------------------------------------------------------------ one epoch
@pytest.mark.parametrize("n", [0, 1, 30, 65])
@pytest.mark.parametrize("k", [15, 200])
def test_one_epoch_teacher_forced(k, n):
    """The kernel (range [n, n + 1)) and the float64 restatement start epoch n from the same float32 positions and the
    restatement's float32 schedule state.  Positions: y0, three queries put exactly on the training position of their first
    firing neighbour (d2 = 0) and queries 20-59 put inside the 0.02 grid of training positions, 0.01 from one of them.  The
    kernel may deviate from float64 by 4 x what a float32 numpy evaluation deviates, plus 1e-5.  Nothing fires in epoch 0
    (next = eps >= 1 by definition), so fired, coincident and clipped are asserted positive for n >= 1."""
    from dynamorph_amd import ops
    idx, dist, (i32, _, yt), d, h = prepared(k)
    y_train = fixture()[2]
    nxt, nxt_neg = state_before(k, n)
    y = h["y0"].copy()
    y[20:60] = y_train[200:240] + np.array([0.01, 0.005], np.float32)
    firing = nxt <= np.float32(n)
    on_top = [i for i in range(70) if firing[i].any() and not 20 <= i < 60][:3]
    for i in on_top:
        y[i] = y_train[idx[i, np.nonzero(firing[i])[0][0]]]
    args = (idx, h["eps"], h["eps_neg"], nxt, nxt_neg, y_train, y, n, NE, A, B, GAMMA, SEED)
    y64, nxt64, neg64, counts = TR.epoch(*args, dtype=np.float64)
    y32, nxt32, neg32, _ = TR.epoch(*args, dtype=np.float32)
    assert np.array_equal(bits(nxt64), bits(nxt32)) and np.array_equal(bits(neg64), bits(neg32))
    want_nxt, want_neg = state_before(k, n + 1)
    assert np.array_equal(bits(nxt32), bits(want_nxt)) and np.array_equal(bits(neg32), bits(want_neg))
    dn, dq, dy = torch.from_numpy(nxt).cuda(), torch.from_numpy(nxt_neg).cuda(), torch.from_numpy(y).cuda()
    ops.umap_transform_layout(i32, d["eps"], d["eps_neg"], dn, dq, yt, dy, n, n + 1, NE, 0, SEED, A, B, GAMMA)
    assert np.array_equal(bits(dn.cpu().numpy()), bits(nxt32)), "next differs from the float32 evaluation"
    assert np.array_equal(bits(dq.cpu().numpy()), bits(neg32)), "next_neg differs from the float32 evaluation"
    dev32 = np.abs(y32.astype(np.float64) - y64).max()
    err = np.abs(dy.cpu().numpy().astype(np.float64) - y64).max()
    moved = np.abs(y64 - y).max()
    print(f"k={k} epoch {n}: {counts}; largest move {moved:.3f}; float32 numpy deviates {dev32:.2e}, the kernel {err:.2e} "
          f"(allowed {4 * dev32 + 1e-5:.2e})")
    if n == 0:
        assert counts["fired"] == 0 and np.array_equal(dy.cpu().numpy(), y)
    else:
        assert len(on_top) == 3 and counts["fired"] > 0 and counts["coincident"] > 0 and counts["clipped"] > 0
        assert counts["negatives"] > 0 and moved > 0
    assert err <= 4 * dev32 + 1e-5


# ------------------------------------------------------------------------------------------------------------- whole run
def _run(k, cuts, group=0, row_offset=0):
    from dynamorph_amd import ops
    _, _, (i32, _, yt), d, _ = prepared(k)
    nxt, nxt_neg, y = d["next"].clone(), d["next_neg"].clone(), d["y0"].clone()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ops.umap_transform_layout(i32, d["eps"], d["eps_neg"], nxt, nxt_neg, yt, y, lo, hi, NE, row_offset, SEED, A, B, GAMMA, group)
    return y.cpu().numpy(), nxt.cpu().numpy(), nxt_neg.cpu().numpy()


@pytest.mark.parametrize("k", [2, 15, 200, 256])
def test_whole_run_cut_and_resumed_and_at_every_lane_count(k):
    h = prepared(k)[4]
    whole = _run(k, (0, NE))
    want_nxt, want_neg = state_before(k, NE)
    assert np.array_equal(bits(whole[1]), bits(want_nxt)), "next after the run differs from the float32 restatement"
    assert np.array_equal(bits(whole[2]), bits(want_neg)), "next_neg after the run differs from the float32 restatement"
    assert np.isfinite(whole[0]).all() and np.abs(whole[0] - h["y0"]).max() > 1e-3
    for other, what in ((_run(k, (0, 20, NE)), "[0, 20) then [20, 66)"), (_run(k, (0, 0, 1, 65, NE, NE)), "five ranges, two empty"),
                        (_run(k, (0, NE), 8), "group 8"), (_run(k, (0, NE), 64), "group 64")):
        for x, y, name in zip(whole, other, ("y", "next", "next_neg")):
            assert np.array_equal(bits(x), bits(y)), f"{what}: {name} differs from the single launch"
    moved = _run(k, (0, NE), row_offset=1)
    assert np.array_equal(bits(moved[1]), bits(whole[1])) and not np.array_equal(bits(moved[0]), bits(whole[0]))


# ----------------------------------------------------------------------------------------------------------- independence
def test_a_row_does_not_depend_on_the_rest_of_the_call():
    from dynamorph_amd import umap_layout as U
    X, Q, y_train, idx, dist = fixture()
    m = U.UMAPEmbedding(n_neighbors=15, seed=SEED)
    m.embedding_, m.n_epochs_, m._X = y_train, 200, X                   # n_epochs_ // 3 = 66
    whole = m.transform(Q)
    init = m.init_t_.copy()
    assert whole.shape == (70, 2) and whole.dtype == np.float32 and np.isfinite(whole).all()
    assert m.sigma_t_.shape == (70,) and init.shape == (70, 2)
    parts = np.concatenate([m.transform(Q[:37]), m.transform(Q[37:], row_offset=37)])
    assert np.array_equal(bits(whole), bits(parts)), "two calls with row_offset differ from one"
    assert np.array_equal(bits(m.transform(Q, chunk_rows=16)), bits(whole)), "chunk_rows changes the result"
    assert np.array_equal(bits(m.init_t_), bits(init))
    assert np.array_equal(bits(m.transform(torch.from_numpy(Q).cuda())), bits(whole)), "a second run (device Q) differs"
    assert np.array_equal(bits(init[2]), bits(init[3])) and not np.array_equal(bits(whole[2]), bits(whole[3]))
    assert np.array_equal(bits(m.transform_graph(idx[:, :15], dist[:, :15])), bits(whole))
    assert np.array_equal(bits(whole), bits(_run(15, (0, NE))[0]))      # the kernels as the tests above drive them
    assert not np.array_equal(bits(m.transform(Q, seed=SEED + 1)), bits(whole))
    m.transform_group = 64
    assert np.array_equal(bits(m.transform(Q)), bits(whole))
    r = pickle.loads(pickle.dumps(m, protocol=4))                        # the host state, moved to the device on first use
    assert isinstance(r._X, np.ndarray) and np.array_equal(bits(r.transform(Q)), bits(whole))


# --------------------------------------------------------------------------------------------------------------- quality
def test_quality_held_out_blobs():
    """Fit on 800 rows of the blobs, place the 200 held out (every fifth row).  The figure: the share of a placed point's 10
    nearest training points in 2-D that carry its label, for the device's result and for the restatement's initial positions
    y0 (the weighted mean of the neighbours), which the layout must not make worse by more than 0.02."""
    from dynamorph_amd import umap_layout as U
    X, labels = UR.blobs()
    held = np.arange(1000) % 5 == 0
    Xtr, Xte, ltr, lte = X[~held], X[held], labels[~held], labels[held]
    m = U.UMAPEmbedding(n_neighbors=15, n_epochs=200)
    Ytr = m.fit_transform(Xtr)
    Yte = m.transform(Xte)
    assert Yte.shape == (200, 2) and np.isfinite(Yte).all()
    idx, dist = TR.query_knn_float64(Xtr, Xte, 15)
    y0 = TR.prepare(idx, dist, Ytr, 66)["y0"]
    share_dev = TR.label_share_against_training(Yte, lte, Ytr, ltr, 10)
    share_y0 = TR.label_share_against_training(y0, lte, Ytr, ltr, 10)
    print(f"held-out blobs: {share_dev:.4f} of the 10 nearest training points share the label (device), {share_y0:.4f} (y0); "
          f"largest |init_t_ - y0| {np.abs(m.init_t_ - y0).max():.2e}; mean move {np.abs(Yte - y0).mean():.3f}")
    assert share_dev >= share_y0 - 0.02


# -------------------------------------------------------------------------------------------------------------- pipeline
def test_pipeline(tmp_path):
    from dynamorph_amd import dim_reduction as DR
    from dynamorph_amd import umap_layout as U
    rng = np.random.default_rng(21)
    dirs, sizes = [], (120, 90, 130)
    for w, n in enumerate(sizes):
        d = tmp_path / f"well{w}"
        d.mkdir()
        with open(d / "p_latent_space_after.pkl", "wb") as f:
            pickle.dump(rng.standard_normal((n, 32)).astype(np.float32) + w, f, protocol=4)
        dirs.append(str(d))
    wdir = tmp_path / "weights"
    out = DR.dim_reduction_umap_embedding(dirs[:2], str(wdir), "p", n_nbrs=(15, 50), n_epochs=60, seed=2, save_models=True)
    assert sorted(os.listdir(wdir)) == ["embedding_umap_nbr15_a1.58_b0.9.pkl", "embedding_umap_nbr50_a1.58_b0.9.pkl", "knn_nbr15.pkl",
                                        "knn_nbr50.pkl", "umap_model_nbr15_a1.58_b0.9.pkl", "umap_model_nbr50_a1.58_b0.9.pkl"]
    with open(wdir / "umap_model_nbr15_a1.58_b0.9.pkl", "rb") as f:
        model = pickle.load(f)
    pooled, _ = DR.pool_latents(dirs[:2], "p")
    assert isinstance(model, U.UMAPEmbedding) and isinstance(model._X, np.ndarray) and np.array_equal(model._X, pooled)
    assert np.array_equal(bits(model.embedding_), bits(out[(15, 1.58, 0.9)])) and model.n_epochs_ == 60 and model.seed == 2
    with open(dirs[2] + "/p_latent_space_after.pkl", "rb") as f:
        well = pickle.load(f)
    want = model.transform(well)
    assert want.shape == (130, 2) and np.isfinite(want).all()
    odir = tmp_path / "out"
    res = DR.umap_transform(dirs[2], str(odir), str(wdir), "p")
    assert sorted(os.listdir(odir)) == ["p_latent_space_after_umap_model_nbr15_a1.58_b0.9.pkl",
                                        "p_latent_space_after_umap_model_nbr50_a1.58_b0.9.pkl"]
    with open(odir / "p_latent_space_after_umap_model_nbr15_a1.58_b0.9.pkl", "rb") as f:
        got = pickle.load(f)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(res["umap_model_nbr15_a1.58_b0.9"]), bits(want))
    odirs = [str(tmp_path / "o0"), str(tmp_path / "o2")]
    all_res = DR.dim_reduction_umap_transform([dirs[0], dirs[2]], odirs, str(wdir), "p")
    assert len(all_res) == 2 and np.array_equal(bits(all_res[1]["umap_model_nbr15_a1.58_b0.9"]), bits(want))
    with open(os.path.join(odirs[1], "p_latent_space_after_umap_model_nbr50_a1.58_b0.9.pkl"), "rb") as f:
        got50 = pickle.load(f)
    assert got50.shape == (130, 2) and not np.array_equal(got50, want)
