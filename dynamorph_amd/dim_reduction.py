"""PCA stage of the pipeline: mirror of run_dim_reduction.py (fit_PCA lines 14-50, process_PCA 52-92, the PCA branch of
dim_reduction 177-281) on dynamorph_amd.pca.PCA / WidePCA; and its UMAP stage: fit_umap (143-207) and umap_transform (94-127) on
dynamorph_amd.umap_layout.UMAPEmbedding; and the clustering of the reduced latents (HiddenStateExtractor/deprecated/
morphology_clustering.py:103-141) on dynamorph_amd.kmeans.KMeans.

File names are the ones process_VAE writes: <prefix>_latent_space<suffix>.pkl in, <prefix>_latent_space<suffix>_PCAed.pkl
out (the reference's '{}_latent_space_{}.pkl'.format(prefix, '_after') names a '..._latent_space__after.pkl' its own pipeline
never writes).
"""
import os
import pickle

import numpy as np

from . import knn as _knn
from .pca import MAX_FEATURES, PCA, WidePCA


def _sklearn_available():
    try:
        import sklearn.decomposition  # noqa: F401
    except ImportError:
        return False
    return True


def fit_PCA(train_data, weights_dir, labels=None, conditions=None, n_components=0.5, **kw):
    """Fit PCA(n_components) to the pooled latents, write <weights_dir>/pca_model.pkl (protocol 4) and return the fitted
    device PCA (WidePCA, the sample-space route, when the latents have more than MAX_FEATURES columns: the VQ_VAE_z32
    latents).  The pickle holds the fitted sklearn PCA when scikit-learn is importable (what the reference's
    process_PCA unpickles), else this package's PCA with its state on the host.  PCA.png is drawn when matplotlib imports."""
    os.makedirs(weights_dir, exist_ok=True)
    model_path = os.path.join(weights_dir, 'pca_model.pkl')
    wide = np.ndim(train_data) == 2 and np.shape(train_data)[1] > MAX_FEATURES
    pca = (WidePCA if wide else PCA)(n_components, **kw)
    pcas = pca.fit_transform(train_data)
    with open(model_path, 'wb') as f:
        pickle.dump(pca.to_sklearn() if _sklearn_available() else pca, f, protocol=4)
    _scatter(pcas, labels, conditions, weights_dir)
    return pca


def _scatter(pcas, labels, conditions, weights_dir, zoom_cutoff=1):
    """run_dim_reduction.py:39-49: PC 1 against PC 2, coloured by label."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        return
    if pcas.shape[1] < 2:
        return
    p = pcas[:, :2].cpu().numpy()
    fig, ax = plt.subplots()
    scatter = ax.scatter(p[:, 0], p[:, 1], s=7, c=labels, cmap='Paired', alpha=0.1)
    scatter.set_facecolor("none")
    ax.set_xlim(np.percentile(p[:, 0], zoom_cutoff), np.percentile(p[:, 0], 100 - zoom_cutoff))
    ax.set_ylim(np.percentile(p[:, 1], zoom_cutoff), np.percentile(p[:, 1], 100 - zoom_cutoff))
    if labels is not None and conditions is not None:
        ax.legend(handles=scatter.legend_elements()[0], loc="upper right", title="condition", labels=conditions)
    ax.set_xlabel('PC 1')
    ax.set_ylabel('PC 2')
    fig.savefig(os.path.join(weights_dir, 'PCA.png'), dpi=300)
    plt.close(fig)


def load_model(weights_dir, device=None):
    """<weights_dir>/pca_model.pkl -- a fitted sklearn PCA (this package's or the reference's) or this package's PCA -- as a
    device PCA."""
    model_path = os.path.join(weights_dir, 'pca_model.pkl')
    try:
        with open(model_path, 'rb') as f:
            obj = pickle.load(f)
    except Exception as ex:
        raise ValueError("Error in loading pre-saved PCA weights") from ex
    if isinstance(obj, PCA):
        return obj
    return (WidePCA if int(obj.n_features_in_) > MAX_FEATURES else PCA).from_sklearn(obj, device=device)


def process_PCA(input_dir, output_dir, weights_dir, prefix, suffix='_after', pca=None):
    """<input_dir>/<prefix>_latent_space<suffix>.pkl -> <output_dir>/<prefix>_latent_space<suffix>_PCAed.pkl (float32,
    protocol 4), transformed on the GPU by the model in <weights_dir> (or `pca`)."""
    os.makedirs(output_dir, exist_ok=True)
    if pca is None:
        pca = load_model(weights_dir)
    with open(os.path.join(input_dir, '{}_latent_space{}.pkl'.format(prefix, suffix)), 'rb') as f:
        dats = pickle.load(f)
    dats_ = pca.transform(np.asarray(dats)).cpu().numpy()
    with open(os.path.join(output_dir, '{}_latent_space{}_PCAed.pkl'.format(prefix, suffix)), 'wb') as f:
        pickle.dump(dats_, f, protocol=4)
    return dats_


def _prefix_list(prefixes):
    if isinstance(prefixes, str):
        prefixes = [prefixes]
    if not prefixes:
        raise ValueError("latent space vector file name must contain a prefix: '<prefix>_latent_space.pkl'")
    return prefixes


def pool_latents(input_dirs, prefixes):
    """The training matrix of run_dim_reduction.py::dim_reduction (fit_model): <prefix>_latent_space_after.pkl of every directory and prefix, in that order, stacked;
    one label per file.  Returns (vectors (N, F), labels)."""
    vectors, labels = [], []
    for label, (d, p) in enumerate((d, p) for d in input_dirs for p in _prefix_list(prefixes)):
        with open(os.path.join(d, '{}_latent_space_after.pkl'.format(p)), 'rb') as f:
            vec = pickle.load(f)
        vectors.append(np.asarray(vec))
        labels += [label] * vec.shape[0]
    return np.concatenate(vectors, axis=0), labels


def dim_reduction_pca(input_dirs, output_dirs, weights_dir, prefixes, fit_model, conditions=None, **kw):
    """The PCA branch of run_dim_reduction.py::dim_reduction.  fit_model: pool <prefix>_latent_space_after.pkl of every
    directory and prefix, in that order, one label per file, and fit (returns the PCA); else transform every (directory,
    prefix) with the saved model (returns the list of outputs)."""
    prefixes = _prefix_list(prefixes)
    if conditions is None:
        conditions = [os.path.basename(d) for d in input_dirs]
    if fit_model:
        weights_output = os.path.dirname(weights_dir) if os.path.isfile(weights_dir) else weights_dir
        vectors, labels = pool_latents(input_dirs, prefixes)
        return fit_PCA(vectors, weights_output, labels=labels, conditions=conditions, **kw)
    pca = load_model(weights_dir)
    return [process_PCA(d, o, weights_dir, p, pca=pca) for d, o in zip(input_dirs, output_dirs) for p in prefixes]


def fit_knn(train_data, weights_dir, n_nbrs=(15, 50, 200), **kw):
    """The neighbour graphs fit_umap's three umap.UMAP(n_neighbors=n) fits start from (run_dim_reduction.py:143-207): ONE
    exact graph at max(n_nbrs) with the row itself in column 0, written as <weights_dir>/knn_nbr<n>.pkl (protocol 4,
    [knn_indices int64, knn_dists float32]) for every n -- the first n columns of that graph, which is sorted.  Returns
    {n: (knn_indices, knn_dists)}.  umap.UMAP(n_neighbors=n, precomputed_knn=tuple(pickle.load(f))) takes a file as it is.
    More than MAX_FEATURES columns (the VQ_VAE_z32 latents): knn.wide_knn_graph, at most knn.WIDE_MAX_ROWS rows; kw goes to it
    (gram=(mean, s, K) hands it a row Gram matrix that exists already)."""
    n_nbrs = sorted(set(int(n) for n in n_nbrs))
    if not n_nbrs or n_nbrs[0] < 1:
        raise ValueError(f"n_nbrs={n_nbrs!r}: need at least one neighbour count >= 1")
    os.makedirs(weights_dir, exist_ok=True)
    if _knn.is_wide(train_data):
        indices, dists = _knn.wide_knn_graph(train_data, n_nbrs[-1], include_self=True, **kw)
    else:
        indices, dists = _knn.knn_graph(train_data, n_nbrs[-1], include_self=True, **kw)
    out = {}
    for n in n_nbrs:
        out[n] = (np.ascontiguousarray(indices[:, :n]), np.ascontiguousarray(dists[:, :n]))
        with open(os.path.join(weights_dir, 'knn_nbr{}.pkl'.format(n)), 'wb') as f:
            pickle.dump([out[n][0], out[n][1]], f, protocol=4)
    return out


def dim_reduction_knn(input_dirs, weights_dir, prefixes, n_nbrs=(15, 50, 200), **kw):
    """The pooling of the UMAP branch of run_dim_reduction.py::dim_reduction (fit_model=True), followed by fit_knn: the same
    files in the same order as dim_reduction_pca pools them, so row i of the graph is row i of the PCA's training matrix."""
    weights_output = os.path.dirname(weights_dir) if os.path.isfile(weights_dir) else weights_dir
    vectors, _ = pool_latents(input_dirs, prefixes)
    return fit_knn(vectors, weights_output, n_nbrs=n_nbrs, **kw)


def fit_umap_embedding(train_data, weights_dir, labels=None, n_nbrs=(15, 50, 200), a_s=(1.58,), b_s=(0.9,), save_models=False,
                       **kw):
    """fit_umap of run_dim_reduction.py:143-207 without umap-learn: ONE exact graph at max(n_nbrs) through fit_knn (the
    knn_nbr<n>.pkl files are still written), then one embedding per (n, a, b) from its first n columns by
    umap_layout.UMAPEmbedding, written as <weights_dir>/embedding_umap_nbr<n>_a<a>_b<b>.pkl
    (protocol 4, [embedding (N, 2) float32, labels]).  The name does not start with 'umap': the reference's umap_transform
    lists umap*.pkl there and calls .transform on what it unpickles.  save_models=True also writes the fitted UMAPEmbedding
    itself as <weights_dir>/umap_model_nbr<n>_a<a>_b<b>.pkl (protocol 4) -- a name that umap_transform, here and in the
    reference, does pick up; every such file carries the training matrix (N F 4 bytes: 5.2 GB for 20 000 VQ_VAE_z32 latents of
    65536 features).  kw: UMAPEmbedding's (n_epochs, negative_sample_rate, gamma, init, init_eigensolver, seed, device).  More than MAX_FEATURES
    columns: the wide route -- ONE row Gram matrix serves the graph's filter and the PCA initialisation.  Returns
    {(n, a, b): embedding}."""
    import torch
    from .umap_layout import UMAPEmbedding, pca_coordinates, wide_gram
    init = kw.pop("init", "pca")
    device = kw.get("device")
    solver = {"eigensolver": kw["init_eigensolver"]} if kw.get("init_eigensolver", "full") != "full" else {}
    if isinstance(init, str) and init != "pca":
        raise ValueError(f"init={init!r}: 'pca' or an (N, 2) array")
    wide = _knn.is_wide(train_data)
    x = _knn._resident(train_data, device)
    if wide and isinstance(init, str):
        with torch.no_grad(), torch.cuda.device(x.device):
            g = wide_gram(x, **solver)
        graphs = fit_knn(x, weights_dir, n_nbrs=n_nbrs, gram=g)
        init = pca_coordinates(x, gram=g, consume_gram=True, **solver).cpu().numpy()      # (the graph is done: K may be used up)
        del g
    else:
        graphs = fit_knn(x, weights_dir, n_nbrs=n_nbrs)
        if isinstance(init, str):
            init = pca_coordinates(x, **solver).cpu().numpy()
    out = {}
    keep = {"X": x} if save_models else {}          # only a model that is saved holds on to the training matrix
    for n in sorted(graphs):
        for a in a_s:
            for b in b_s:
                model = UMAPEmbedding(n_neighbors=n, a=a, b=b, **kw)
                model.fit_graph(graphs[n][0], graphs[n][1], init, **keep)
                emb = model.embedding_
                out[(n, a, b)] = emb
                with open(os.path.join(weights_dir, 'embedding_umap_nbr{}_a{}_b{}.pkl'.format(n, a, b)), 'wb') as f:
                    pickle.dump([emb, labels], f, protocol=4)
                if save_models:
                    with open(os.path.join(weights_dir, 'umap_model_nbr{}_a{}_b{}.pkl'.format(n, a, b)), 'wb') as f:
                        pickle.dump(model, f, protocol=4)
    return out


def dim_reduction_umap_embedding(input_dirs, weights_dir, prefixes, n_nbrs=(15, 50, 200), a_s=(1.58,), b_s=(0.9,), **kw):
    """The pooling of the UMAP branch of run_dim_reduction.py::dim_reduction (fit_model=True) -- the same files in the same
    order as dim_reduction_knn and dim_reduction_pca pool them, one label per file -- followed by fit_umap_embedding."""
    weights_output = os.path.dirname(weights_dir) if os.path.isfile(weights_dir) else weights_dir
    vectors, labels = pool_latents(input_dirs, prefixes)
    return fit_umap_embedding(vectors, weights_output, labels=labels, n_nbrs=n_nbrs, a_s=a_s, b_s=b_s, **kw)


def score_umap_embeddings(train_data, weights_dir, n_neighbors=15, **kw):
    """Which of fit_umap_embedding's embeddings is faithful to the latents: every <weights_dir>/embedding_umap_nbr*_a*_b*.pkl
    scored against train_data (the matrix they were fitted on, rows in the same order) in ONE quality.embedding_quality
    call.  Writes <weights_dir>/embedding_quality.pkl (protocol 4, a plain dict {file name without
    .pkl: {"trustworthiness", "continuity", "neighbor_recall"}}) and returns it.  kw: embedding_quality's (chunk_rows,
    device, shift, cap, x_graph)."""
    import fnmatch
    from .quality import embedding_quality
    embeddings = {}
    for fname in sorted(fnmatch.filter(os.listdir(weights_dir), 'embedding_umap_nbr*_a*_b*.pkl')):
        with open(os.path.join(weights_dir, fname), 'rb') as f:
            embeddings[os.path.splitext(fname)[0]] = np.asarray(pickle.load(f)[0], dtype=np.float32)
    if not embeddings:
        raise ValueError(f"no embedding_umap_nbr*_a*_b*.pkl in {weights_dir}: fit_umap_embedding writes them")
    scores = embedding_quality(train_data, embeddings, n_neighbors=n_neighbors, **kw)
    with open(os.path.join(weights_dir, 'embedding_quality.pkl'), 'wb') as f:
        pickle.dump(scores, f, protocol=4)
    return scores


def dim_reduction_score_umap_embeddings(input_dirs, weights_dir, prefixes, n_neighbors=15, **kw):
    """The pooling of dim_reduction_umap_embedding -- the same files in the same order, so row i of the pooled matrix is row
    i of every embedding -- followed by score_umap_embeddings."""
    weights_output = os.path.dirname(weights_dir) if os.path.isfile(weights_dir) else weights_dir
    vectors, _ = pool_latents(input_dirs, prefixes)
    return score_umap_embeddings(vectors, weights_output, n_neighbors=n_neighbors, **kw)


def load_umap_models(weights_dir):
    """{model name: model} of every umap*.pkl in weights_dir, in sorted order (run_dim_reduction.py:108-117).  A file that does
    not unpickle to an object with a transform method raises the reference's ValueError."""
    models = {}
    for fname in sorted(f for f in os.listdir(weights_dir) if f.startswith('umap') and f.endswith('.pkl')):
        try:
            with open(os.path.join(weights_dir, fname), 'rb') as f:
                model = pickle.load(f)
        except Exception as ex:
            raise ValueError("Error in loading pre-saved PCA weights") from ex
        if not callable(getattr(model, "transform", None)):
            raise ValueError("Error in loading pre-saved PCA weights")
        models[os.path.splitext(fname)[0]] = model
    return models


def umap_transform(input_dir, output_dir, weights_dir, prefix, suffix='_after', models=None):
    """umap_transform of run_dim_reduction.py:94-127: for every umap*.pkl model in weights_dir (or `models`, as
    load_umap_models returns them) <input_dir>/<prefix>_latent_space<suffix>.pkl -> <output_dir>/<prefix>_latent_space<suffix>_
    <model name>.pkl (float32, protocol 4), placed into the model's embedding on the GPU.  Returns {model name: array}."""
    os.makedirs(output_dir, exist_ok=True)
    if models is None:
        models = load_umap_models(weights_dir)
    with open(os.path.join(input_dir, '{}_latent_space{}.pkl'.format(prefix, suffix)), 'rb') as f:
        dats = pickle.load(f)
    out = {}
    for name, model in models.items():
        dats_ = np.asarray(model.transform(np.asarray(dats)), dtype=np.float32)
        with open(os.path.join(output_dir, '{}_latent_space{}_{}.pkl'.format(prefix, suffix, name)), 'wb') as f:
            pickle.dump(dats_, f, protocol=4)
        out[name] = dats_
    return out


def dim_reduction_umap_transform(input_dirs, output_dirs, weights_dir, prefixes):
    """The fit_model=False branch of run_dim_reduction.py::dim_reduction for UMAP (which the reference refuses): every
    (directory, prefix) through umap_transform with the models of weights_dir, loaded once.  Returns the list of its results."""
    prefixes = _prefix_list(prefixes)
    models = load_umap_models(weights_dir)
    return [umap_transform(d, o, weights_dir, p, models=models) for d, o in zip(input_dirs, output_dirs) for p in prefixes]


# ------------------------------------------------------------------ k-means of the reduced latents
def _sklearn_cluster_available():
    try:
        import sklearn.cluster  # noqa: F401
    except ImportError:
        return False
    return True


def fit_kmeans(train_data, weights_dir, n_clusters=4, **kw):
    """Fit KMeans(n_clusters) to the (PCA-ed) latents, write <weights_dir>/kmeans_model.pkl (protocol 4) and return the fitted
    device KMeans.  The pickle holds the fitted sklearn KMeans when scikit-learn is importable, else this package's KMeans, as
    fit_PCA does.  kw: KMeans's (init, n_init, max_iter, tol, seed, device)."""
    from .kmeans import KMeans
    os.makedirs(weights_dir, exist_ok=True)
    model = KMeans(n_clusters, **kw).fit(train_data)
    with open(os.path.join(weights_dir, 'kmeans_model.pkl'), 'wb') as f:
        pickle.dump(model.to_sklearn() if _sklearn_cluster_available() else model, f, protocol=4)
    return model


def load_kmeans_model(weights_dir, device=None):
    """<weights_dir>/kmeans_model.pkl -- a fitted sklearn KMeans or this package's KMeans -- as a device KMeans."""
    from .kmeans import KMeans
    try:
        with open(os.path.join(weights_dir, 'kmeans_model.pkl'), 'rb') as f:
            obj = pickle.load(f)
    except Exception as ex:
        raise ValueError("Error in loading pre-saved k-means weights") from ex
    return obj if isinstance(obj, KMeans) else KMeans.from_sklearn(obj, device=device)


def process_kmeans(input_dir, output_dir, weights_dir, prefix, suffix='_after_PCAed', model=None):
    """<input_dir>/<prefix>_latent_space<suffix>.pkl -> <output_dir>/<prefix>_latent_space<suffix>_clusters.pkl (int32 labels,
    protocol 4), labelled on the GPU by the model in <weights_dir> (or `model`)."""
    os.makedirs(output_dir, exist_ok=True)
    if model is None:
        model = load_kmeans_model(weights_dir)
    with open(os.path.join(input_dir, '{}_latent_space{}.pkl'.format(prefix, suffix)), 'rb') as f:
        dats = pickle.load(f)
    labels = np.asarray(model.predict(np.asarray(dats)), dtype=np.int32)
    with open(os.path.join(output_dir, '{}_latent_space{}_clusters.pkl'.format(prefix, suffix)), 'wb') as f:
        pickle.dump(labels, f, protocol=4)
    return labels


def trajectory_windows(vs, trajs, length=5, diffs=False):
    """generate_short_traj_morphorlogy over list(trajs.values()) (morphology_clustering.py:103-113): every window of `length`
    consecutive frames of every trajectory, in the reference's order, as one row of length * F descriptors -- or, diffs=True,
    the (length - 1) * F differences of consecutive frames (Kmean_on_short_traj_diffs).  trajs: {name: frame indices into vs}
    or a list of index lists; a trajectory shorter than `length` contributes nothing.  Returns (windows float32 (n, .),
    owners: the position of each window's trajectory in trajs, int64 (n,))."""
    vs = np.asarray(vs)
    if vs.ndim != 2:
        raise ValueError(f"vs has shape {vs.shape}, expected (frames, features)")
    length = int(length)
    if length < 1 or (diffs and length < 2):
        raise ValueError(f"length = {length}: at least 1 frame, 2 for differences")
    tlist = list(trajs.values()) if isinstance(trajs, dict) else list(trajs)
    starts, owners = [], []
    for o, t in enumerate(tlist):
        t = np.asarray(t, dtype=np.int64)
        n_sub = len(t) - (length - 1)
        for i in range(max(n_sub, 0)):
            starts.append(t[i:i + length])
            owners.append(o)
    F = vs.shape[1]
    if not starts:
        return np.zeros((0, (length - 1 if diffs else length) * F), np.float32), np.zeros(0, np.int64)
    w = vs[np.stack(starts, 0)]                                    # (n, length, F)
    if diffs:
        w = w[:, 1:] - w[:, :-1]
    return np.ascontiguousarray(w.reshape(len(starts), -1), dtype=np.float32), np.asarray(owners, np.int64)


def kmeans_on_short_trajs(vs, trajs, length=5, n_clusters=4, diffs=False, **kw):
    """Kmean_on_short_trajs / Kmean_on_short_traj_diffs (morphology_clustering.py:115-141): one KMeans(n_clusters) over the
    windows of all trajectories, then {trajectory: labels of its windows} (int32; an empty array for a trajectory shorter than
    `length`, where the reference's np.stack raises).  The labels of the fit ARE the prediction of the fitted centres for
    the same rows, so nothing is labelled twice."""
    from .kmeans import KMeans
    windows, owners = trajectory_windows(vs, trajs, length=length, diffs=diffs)
    labels = KMeans(n_clusters, **kw).fit(windows).labels_
    return {t: labels[owners == o].astype(np.int32) for o, t in enumerate(trajs)}
