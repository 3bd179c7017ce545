#!/usr/bin/env python3
"""Golden fixture for the latent PCA: tests/golden/g13_pca.npz.

The reference's call, sklearn.decomposition.PCA(0.5, svd_solver='auto') (run_dim_reduction.py:33), on planted-spectrum
latents (tests/helpers/pca_fixture.py) of N = 3000 rows and F = 4096 / 1000 features: once on the float32 data (what the
reference produces) and once on a float64 copy (the tight yardstick).  Only the recipe, the checksum of X, the fitted
attributes, the solver scikit-learn picked and the transform of the first 64 rows are stored.

    python3 tests/golden/make_golden_pca.py
"""
import os
import sys

import numpy as np
from sklearn.decomposition import PCA

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
from pca_fixture import checksum, make_x, recipe  # noqa: E402

ATTRS = ("mean_", "components_", "explained_variance_", "explained_variance_ratio_", "singular_values_", "noise_variance_",
         "n_components_")


def main():
    out = {}
    for tag, F, seed in (("f4096", 4096, 13), ("f1000", 1000, 14)):
        rec = recipe(3000, F, seed)
        X = make_x(rec)
        for k, v in rec.items():
            out[f"{tag}_recipe_{k}"] = np.asarray(v)
        out[f"{tag}_sha256"] = np.array(checksum(X))
        for prec, data in (("f32", X.astype(np.float32)), ("f64", X)):
            pca = PCA(0.5, svd_solver='auto')
            pca.fit(data)
            for a in ATTRS:
                out[f"{tag}_{prec}_{a}"] = np.asarray(getattr(pca, a))
            out[f"{tag}_{prec}_solver"] = np.array(pca._fit_svd_solver)
            out[f"{tag}_{prec}_transform64"] = pca.transform(data[:64])
            # every cumulative ratio of the float64 fit, for the check below
            if prec == "f64":
                full = PCA(None, svd_solver='full').fit(X)
                cum = np.cumsum(full.explained_variance_ratio_)
                gap = np.abs(cum - 0.5).min()
                assert gap >= 1e-3, (tag, gap)
                out[f"{tag}_f64_boundary_gap"] = np.array(gap)
            print(tag, prec, pca._fit_svd_solver, pca.n_components_, flush=True)
    np.savez_compressed(os.path.join(HERE, "g13_pca.npz"), **out)


if __name__ == "__main__":
    main()
