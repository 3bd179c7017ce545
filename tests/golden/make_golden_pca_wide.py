#!/usr/bin/env python3
"""Golden fixture for the sample-space ("wide") latent PCA: tests/golden/g17_pca_wide.npz.

The reference's call, sklearn.decomposition.PCA(0.5, svd_solver='auto') (run_dim_reduction.py:33), on planted-spectrum
latents (tests/helpers/pca_fixture.py) wider than the covariance route takes:
    f16385   257 x 16385: one feature above DM_PCA_MAX_FEATURES, odd (the scalar-load form), N no multiple of the tile
    f65536   130 x 65536: the width of the VQ_VAE_z32 latents
Stored: the recipe, the checksum of X, the fitted attributes of the float64 fit (components_ rounded to float32, which keeps
the file below 1 MiB and costs 1e-14 of cosine; f65536 without components_), n_components_ and the solver of the float32
fit, and the float64 fit's transform of the first 64 rows.

    python3 tests/golden/make_golden_pca_wide.py
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
    for tag, N, F, seed in (("f16385", 257, 16385, 18), ("f65536", 130, 65536, 19)):
        rec = recipe(N, F, seed)
        X = make_x(rec)
        for k, v in rec.items():
            out[f"{tag}_recipe_{k}"] = np.asarray(v)
        out[f"{tag}_sha256"] = np.array(checksum(X))
        pca = PCA(0.5, svd_solver='auto').fit(X)
        for a in ATTRS:
            v = np.asarray(getattr(pca, a))
            if a == "components_":
                if tag == "f65536":
                    continue
                v = v.astype(np.float32)
            out[f"{tag}_f64_{a}"] = v
        out[f"{tag}_f64_solver"] = np.array(pca._fit_svd_solver)
        out[f"{tag}_f64_transform64"] = pca.transform(X[:64])
        p32 = PCA(0.5, svd_solver='auto').fit(X.astype(np.float32))
        out[f"{tag}_f32_n_components_"] = np.asarray(p32.n_components_)
        out[f"{tag}_f32_solver"] = np.array(p32._fit_svd_solver)
        # every cumulative ratio of the float64 fit: the 0.5 boundary is not a matter of rounding
        cum = np.cumsum(PCA(None, svd_solver='full').fit(X).explained_variance_ratio_)
        gap = np.abs(cum - 0.5).min()
        assert gap >= 1e-3, (tag, gap)
        out[f"{tag}_f64_boundary_gap"] = np.array(gap)
        print(tag, pca._fit_svd_solver, pca.n_components_, p32._fit_svd_solver, p32.n_components_, gap, flush=True)
    np.savez_compressed(os.path.join(HERE, "g17_pca_wide.npz"), **out)


if __name__ == "__main__":
    main()
