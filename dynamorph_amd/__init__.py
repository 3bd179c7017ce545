"""dynamorph_amd -- MI355X-native VQ-VAE latent-encoding path of mehta-lab/dynamorph.

Public surface = the reference's module surface for this path:
    VQ_VAE, VQ_VAE_z16, VQ_VAE_z32, VectorQuantizer, ResidualBlock      (dynamorph_amd.vq_vae)
computed by hand-written gfx950 HIP kernels behind the C ABI in include/dynamorph_hip.h, and the per-patch scoring drivers
of the inference path:
    score_patches, score_patches_sharded, score_VAE                     (dynamorph_amd.patch_vae)
    patch_gradients, patch_gradients_sharded                            (dynamorph_amd.patch_vae)
and the clustering of the latents behind them (sklearn.cluster.KMeans of the reference's clustering scripts):
    KMeans                                                              (dynamorph_amd.kmeans)
and how faithful an embedding of the latents is (sklearn.manifold.trustworthiness at any N, and its converse):
    trustworthiness, continuity, embedding_quality                      (dynamorph_amd.quality)
"""
from .vq_vae import VQ_VAE, VQ_VAE_z16, VQ_VAE_z32, VectorQuantizer, ResidualBlock  # noqa: F401
from .patch_vae import score_patches, score_patches_sharded, score_VAE, patch_gradients, patch_gradients_sharded  # noqa: F401
from .kmeans import KMeans  # noqa: F401
from .quality import trustworthiness, continuity, embedding_quality  # noqa: F401

__all__ = ["VQ_VAE", "VQ_VAE_z16", "VQ_VAE_z32", "VectorQuantizer", "ResidualBlock",
           "score_patches", "score_patches_sharded", "score_VAE", "patch_gradients", "patch_gradients_sharded", "KMeans",
           "trustworthiness", "continuity", "embedding_quality"]
