// score.hip -- per-patch losses and code usage (dynamorph_amd.patch_vae.score_patches).
//
// Reference: what model.forward(sample) returns for ONE patch (HiddenStateExtractor/vq_vae.py:300-338, vae.py:430-470;
// plot_scripts/recon_loss.py loops it over 5000 single patches): recon_loss (:320-323), the quantiser's loss and perplexity
// (:150-176) taken over that patch alone.  The batched loss kernels keep one partial sum per persistent workgroup and one
// histogram per call: both mix patches.  Here every sum belongs to one patch and is taken in an order that depends on the
// patch's own shape only -- one workgroup per (patch, channel) plane or per patch, a thread's elements in index order, the
// threads of a wave by butterfly, the four waves in wave order -- so a patch's values are the same to the bit whatever the
// batch size, its place in the batch and its neighbours.  No float atomics; the code counters are integer LDS atomics.
// (The fused decoder tail has its own per-patch form: dm_dec_tail_score in dec_tail.hip.)
#include "dm_common.h"

namespace {

constexpr int SC_MAX_GRID = 4096;
constexpr int SC_WINDOW = 4096;          // code counters a workgroup keeps in LDS at a time (16 KB); larger codebooks walk windows

// patch_sums[b][c] = sum over the plane of (dec*m - x*m)^2 / var[c]: dm_recon_loss's arithmetic per element.  VEC: H*W is a
// multiple of 4 (planes are 16-byte aligned): four pixels per load.
template <bool VEC>
__global__ __launch_bounds__(DM_BLOCK)
void recon_loss_per_sample_kernel(const float *__restrict__ dec, const float *__restrict__ x, const float *__restrict__ mask,
                                  int MC, const float *__restrict__ cvar, double *__restrict__ patch_sums, int NIN, int HW,
                                  long long nplanes)
{
    __shared__ double s_red[4];
    for (long long plane = blockIdx.x; plane < nplanes; plane += gridDim.x) {
        const long long b = plane / NIN;
        const int c = (int)(plane - b * NIN);
        const float v = cvar[c];
        const float *__restrict__ dp = dec + plane * HW, *__restrict__ xp = x + plane * HW;
        const float *__restrict__ mp = mask ? mask + (b * MC + (MC == 1 ? 0 : c)) * HW : nullptr;
        double loss = 0.0;
        if constexpr (VEC) {
            for (int p = threadIdx.x; p < HW / 4; p += DM_BLOCK) {
                const f32x4 o = *reinterpret_cast<const f32x4 *>(dp + 4 * p);
                const f32x4 xv = *reinterpret_cast<const f32x4 *>(xp + 4 * p);
                f32x4 t = o - xv;
                if (mp) {
                    const f32x4 mv = *reinterpret_cast<const f32x4 *>(mp + 4 * p);
                    t = o * mv - xv * mv;
                }
                const f32x4 sq = t * t;
                loss += (double)(sq.x / v) + (double)(sq.y / v) + (double)(sq.z / v) + (double)(sq.w / v);
            }
        } else {
            for (int p = threadIdx.x; p < HW; p += DM_BLOCK) {
                const float o = dp[p], xv = xp[p];
                float t = o - xv;
                if (mp) {
                    const float mv = mp[p];
                    t = o * mv - xv * mv;
                }
                const float sq = t * t;
                loss += (double)(sq / v);
            }
        }
        const double tot = block_sum(loss, s_red);
        if (threadIdx.x == 0) patch_sums[plane] = tot;
    }
}

// One workgroup per patch: scalars[b] = (loss, perplexity, mse) of vq_finalize_kernel's arithmetic over the patch's own
// H*W positions, counts[b][k] on request.  q = codebook[idx] is gathered (K*D floats: cache-resident), z is read once.
// EMA: the loss of the EMA codebook mode, cc * mse (no q_latent_loss term).
template <bool EMA = false>
__global__ __launch_bounds__(DM_BLOCK)
void vq_patch_scalars_kernel(const float *__restrict__ z, const long long *__restrict__ idx, const float *__restrict__ cb,
                             float cc, float *__restrict__ scalars, int *__restrict__ counts, int B, int D, int K, int HW)
{
#pragma clang fp contract(off)       // vq.hip is built without contraction: mse + cc * mse is a product and a sum there
    __shared__ double s_red[4];
    __shared__ int s_cnt[SC_WINDOW];
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const long long *__restrict__ ip = idx + (long long)b * HW;
        const float *__restrict__ zp = z + (long long)b * D * HW;
        double sse = 0.0;
        for (int p = threadIdx.x; p < HW; p += DM_BLOCK) {
            long long k = ip[p];
            k = k < 0 ? 0 : (k >= K ? K - 1 : k);
            const float *__restrict__ q = cb + k * D;
            for (int d = 0; d < D; ++d) {
                const float df = q[d] - zp[(long long)d * HW + p];
                sse += (double)df * (double)df;
            }
        }
        double e = 0.0;
        for (int k0 = 0; k0 < K; k0 += SC_WINDOW) {
            const int kn = K - k0 < SC_WINDOW ? K - k0 : SC_WINDOW;
            __syncthreads();                                    // the previous window (or patch) is done with s_cnt
            for (int k = threadIdx.x; k < kn; k += DM_BLOCK) s_cnt[k] = 0;
            __syncthreads();
            for (int p = threadIdx.x; p < HW; p += DM_BLOCK) {
                long long k = ip[p];
                k = k < 0 ? 0 : (k >= K ? K - 1 : k);
                if (k >= k0 && k < k0 + kn) atomicAdd(&s_cnt[(int)k - k0], 1);
            }
            __syncthreads();
            for (int k = threadIdx.x; k < kn; k += DM_BLOCK) {
                const int cnt = s_cnt[k];
                const float pk = (float)cnt / (float)HW;
                e += (double)(pk * logf(pk + 1e-10f));
                if (counts) counts[(long long)b * K + k0 + k] = cnt;
            }
        }
        const double tsse = block_sum(sse, s_red);
        const double ent = block_sum(e, s_red);
        if (threadIdx.x == 0) {
            const float mse = (float)(tsse / ((double)HW * (double)D));
            scalars[3 * b + 0] = EMA ? cc * mse : mse + cc * mse;
            scalars[3 * b + 1] = expf(-(float)ent);
            scalars[3 * b + 2] = mse;
        }
    }
}

// out[b] = (recon, commitment, total, perplexity, recon per channel): recon from the SAME double sums as the channels'
// values, rounded to float once.
__global__ __launch_bounds__(DM_BLOCK)
void score_finalize_kernel(const double *__restrict__ patch_sums, const float *__restrict__ vq_scalars, float w_recon,
                           float w_commit, long long chw, float *__restrict__ out, int B, int NIN)
{
    const int b = blockIdx.x * DM_BLOCK + threadIdx.x;
    if (b >= B) return;
    const double hw = (double)(chw / NIN);
    float *__restrict__ o = out + (long long)b * (4 + NIN);
    double tot = 0.0;
    for (int c = 0; c < NIN; ++c) {
        const double s = patch_sums[(long long)b * NIN + c];
        tot += s;
        o[4 + c] = (float)(s / hw);
    }
    const float recon = (float)(tot / (double)chw);
    const float commit = vq_scalars[3 * b + 0];
    o[0] = recon;
    o[1] = commit;
    o[2] = w_recon * recon + w_commit * commit;
    o[3] = vq_scalars[3 * b + 1];
}

}  // namespace

extern "C" int dm_recon_loss_per_sample(const float *decoded, const float *x, const float *mask, int mask_channels,
                                        const float *channel_var, double *patch_sums, int B, int NIN, int H, int W,
                                        void *stream)
{
    DM_REQUIRE(decoded && x && channel_var && patch_sums, "dm_recon_loss_per_sample: NULL pointer");
    DM_REQUIRE(B > 0 && NIN > 0 && H > 0 && W > 0, "dm_recon_loss_per_sample: bad shape (%d, %d, %d, %d)", B, NIN, H, W);
    DM_REQUIRE(!mask || mask_channels == 1 || mask_channels == NIN, "dm_recon_loss_per_sample: mask channels %d", mask_channels);
    DM_REQUIRE((long long)H * W < (1LL << 31), "dm_recon_loss_per_sample: plane too large for 32-bit offsets");
    const long long nplanes = (long long)B * NIN;
    const int HW = H * W, grid = (int)(nplanes < SC_MAX_GRID ? nplanes : SC_MAX_GRID);
    hipStream_t st = (hipStream_t)stream;
    if (HW % 4 == 0)
        hipLaunchKernelGGL(recon_loss_per_sample_kernel<true>, dim3(grid), dim3(DM_BLOCK), 0, st, decoded, x, mask, mask_channels,
                           channel_var, patch_sums, NIN, HW, nplanes);
    else
        hipLaunchKernelGGL(recon_loss_per_sample_kernel<false>, dim3(grid), dim3(DM_BLOCK), 0, st, decoded, x, mask, mask_channels,
                           channel_var, patch_sums, NIN, HW, nplanes);
    return dm_launch_status("dm_recon_loss_per_sample");
}

extern "C" int dm_vq_patch_scalars(const float *z, const int64_t *idx, const float *codebook, float commitment_cost,
                                   float *scalars, int32_t *counts, int B, int D, int K, int H, int W, void *stream)
{
    DM_REQUIRE(z && idx && codebook && scalars, "dm_vq_patch_scalars: NULL pointer");
    DM_REQUIRE(B > 0 && D > 0 && K > 0 && H > 0 && W > 0, "dm_vq_patch_scalars: bad shape (%d, %d, %d, %d, %d)", B, D, K, H, W);
    DM_REQUIRE((long long)H * W < (1LL << 31), "dm_vq_patch_scalars: latent too large for 32-bit offsets");
    hipLaunchKernelGGL(vq_patch_scalars_kernel<>, dim3(B < SC_MAX_GRID ? B : SC_MAX_GRID), dim3(DM_BLOCK), 0, (hipStream_t)stream,
                       z, reinterpret_cast<const long long *>(idx), codebook, commitment_cost, scalars, counts, B, D, K, H * W);
    return dm_launch_status("dm_vq_patch_scalars");
}

extern "C" int dm_vq_patch_scalars_ema(const float *z, const int64_t *idx, const float *codebook, float commitment_cost,
                                       float *scalars, int32_t *counts, int B, int D, int K, int H, int W, void *stream)
{
    DM_REQUIRE(z && idx && codebook && scalars, "dm_vq_patch_scalars_ema: NULL pointer");
    DM_REQUIRE(B > 0 && D > 0 && K > 0 && H > 0 && W > 0, "dm_vq_patch_scalars_ema: bad shape (%d, %d, %d, %d, %d)", B, D, K, H, W);
    DM_REQUIRE((long long)H * W < (1LL << 31), "dm_vq_patch_scalars_ema: latent too large for 32-bit offsets");
    hipLaunchKernelGGL(vq_patch_scalars_kernel<true>, dim3(B < SC_MAX_GRID ? B : SC_MAX_GRID), dim3(DM_BLOCK), 0,
                       (hipStream_t)stream, z, reinterpret_cast<const long long *>(idx), codebook, commitment_cost, scalars,
                       counts, B, D, K, H * W);
    return dm_launch_status("dm_vq_patch_scalars_ema");
}

extern "C" int dm_score_finalize(const double *patch_sums, const float *vq_scalars, float weight_recon,
                                 float weight_commitment, int64_t chw, float *out, int B, int NIN, void *stream)
{
    DM_REQUIRE(patch_sums && vq_scalars && out, "dm_score_finalize: NULL pointer");
    DM_REQUIRE(B > 0 && NIN > 0 && chw > 0 && chw % NIN == 0, "dm_score_finalize: bad argument");
    hipLaunchKernelGGL(score_finalize_kernel, dim3((B + DM_BLOCK - 1) / DM_BLOCK), dim3(DM_BLOCK), 0, (hipStream_t)stream,
                       patch_sums, vq_scalars, weight_recon, weight_commitment, (long long)chw, out, B, NIN);
    return dm_launch_status("dm_score_finalize");
}
