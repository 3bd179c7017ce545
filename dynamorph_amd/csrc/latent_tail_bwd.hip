// latent_tail_bwd.hip -- the data-only backward of the 16 x 16 part of the encoder with per-sample BatchNorm statistics, one
// patch per workgroup pass: the mirror of latent_tail.hip.
//
// g_z (the gradient at the encoder's output) goes back through enc.12 (every residual layer: BatchNorm, 1x1, ReLU, BatchNorm,
// 3x3, ReLU, + skip), enc.11 (BatchNorm) and enc.10 (3x3) to dy3, the gradient at enc.7's raw output a3 masked by
// relu(BN3(a3)), with the patch's (sum dy3, sum dy3 * a3) for enc.8's backward.  engine.residual_backward / latent_stage_backward
// state the arithmetic; as separate launches it is one statistics launch, five finalisers and five data-gradient launches.
// Here the gradients never leave the CU; the tensors the forward pass saved (ra, rb, h_in, a4, a3) are read from HBM once or
// twice each: 16 (g_z) + per layer 2 * 32 + 2 * 16 + 16 (ra twice, rb twice, h_in) + 2 * 16 (a4) + 2 * 16 (a3) + 16 (dy3) KB
// = 320 KB per patch at two layers, against about 530 KB for the chain.
//   G  (16 ch, 256-float planes)             the gradient on the residual stream
//   P  (32 ch, zero-padded 18 x 24 planes)   a product's input: BatchNorm's backward da = c0 dy + (c1 a + c2) of the layer above
//   Y  (32 ch, 256-float planes)             a product's masked output, before its BatchNorm backward
//   W  (<= 4608 floats)                      the product's weights as B operands [tap][k][n], taps flipped
// Products are v_mfma_f32_16x16x4_f32 (exact fp32 chains): M = 16 positions of one row, N = 16 channels of the layer's INPUT,
// K = 4 channels of its output per step; a wave owns four rows.  The (sum dy, sum dy * a) of a BatchNorm: thread (channel
// t >> 4, row t & 15) adds its 16 positions in index order in double, the 16 rows by four DPP exchange steps in double -- one
// order whatever the batch; thread c then forms bn_backward_finalize_kernel's coefficients for channel c in double.
#include "dm_common.h"

namespace {

constexpr int LB_RS = 24, LB_PS = 18 * LB_RS;          // as latent_tail.hip's T: column x at j = x + 4, j = 3 / 20 zero
constexpr int LB_MAX_RES = 4;
constexpr int LB_G = 0, LB_P = LB_G + 16 * 256, LB_Y = LB_P + 32 * LB_PS, LB_W = LB_Y + 32 * 256, LB_FLOATS = LB_W + 32 * 16 * 9;

struct LbLayer {
    const float *ra, *rb, *h_in, *coefa, *saveda, *savedb, *ga, *gb, *wa, *wb;
};
struct LbParams {
    const float *g_z, *a3, *coef3, *a4, *saved4, *g4, *w10;
    float *dy3;
    double *st3;
    LbLayer l[LB_MAX_RES];
    int B, nres;
};

// (sum src, sum src * q) over the 256 positions of each of C channels -> s_sum[c][2].  src: LDS [C][256]; q: the patch's [C][256].
template <int C>
__device__ __forceinline__ void lb_stats(const float *__restrict__ src, const float *__restrict__ q, double *__restrict__ s_sum, int t)
{
#pragma unroll
    for (int half = 0; half < C / 16; ++half) {
        const int c = 16 * half + (t >> 4), j = t & 15;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(src + c * 256 + 16 * j + 4 * i);
            const f32x4 u = *reinterpret_cast<const f32x4 *>(q + c * 256 + 16 * j + 4 * i);
            s1 += (double)v.x; s2 += (double)v.x * (double)u.x;
            s1 += (double)v.y; s2 += (double)v.y * (double)u.y;
            s1 += (double)v.z; s2 += (double)v.z * (double)u.z;
            s1 += (double)v.w; s2 += (double)v.w * (double)u.w;
        }
        s1 += lane_xor1(s1); s2 += lane_xor1(s2);
        s1 += lane_xor2(s1); s2 += lane_xor2(s2);
        s1 += lane_xor4(s1); s2 += lane_xor4(s2);
        s1 += lane_xor8(s1); s2 += lane_xor8(s2);
        if (j == 0) { s_sum[c * 2] = s1; s_sum[c * 2 + 1] = s2; }
    }
    __syncthreads();
}

// bn_backward_finalize_kernel's coefficients of channel t from the patch's sums, count 256 -> s_coef[t][4]
template <int C>
__device__ __forceinline__ void lb_coef(const double *__restrict__ s_sum, const float *__restrict__ saved, const float *__restrict__ gamma,
                                        float *__restrict__ s_coef, int t)
{
    if (t < C) {
        const double sum_dy = s_sum[t * 2], sum_dya = s_sum[t * 2 + 1], inv_n = 1.0 / 256.0;
        const double mean = (double)saved[t * 2], invstd = (double)saved[t * 2 + 1], g = gamma ? (double)gamma[t] : 1.0;
        const double sum_dyxh = invstd * (sum_dya - mean * sum_dy);
        const double scale = g * invstd, c1 = sum_dy * inv_n, c2 = sum_dyxh * inv_n;
        const double Bc = -scale * invstd * c2;
        s_coef[t * 4 + 0] = (float)scale;
        s_coef[t * 4 + 1] = (float)Bc;
        s_coef[t * 4 + 2] = (float)(-scale * c1 - Bc * mean);
    }
    __syncthreads();
}

// da = c0 src + (c1 a + c2) (dm_operand AFFINE2's order) into the interior of the padded planes
template <int C>
__device__ __forceinline__ void lb_to_padded(const float *__restrict__ src, const float *__restrict__ a, const float *__restrict__ s_coef,
                                             float *__restrict__ pd, int t)
{
#pragma unroll
    for (int half = 0; half < C / 16; ++half) {
        const int c = 16 * half + (t >> 4), j = t & 15;
        const float c0 = s_coef[c * 4], c1 = s_coef[c * 4 + 1], c2 = s_coef[c * 4 + 2];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(src + c * 256 + 16 * j + 4 * i);
            const f32x4 u = *reinterpret_cast<const f32x4 *>(a + c * 256 + 16 * j + 4 * i);
            *reinterpret_cast<f32x4 *>(pd + c * LB_PS + (j + 1) * LB_RS + 4 + 4 * i) = c0 * v + (c1 * u + c2);
        }
    }
    __syncthreads();
}

// weights (CO, CI, 3, 3) of a forward convolution as the B operands of its data gradient: W[tap'][co][ci] = w[co][ci][8 - tap']
__device__ __forceinline__ void lb_stage_w3(const float *__restrict__ w, int CO, int CI, float *__restrict__ W, int t)
{
    for (int e = t; e < CO * CI * 9; e += 256) {
        const int tp = e / (CO * CI), rem = e - tp * (CO * CI);
        W[e] = w[rem * 9 + 8 - tp];
    }
}

// acc[mt][nt] (row 4 wave + mt, channels 16 nt + n, positions 4 q .. 4 q + 3) = sum over taps and the CIN channels of P
template <int CIN, int NT, int TAPS>
__device__ __forceinline__ void lb_product(const float *__restrict__ pd, const float *__restrict__ W, f32x4 (&acc)[4][NT], int wave, int lane)
{
    const int n = lane & 15, q = lane >> 4;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp) {
        const int ky = TAPS == 9 ? tp / 3 : 1, kx = TAPS == 9 ? tp % 3 : 1;
#pragma unroll
        for (int cg = 0; cg < CIN / 4; ++cg) {
            const int k = 4 * cg + q;
            float a[4], b[NT];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[mt] = pd[k * LB_PS + (4 * wave + mt + ky) * LB_RS + 3 + n + kx];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b[nt] = W[(tp * CIN + k) * (16 * NT) + 16 * nt + n];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ f32x4 lb_gate(f32x4 t, f32x4 v)
{
    return (f32x4){t.x > 0.f ? v.x : 0.f, t.y > 0.f ? v.y : 0.f, t.z > 0.f ? v.z : 0.f, t.w > 0.f ? v.w : 0.f};
}

__global__ __launch_bounds__(256) void latent_tail_bwd_kernel(LbParams P)
{
    extern __shared__ __attribute__((aligned(16))) float lb_smem[];
    __shared__ double s_sum[32 * 2];
    __shared__ __attribute__((aligned(16))) float s_coef[32 * 4];
    float *G = lb_smem + LB_G, *pd = lb_smem + LB_P, *Y = lb_smem + LB_Y, *W = lb_smem + LB_W;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n = lane & 15, q = lane >> 4;
    for (int e = t; e < 32 * LB_PS; e += 256) pd[e] = 0.f;          // the halo stays zero: only interiors are written below
    for (int b = blockIdx.x; b < P.B; b += gridDim.x) {
        const long long o16 = (long long)b * (16 * 256), o32 = (long long)b * (32 * 256);
        for (int e = t; e < 16 * 64; e += 256)
            *reinterpret_cast<f32x4 *>(G + 4 * e) = *reinterpret_cast<const f32x4 *>(P.g_z + o16 + 4 * e);
        __syncthreads();
        for (int l = P.nres - 1; l >= 0; --l) {
            const LbLayer &R = P.l[l];
            const float *ra = R.ra + o32, *rb = R.rb + o16, *hin = R.h_in + o16;
            // BatchNorm b backward, then the 1x1 convolution's data gradient (16 -> 32), masked by relu(BNa(ra))
            lb_stats<16>(G, rb, s_sum, t);
            lb_coef<16>(s_sum, R.savedb + (long long)b * 32, R.gb, s_coef, t);
            lb_to_padded<16>(G, rb, s_coef, pd, t);
            for (int e = t; e < 16 * 32; e += 256) W[e] = R.wb[e];                // B[k = co][n = ci] is wb as stored
            __syncthreads();
            {
                f32x4 acc[4][2];
                lb_product<16, 2, 1>(pd, W, acc, wave, lane);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int ch = 16 * nt + n;
                    const float c0 = R.coefa[((long long)b * 32 + ch) * 4], c2 = R.coefa[((long long)b * 32 + ch) * 4 + 2];
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) {
                        const int p0 = 16 * (4 * wave + mt) + 4 * q;
                        const f32x4 r = *reinterpret_cast<const f32x4 *>(ra + ch * 256 + p0);
                        *reinterpret_cast<f32x4 *>(Y + ch * 256 + p0) = lb_gate(c0 * r + c2, acc[mt][nt]);
                    }
                }
            }
            __syncthreads();
            // BatchNorm a backward, then the 3x3 convolution's data gradient (32 -> 16), masked by relu(h_in), + skip
            lb_stats<32>(Y, ra, s_sum, t);
            lb_coef<32>(s_sum, R.saveda + (long long)b * 64, R.ga, s_coef, t);
            lb_to_padded<32>(Y, ra, s_coef, pd, t);
            lb_stage_w3(R.wa, 32, 16, W, t);
            __syncthreads();
            {
                f32x4 acc[4][1];
                lb_product<32, 1, 9>(pd, W, acc, wave, lane);
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) {
                    const int p0 = 16 * (4 * wave + mt) + 4 * q;
                    const f32x4 h = *reinterpret_cast<const f32x4 *>(hin + n * 256 + p0);
                    f32x4 *g = reinterpret_cast<f32x4 *>(G + n * 256 + p0);
                    *g = *g + lb_gate(h, acc[mt][0]);
                }
            }
            __syncthreads();
        }
        // enc.11's backward, then enc.10's data gradient (16 -> 16), masked by relu(BN3(a3))
        const float *a4 = P.a4 + o16, *a3 = P.a3 + o16;
        lb_stats<16>(G, a4, s_sum, t);
        lb_coef<16>(s_sum, P.saved4 + (long long)b * 32, P.g4, s_coef, t);
        lb_to_padded<16>(G, a4, s_coef, pd, t);
        lb_stage_w3(P.w10, 16, 16, W, t);
        __syncthreads();
        {
            f32x4 acc[4][1];
            lb_product<16, 1, 9>(pd, W, acc, wave, lane);
            const float c0 = P.coef3[((long long)b * 16 + n) * 4], c2 = P.coef3[((long long)b * 16 + n) * 4 + 2];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int p0 = 16 * (4 * wave + mt) + 4 * q;
                const f32x4 r = *reinterpret_cast<const f32x4 *>(a3 + n * 256 + p0);
                const f32x4 out = lb_gate(c0 * r + c2, acc[mt][0]);
                *reinterpret_cast<f32x4 *>(Y + n * 256 + p0) = out;
                *reinterpret_cast<f32x4 *>(P.dy3 + o16 + n * 256 + p0) = out;
            }
        }
        __syncthreads();
        lb_stats<16>(Y, a3, s_sum, t);
        if (t < 32) P.st3[(long long)b * 32 + t] = s_sum[t];
        __syncthreads();
    }
}

DmPerDeviceOnce g_lb_once;

}  // namespace

extern "C" int dm_latent_tail_backward(const dm_latent_tail_bwd_args *a, void *stream)
{
    DM_REQUIRE(a, "dm_latent_tail_backward: NULL arguments");
    DM_REQUIRE(dm_latent_tail_supported(a->C, a->CR, a->H, a->W, a->nres), "dm_latent_tail_backward: built for 16 channels, 32 residual "
               "channels on a 16 x 16 latent grid, at most %d residual layers (got %d / %d on %d x %d, %d layers)", LB_MAX_RES,
               a->C, a->CR, a->H, a->W, a->nres);
    DM_REQUIRE(a->B > 0 && a->g_z && a->a3 && a->coef3 && a->a4 && a->saved4 && a->w10 && a->dy3 && a->stats3,
               "dm_latent_tail_backward: NULL pointer");
    uintptr_t al = (uintptr_t)a->g_z | (uintptr_t)a->a3 | (uintptr_t)a->a4 | (uintptr_t)a->dy3;
    LbParams P;
    P.g_z = a->g_z; P.a3 = a->a3; P.coef3 = a->coef3; P.a4 = a->a4; P.saved4 = a->saved4; P.g4 = a->gamma4; P.w10 = a->w10;
    P.dy3 = a->dy3; P.st3 = a->stats3; P.B = a->B; P.nres = a->nres;
    for (int l = 0; l < LB_MAX_RES; ++l) {
        const dm_latent_tail_bwd_res &r = a->res[l];
        const bool on = l < a->nres;
        if (on) {
            DM_REQUIRE(r.ra && r.rb && r.h_in && r.coefa && r.saveda && r.savedb && r.wa && r.wb,
                       "dm_latent_tail_backward: residual layer %d: NULL pointer", l);
            al |= (uintptr_t)r.ra | (uintptr_t)r.rb | (uintptr_t)r.h_in;
        }
        P.l[l] = on ? LbLayer{r.ra, r.rb, r.h_in, r.coefa, r.saveda, r.savedb, r.gamma_a, r.gamma_b, r.wa, r.wb}
                    : LbLayer{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    }
    DM_REQUIRE((al & 15) == 0, "dm_latent_tail_backward: the activation tensors must be 16-byte aligned");
    const size_t lds = LB_FLOATS * sizeof(float);
    const int rc = dm_reserve_lds(g_lb_once, {{(const void *)latent_tail_bwd_kernel, lds}}, "dm_latent_tail_backward");
    if (rc) return rc;
    const int grid = a->B < 256 ? a->B : 256;                 // 120 KB of LDS: one workgroup per CU
    hipLaunchKernelGGL(latent_tail_bwd_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, P);
    return dm_launch_status("dm_latent_tail_backward");
}
