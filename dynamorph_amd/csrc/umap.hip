// umap.hip -- the UMAP fit behind the exact k-NN graph (knn.hip): smooth distances, membership strengths and one epoch of
// the deterministic layout.  The symmetrisation, the pruning and the schedule arrays are sorting
// and merging of integer keys and stay with torch (dynamorph_amd/umap_layout.py).
//
// Compiled with -ffp-contract=off (Makefile): the membership argument, the schedule state and the layout updates are one
// fixed sequence of fp32 operations, so a float32 numpy evaluation of the schedule gives the same bits.
#include "dm_common.h"
#include <math.h>

namespace {

constexpr unsigned long long UM_GOLDEN = 0x9E3779B97F4A7C15ull;

// The finaliser of splitmix64 (Steele, Lea, Flood 2014): a bijection of 64-bit words.
__host__ __device__ __forceinline__ unsigned long long um_mix64(unsigned long long z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// ---------------------------------------------------------------------------------------------------- smooth distances
// One wave per row; lane l holds columns l, l + 64, l + 128, l + 192.  Sums are float64: the lanes' partial sums in column
// order, then the butterfly of wave_sum, which leaves the same total in every lane (so every lane takes the same branch).
__global__ __launch_bounds__(256) void umap_rowmean_kernel(const float *__restrict__ dists, long long N, int k,
                                                           double *__restrict__ row_mean)
{
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const float *__restrict__ d = dists + row * k;
    double s = 0.0;
    for (int c = lane; c < k; c += 64) s += (double)d[c];
    s = wave_sum(s);
    if (lane == 0) row_mean[row] = s / (double)k;
}

// The mean of all N k distances = the mean of the row means (every row has k columns): one workgroup, thread t adds rows
// t, t + 256, ... in that order.
__global__ __launch_bounds__(256) void umap_globalmean_kernel(const double *__restrict__ row_mean, long long N,
                                                              double *__restrict__ global_mean)
{
    __shared__ double scratch[4];
    double s = 0.0;
    for (long long r = threadIdx.x; r < N; r += 256) s += row_mean[r];
    s = block_sum(s, scratch);
    if (threadIdx.x == 0) *global_mean = s / (double)N;
}

__global__ __launch_bounds__(256) void umap_smooth_kernel(const float *__restrict__ dists, long long N, int k,
                                                          const double *__restrict__ row_mean,
                                                          const double *__restrict__ global_mean, float *__restrict__ rho,
                                                          float *__restrict__ sigma)
{
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int lane = threadIdx.x & 63;
    const float *__restrict__ d = dists + row * k;
    float v[4];
    bool valid[4];
    float rmin = INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int c = lane + 64 * t;
        valid[t] = c >= 1 && c < k;
        v[t] = valid[t] ? d[c] : 0.f;
        if (valid[t] && v[t] > 0.f) rmin = fminf(rmin, v[t]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rmin = fminf(rmin, __shfl_xor(rmin, o, 64));
    const float rho_f = rmin == INFINITY ? 0.f : rmin;
    double x[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = (double)v[t] - (double)rho_f;
    const double target = log2((double)k);
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int step = 0; step < 64; ++step) {
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (valid[t]) s += x[t] > 0.0 ? exp(-(x[t] / mid)) : 1.0;
        s = wave_sum(s);
        if (fabs(s - target) < 1e-5) break;
        if (s > target) {
            hi = mid;
            mid = (lo + hi) * 0.5;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.0 : (lo + hi) * 0.5;
        }
    }
    const double floor_ = 1e-3 * (rho_f > 0.f ? row_mean[row] : *global_mean);
    if (mid < floor_) mid = floor_;
    if (lane == 0) {
        rho[row] = rho_f;
        sigma[row] = (float)mid;
    }
}

// ---------------------------------------------------------------------------------------------------------- membership
__global__ __launch_bounds__(256) void umap_membership_kernel(const int *__restrict__ indices, const float *__restrict__ dists,
                                                              long long N, int k, const float *__restrict__ rho,
                                                              const float *__restrict__ sigma, float *__restrict__ out)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * k) return;
    const long long row = idx / k;
    float a = 0.f;
    if ((long long)indices[idx] != row) {
        const float t = dists[idx] - rho[row];
        const float s = sigma[row];
        a = (t <= 0.f || s == 0.f) ? 1.f : expf(-(t / s));
    }
    out[idx] = a;
}

// --------------------------------------------------------------------------------------------------------------- layout
__device__ __forceinline__ float um_clip(float x) { return fminf(fmaxf(x, -4.f), 4.f); }

// log2 of a positive float on the hardware's v_log_f32 (1 ulp); a subnormal argument, which the instruction would read as
// zero, is scaled into range first.  With v_exp_f32 (1 ulp) this gives x^p = exp2(p log2 x) to about (1 + |p log2 x|) 2^-23
// in 3 instructions where powf takes about a hundred; the serial chain of a row's updates is what bounds an epoch.
__device__ __forceinline__ float um_log2(float x)
{
    const bool tiny = x < 0x1p-64f;
    const float l = __builtin_amdgcn_logf(tiny ? x * 0x1p64f : x);
    return tiny ? l - 64.f : l;
}

// One epoch: G lanes own vertex i (its CSR row, its position, the schedule state of its entries); nothing else writes what
// they write.  The G lanes scan G entries of the row at a time: each lane reads its entry's schedule state, advances it, and
// where the entry fires requests the neighbour's position -- all gathers of a chunk are in flight before the first update.
// The updates themselves run in row order on every lane of the group alike (the running position c is the same bits in
// each), the operands handed round by lane exchanges; the negatives of a firing entry are drawn and gathered G at a time the
// same way.  Control flow is uniform within a group, so a lane exchange never reads a lane that is somewhere else.  The
// result does not depend on G.
template <int G>
__global__ __launch_bounds__(256) void umap_epoch_kernel(const long long *__restrict__ indptr, const int *__restrict__ cols,
                                                         long long N, const float *__restrict__ eps,
                                                         const float *__restrict__ eps_neg, float *__restrict__ next,
                                                         float *__restrict__ next_neg, const f32x2 *__restrict__ yin,
                                                         f32x2 *__restrict__ yout, float nf, float alpha, float a, float b,
                                                         float gamma, unsigned long long key)
{
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
    if (i >= N) return;
    const int l = threadIdx.x & (G - 1);
    const int group_shift = (threadIdx.x & 63) & ~(G - 1);
    const unsigned group_bits = G == 32 ? 0xffffffffu : ((1u << G) - 1u);
    const f32x2 c0 = yin[i];
    float cx = c0.x, cy = c0.y;
    const float m2ab = -2.f * a * b, g2b = 2.f * gamma * b, bm1 = b - 1.f;
    const long long e0 = indptr[i], e1 = indptr[i + 1];
    for (long long base = e0; base < e1; base += G) {
        const long long e = base + l;
        bool fires = false;
        float jx = 0.f, jy = 0.f;
        int nn = 0;
        if (e < e1) {
            const float nx = next[e];
            if (nx <= nf) {
                fires = true;
                const f32x2 yj = yin[cols[e]];
                jx = yj.x; jy = yj.y;
                next[e] = nx + eps[e];
                const float en = eps_neg[e], nq = next_neg[e];
                nn = (int)((nf - nq) / en);
                next_neg[e] = nq + (float)nn * en;
            }
        }
        unsigned mask = (unsigned)(__ballot(fires) >> group_shift) & group_bits;
        while (mask) {
            const int t = __ffs(mask) - 1;
            mask &= mask - 1;
            const float ox = __shfl(jx, t, G), oy = __shfl(jy, t, G);
            const int onn = __shfl(nn, t, G);
#pragma unroll
            for (int r = 0; r < 2; ++r) {           // head of (i -> j), tail of the mirrored (j -> i)
                const float dx = cx - ox, dy = cy - oy;
                const float d2 = dx * dx + dy * dy;
                float g = 0.f;
                if (d2 > 0.f) {
                    const float lg = um_log2(d2);
                    const float pb = __builtin_amdgcn_exp2f(b * lg), pb1 = __builtin_amdgcn_exp2f(bm1 * lg);
                    g = (m2ab * pb1) * __builtin_amdgcn_rcpf(a * pb + 1.f);          // (denominator >= 1)
                }
                cx += alpha * um_clip(g * dx);
                cy += alpha * um_clip(g * dy);
            }
            const unsigned long long ke = um_mix64(key ^ (unsigned long long)(base + t));
            for (int p0 = 0; p0 < onn; p0 += G) {
                const int p = p0 + l;
                int v = 0;
                float vx = 0.f, vy = 0.f;
                if (p < onn) {
                    v = (int)((unsigned)(um_mix64(ke + UM_GOLDEN * (unsigned long long)(p + 1)) >> 32) % (unsigned)N);
                    const f32x2 yv = yin[v];
                    vx = yv.x; vy = yv.y;
                }
                const int cnt = onn - p0 < G ? onn - p0 : G;
                for (int q = 0; q < cnt; ++q) {
                    const int vv = __shfl(v, q, G);
                    const float qx = __shfl(vx, q, G), qy = __shfl(vy, q, G);
                    if ((long long)vv == i) continue;
                    const float dx = cx - qx, dy = cy - qy;
                    const float d2 = dx * dx + dy * dy;
                    if (d2 > 0.f) {
                        const float pb = __builtin_amdgcn_exp2f(b * um_log2(d2));
                        const float g = g2b * __builtin_amdgcn_rcpf((0.001f + d2) * (a * pb + 1.f));   // (denominator >= 0.001)
                        cx += alpha * um_clip(g * dx);
                        cy += alpha * um_clip(g * dy);
                    }
                }
            }
        }
    }
    if (l == 0) yout[i] = (f32x2){cx, cy};
}

template <int G>
void epoch_launch(const int64_t *indptr, const int32_t *cols, long long N, const float *eps, const float *eps_neg, float *next,
                  float *next_neg, const float *yin, float *yout, float nf, float alpha, float a, float b, float gamma,
                  unsigned long long key, hipStream_t s)
{
    const unsigned blocks = (unsigned)((N * G + 255) / 256);
    hipLaunchKernelGGL(umap_epoch_kernel<G>, dim3(blocks), dim3(256), 0, s, (const long long *)indptr, cols, N, eps, eps_neg, next,
                       next_neg, (const f32x2 *)yin, (f32x2 *)yout, nf, alpha, a, b, gamma, key);
}

const char *umap_shape(int64_t N, int k)
{
    if (N < 1 || N > 0x7fffffffLL) return "N must lie in 1 .. 2^31 - 1";
    if (k < 2 || k > DM_UMAP_MAX_K) return "k outside 2 .. DM_UMAP_MAX_K";
    if (k > N) return "k exceeds N";
    return nullptr;
}

}  // namespace

extern "C" int dm_umap_smooth(const float *dists, int64_t N, int k, float *rho, float *sigma, double *row_mean,
                              double *global_mean, void *stream)
{
    DM_REQUIRE(dists && rho && sigma && row_mean && global_mean, "dm_umap_smooth: dists / rho / sigma / row_mean / global_mean is NULL");
    const char *why = umap_shape(N, k);
    DM_REQUIRE(!why, "dm_umap_smooth: N = %lld, k = %d: %s", (long long)N, k, why ? why : "");
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((N + 3) / 4);
    hipLaunchKernelGGL(umap_rowmean_kernel, dim3(blocks), dim3(256), 0, s, dists, (long long)N, k, row_mean);
    hipLaunchKernelGGL(umap_globalmean_kernel, dim3(1), dim3(256), 0, s, (const double *)row_mean, (long long)N, global_mean);
    hipLaunchKernelGGL(umap_smooth_kernel, dim3(blocks), dim3(256), 0, s, dists, (long long)N, k, (const double *)row_mean,
                       (const double *)global_mean, rho, sigma);
    return dm_launch_status("dm_umap_smooth");
}

extern "C" int dm_umap_membership(const int32_t *indices, const float *dists, int64_t N, int k, const float *rho,
                                  const float *sigma, float *membership, void *stream)
{
    DM_REQUIRE(indices && dists && rho && sigma && membership, "dm_umap_membership: indices / dists / rho / sigma / membership is NULL");
    const char *why = umap_shape(N, k);
    DM_REQUIRE(!why, "dm_umap_membership: N = %lld, k = %d: %s", (long long)N, k, why ? why : "");
    const unsigned blocks = (unsigned)((N * k + 255) / 256);
    hipLaunchKernelGGL(umap_membership_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, indices, dists, (long long)N, k,
                       rho, sigma, membership);
    return dm_launch_status("dm_umap_membership");
}

extern "C" int dm_umap_epoch(const int64_t *indptr, const int32_t *cols, int64_t N, int64_t nnz, const float *eps,
                             const float *eps_neg, float *next, float *next_neg, const float *y_in, float *y_out, int epoch,
                             int n_epochs, float a, float b, float gamma, uint64_t seed, int group, void *stream)
{
    DM_REQUIRE(indptr && y_in && y_out, "dm_umap_epoch: indptr / y_in / y_out is NULL");
    DM_REQUIRE(N >= 1 && N <= 0x7fffffffLL, "dm_umap_epoch: N = %lld must lie in 1 .. 2^31 - 1", (long long)N);
    DM_REQUIRE(nnz >= 0, "dm_umap_epoch: nnz = %lld is negative", (long long)nnz);
    DM_REQUIRE(nnz == 0 || (cols && eps && eps_neg && next && next_neg),
               "dm_umap_epoch: cols / eps / eps_neg / next / next_neg is NULL");
    DM_REQUIRE(y_in != y_out, "dm_umap_epoch: y_in and y_out are the same buffer");
    DM_REQUIRE(n_epochs >= 1 && epoch >= 0 && epoch < n_epochs, "dm_umap_epoch: epoch %d outside 0 .. n_epochs - 1 = %d", epoch,
               n_epochs - 1);
    DM_REQUIRE(a > 0.f && b > 0.f, "dm_umap_epoch: a = %g and b = %g must be positive", (double)a, (double)b);
    DM_REQUIRE(group == 0 || group == 1 || group == 8 || group == 32, "dm_umap_epoch: group = %d, must be 0 (auto), 1, 8 or 32", group);
    // Every lane of a group repeats the updates, so a group of G costs G issue slots per update, while the scan of a row and
    // its gathers go G at a time: 8 is the fastest form without hubs and within 15 % of 32 with them.
    if (group == 0) group = 8;
    const float nf = (float)epoch;
    const float alpha = 1.0f - nf / (float)n_epochs;
    const unsigned long long key = um_mix64((unsigned long long)seed + UM_GOLDEN * (unsigned long long)(epoch + 1));
    hipStream_t s = (hipStream_t)stream;
    if (group == 1)
        epoch_launch<1>(indptr, cols, N, eps, eps_neg, next, next_neg, y_in, y_out, nf, alpha, a, b, gamma, key, s);
    else if (group == 8)
        epoch_launch<8>(indptr, cols, N, eps, eps_neg, next, next_neg, y_in, y_out, nf, alpha, a, b, gamma, key, s);
    else
        epoch_launch<32>(indptr, cols, N, eps, eps_neg, next, next_neg, y_in, y_out, nf, alpha, a, b, gamma, key, s);
    return dm_launch_status("dm_umap_epoch");
}
