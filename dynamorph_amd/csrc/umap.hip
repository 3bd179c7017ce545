// umap.hip -- the UMAP fit behind the exact k-NN graph (knn.hip): smooth distances, membership strengths and one epoch of
// the deterministic layout.  The symmetrisation, the pruning and the schedule arrays are sorting
// and merging of integer keys and stay with torch (dynamorph_amd/umap_layout.py).  And the transform of new points into a
// fitted embedding (section 3.5d): one kernel from the query graph to the schedule and the start positions, and one launch
// for all epochs of the layout, in which only the new points move.
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

// The two updates of the running position (cx, cy), shared by the fit's epoch kernel and the transform's layout kernel.
// Attraction toward (ox, oy): g = -2ab d2^(b-1) / (a d2^b + 1), 0 at d2 = 0; m2ab = -2ab, bm1 = b - 1.
__device__ __forceinline__ void um_attract(float &cx, float &cy, float ox, float oy, float alpha, float a, float b, float bm1,
                                           float m2ab)
{
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

// Repulsion from (qx, qy): g = 2 gamma b / ((0.001 + d2)(a d2^b + 1)), nothing at d2 = 0; g2b = 2 gamma b.
__device__ __forceinline__ void um_repel(float &cx, float &cy, float qx, float qy, float alpha, float a, float b, float g2b)
{
    const float dx = cx - qx, dy = cy - qy;
    const float d2 = dx * dx + dy * dy;
    if (d2 > 0.f) {
        const float pb = __builtin_amdgcn_exp2f(b * um_log2(d2));
        const float g = g2b * __builtin_amdgcn_rcpf((0.001f + d2) * (a * pb + 1.f));   // (denominator >= 0.001)
        cx += alpha * um_clip(g * dx);
        cy += alpha * um_clip(g * dy);
    }
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
            for (int r = 0; r < 2; ++r)             // head of (i -> j), tail of the mirrored (j -> i)
                um_attract(cx, cy, ox, oy, alpha, a, b, bm1, m2ab);
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
                    um_repel(cx, cy, qx, qy, alpha, a, b, g2b);
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

// ----------------------------------------------------------------------------------- transform of new points (section 3.5d)
// One wave per query row; lane l holds columns l, l + 64, l + 128, l + 192 of the row's k sorted distances to training rows.
// One residency of the row gives its mean, the search for sigma (rho = 0, every column counts), the memberships, their
// maximum, the schedule arrays and the membership-weighted mean of the neighbours' training positions.  Sums are float64 in
// the order of umap_rowmean_kernel / umap_smooth_kernel: a lane's columns in order, then the butterfly of wave_sum.
__global__ __launch_bounds__(256) void umap_transform_prepare_kernel(const int *__restrict__ indices,
                                                                     const float *__restrict__ dists, long long R, int k,
                                                                     const f32x2 *__restrict__ y_train, float n_epochs_f,
                                                                     float rate_f, float *__restrict__ sigma,
                                                                     float *__restrict__ membership, float *__restrict__ eps,
                                                                     float *__restrict__ eps_neg, float *__restrict__ next,
                                                                     float *__restrict__ next_neg, f32x2 *__restrict__ y0)
{
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const int lane = threadIdx.x & 63;
    const float *__restrict__ d = dists + row * k;
    const int *__restrict__ ix = indices + row * k;
    float v[4];
    bool valid[4];
    f32x2 yj[4];
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int c = lane + 64 * t;
        valid[t] = c < k;
        v[t] = valid[t] ? d[c] : 0.f;
        yj[t] = valid[t] ? y_train[ix[c]] : (f32x2){0.f, 0.f};
        if (valid[t]) s += (double)v[t];
    }
    const double row_mean = wave_sum(s) / (double)k;
    double x[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) x[t] = (double)v[t];
    const double target = log2((double)k);
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int step = 0; step < 64; ++step) {
        double sm = 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (valid[t]) sm += x[t] > 0.0 ? exp(-(x[t] / mid)) : 1.0;
        sm = wave_sum(sm);
        if (fabs(sm - target) < 1e-5) break;
        if (sm > target) {
            hi = mid;
            mid = (lo + hi) * 0.5;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.0 : (lo + hi) * 0.5;
        }
    }
    const double floor_ = 1e-3 * row_mean;
    if (mid < floor_) mid = floor_;
    const float sg = (float)mid;
    float a[4];
    float m = 0.f;
    double sa = 0.0, sx = 0.0, sy = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        a[t] = !valid[t] ? 0.f : (v[t] <= 0.f || sg == 0.f) ? 1.f : expf(-(v[t] / sg));
        m = fmaxf(m, a[t]);
        if (valid[t]) {
            sa += (double)a[t];
            sx += (double)a[t] * (double)yj[t].x;
            sy += (double)a[t] * (double)yj[t].y;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    sa = wave_sum(sa);
    sx = wave_sum(sx);
    sy = wave_sum(sy);
    const float thr = m / n_epochs_f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (!valid[t]) continue;
        const long long e = row * k + lane + 64 * t;
        const bool pruned = a[t] == 0.f || a[t] < thr;
        const float ep = pruned ? INFINITY : m / a[t];
        const float en = pruned ? INFINITY : ep / rate_f;
        membership[e] = a[t];
        eps[e] = ep;
        next[e] = ep;
        eps_neg[e] = en;
        next_neg[e] = en;
    }
    if (lane == 0) {
        sigma[row] = sg;
        // all memberships zero (no finite distance within reach of the search): the nearest neighbour's position
        y0[row] = sa > 0.0 ? (f32x2){(float)(sx / sa), (float)(sy / sa)} : y_train[ix[0]];
    }
}

// All epochs [n0, n1) of a query in one launch: the training positions are fixed and a query reads nothing another query
// writes, so there is nothing to wait for between epochs.  G lanes own query i; its running position c is a register (the
// same bits in every lane of the group) and the schedule state next / next_neg of its row lies in LDS from the first epoch
// to the last -- entry j always in the hands of lane j mod G, so the LDS words are private to a lane and no barrier is
// needed.  Pruned entries (+inf, never firing) are found once while loading and only the columns before the last live
// one are scanned.  An epoch is the fit kernel's: scan G entries at a time, advance the state of those that fire and
// request their neighbours' positions, then update c in column order on every lane of the group alike, the negatives drawn
// and gathered G at a time.  eps / eps_neg / indices are read where an entry fires.  Positions and state are written back
// once, after epoch n1 - 1.  Control flow is uniform within a group; the result does not depend on G.
constexpr int UM_T_THREADS = 128;

template <int G>
__global__ __launch_bounds__(UM_T_THREADS) void umap_transform_layout_kernel(
    const int *__restrict__ indices, const float *__restrict__ eps, const float *__restrict__ eps_neg, float *__restrict__ next,
    float *__restrict__ next_neg, long long R, int k, int stride, unsigned M, const f32x2 *__restrict__ y_train,
    f32x2 *__restrict__ y, int n0, int n1, float n_epochs_f, unsigned long long row_offset, unsigned long long seed, float a,
    float b, float gamma)
{
    extern __shared__ float um_state[];
    constexpr int Q = UM_T_THREADS / G;             // queries of a workgroup
    const int q = threadIdx.x / G;
    const long long i = (long long)blockIdx.x * Q + q;
    if (i >= R) return;
    const int l = threadIdx.x & (G - 1);
    const int group_shift = (threadIdx.x & 63) & ~(G - 1);
    const unsigned long long group_bits = G == 64 ? ~0ull : ((1ull << G) - 1ull);
    float *nx = um_state + q * stride, *nq = um_state + (Q + q) * stride;
    const long long row = i * k;
    int kact = 0;
    for (int j = l; j < k; j += G) {
        const float x = next[row + j];
        nx[j] = x;
        nq[j] = next_neg[row + j];
        if (x < INFINITY) kact = j + 1;
    }
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) {
        const int other = __shfl_xor(kact, o, G);
        kact = other > kact ? other : kact;
    }
    const f32x2 c0 = y[i];
    float cx = c0.x, cy = c0.y;
    const float m2ab = -2.f * a * b, g2b = 2.f * gamma * b, bm1 = b - 1.f;
    const unsigned long long entry0 = (row_offset + (unsigned long long)i) * (unsigned long long)k;
    for (int n = n0; n < n1; ++n) {
        const float nf = (float)n;
        const float alpha = 0.25f * (1.0f - nf / n_epochs_f);
        const unsigned long long key = um_mix64(seed + UM_GOLDEN * (unsigned long long)(n + 1));
        for (int base = 0; base < kact; base += G) {
            const int j = base + l;
            bool fires = false;
            float jx = 0.f, jy = 0.f;
            int nn = 0;
            if (j < kact) {
                const float x = nx[j];
                if (x <= nf) {
                    fires = true;
                    const f32x2 yj = y_train[indices[row + j]];
                    jx = yj.x; jy = yj.y;
                    nx[j] = x + eps[row + j];
                    const float en = eps_neg[row + j], nqj = nq[j];
                    nn = (int)((nf - nqj) / en);
                    nq[j] = nqj + (float)nn * en;
                }
            }
            unsigned long long mask = (__ballot(fires) >> group_shift) & group_bits;
            while (mask) {
                const int t = __ffsll(mask) - 1;
                mask &= mask - 1;
                const float ox = __shfl(jx, t, G), oy = __shfl(jy, t, G);
                const int onn = __shfl(nn, t, G);
                um_attract(cx, cy, ox, oy, alpha, a, b, bm1, m2ab);         // once: only the query moves
                const unsigned long long ke = um_mix64(key ^ (entry0 + (unsigned long long)(base + t)));
                for (int p0 = 0; p0 < onn; p0 += G) {
                    const int p = p0 + l;
                    float vx = 0.f, vy = 0.f;
                    if (p < onn) {
                        const f32x2 yv = y_train[(unsigned)(um_mix64(ke + UM_GOLDEN * (unsigned long long)(p + 1)) >> 32) % M];
                        vx = yv.x; vy = yv.y;
                    }
                    const int cnt = onn - p0 < G ? onn - p0 : G;
                    for (int r = 0; r < cnt; ++r)
                        um_repel(cx, cy, __shfl(vx, r, G), __shfl(vy, r, G), alpha, a, b, g2b);
                }
            }
        }
    }
    for (int j = l; j < kact; j += G) {
        next[row + j] = nx[j];
        next_neg[row + j] = nq[j];
    }
    if (l == 0) y[i] = (f32x2){cx, cy};
}

// The LDS row of a query: the smallest stride >= k that is 8 modulo 16 words, so that the four groups of eight lanes in a
// half-wave (the unit of ds_read_b32 banking, 32 banks) start on different banks.
int transform_stride(int k) { return k + ((8 - k % 16) + 16) % 16; }

template <int G>
void transform_layout_launch(const int32_t *indices, const float *eps, const float *eps_neg, float *next, float *next_neg,
                             long long R, int k, unsigned M, const float *y_train, float *y, int n0, int n1, int n_epochs,
                             unsigned long long row_offset, unsigned long long seed, float a, float b, float gamma, hipStream_t s)
{
    constexpr int Q = UM_T_THREADS / G;
    const int stride = transform_stride(k);
    const unsigned blocks = (unsigned)((R + Q - 1) / Q);
    const size_t lds = (size_t)2 * Q * stride * sizeof(float);          // at most 2 * 16 * 264 * 4 = 33 792 bytes
    hipLaunchKernelGGL(umap_transform_layout_kernel<G>, dim3(blocks), dim3(UM_T_THREADS), lds, s, indices, eps, eps_neg, next,
                       next_neg, R, k, stride, M, (const f32x2 *)y_train, (f32x2 *)y, n0, n1, (float)n_epochs, row_offset, seed,
                       a, b, gamma);
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

extern "C" int dm_umap_transform_prepare(const int32_t *indices, const float *dists, int64_t R, int k, int64_t M,
                                         const float *y_train, int n_epochs, int negative_sample_rate, float *sigma,
                                         float *membership, float *eps, float *eps_neg, float *next, float *next_neg, float *y0,
                                         void *stream)
{
    DM_REQUIRE(indices && dists && y_train && sigma && membership && eps && eps_neg && next && next_neg && y0,
               "dm_umap_transform_prepare: indices / dists / y_train / sigma / membership / eps / eps_neg / next / next_neg / y0 is NULL");
    DM_REQUIRE(R >= 1 && R <= 0x7fffffffLL, "dm_umap_transform_prepare: R = %lld must lie in 1 .. 2^31 - 1", (long long)R);
    const char *why = umap_shape(M, k);
    DM_REQUIRE(!why, "dm_umap_transform_prepare: M = %lld, k = %d: %s", (long long)M, k, why ? why : "");
    DM_REQUIRE(n_epochs >= 1, "dm_umap_transform_prepare: n_epochs = %d must be at least 1", n_epochs);
    DM_REQUIRE(negative_sample_rate >= 1 && negative_sample_rate <= 1000,
               "dm_umap_transform_prepare: negative_sample_rate = %d outside 1 .. 1000", negative_sample_rate);
    const unsigned blocks = (unsigned)((R + 3) / 4);
    hipLaunchKernelGGL(umap_transform_prepare_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, indices, dists,
                       (long long)R, k, (const f32x2 *)y_train, (float)n_epochs, (float)negative_sample_rate, sigma, membership,
                       eps, eps_neg, next, next_neg, (f32x2 *)y0);
    return dm_launch_status("dm_umap_transform_prepare");
}

extern "C" int dm_umap_transform_layout(const int32_t *indices, const float *eps, const float *eps_neg, float *next,
                                        float *next_neg, int64_t R, int k, int64_t M, const float *y_train, float *y,
                                        int epoch_begin, int epoch_end, int n_epochs, int64_t row_offset, float a, float b,
                                        float gamma, uint64_t seed, int group, void *stream)
{
    DM_REQUIRE(indices && eps && eps_neg && next && next_neg && y_train && y,
               "dm_umap_transform_layout: indices / eps / eps_neg / next / next_neg / y_train / y is NULL");
    DM_REQUIRE(R >= 1 && R <= 0x7fffffffLL, "dm_umap_transform_layout: R = %lld must lie in 1 .. 2^31 - 1", (long long)R);
    const char *why = umap_shape(M, k);
    DM_REQUIRE(!why, "dm_umap_transform_layout: M = %lld, k = %d: %s", (long long)M, k, why ? why : "");
    DM_REQUIRE(n_epochs >= 1 && epoch_begin >= 0 && epoch_begin <= epoch_end && epoch_end <= n_epochs,
               "dm_umap_transform_layout: epochs [%d, %d) outside [0, n_epochs = %d]", epoch_begin, epoch_end, n_epochs);
    DM_REQUIRE(row_offset >= 0, "dm_umap_transform_layout: row_offset = %lld is negative", (long long)row_offset);
    DM_REQUIRE(a > 0.f && b > 0.f, "dm_umap_transform_layout: a = %g and b = %g must be positive", (double)a, (double)b);
    DM_REQUIRE(group == 0 || group == 8 || group == 64, "dm_umap_transform_layout: group = %d, must be 0 (auto), 8 or 64", group);
    // As in dm_umap_epoch every lane of a group repeats the updates: 8 lanes scan a row of 15 in two steps and leave eight
    // queries to a wave; a whole wave per query scans 64 entries at once (DESIGN.md section 3.5d has both measured).
    if (group == 0) group = 8;
    hipStream_t s = (hipStream_t)stream;
    if (group == 8)
        transform_layout_launch<8>(indices, eps, eps_neg, next, next_neg, R, k, (unsigned)M, y_train, y, epoch_begin, epoch_end,
                                   n_epochs, (unsigned long long)row_offset, seed, a, b, gamma, s);
    else
        transform_layout_launch<64>(indices, eps, eps_neg, next, next_neg, R, k, (unsigned)M, y_train, y, epoch_begin, epoch_end,
                                    n_epochs, (unsigned long long)row_offset, seed, a, b, gamma, s);
    return dm_launch_status("dm_umap_transform_layout");
}
