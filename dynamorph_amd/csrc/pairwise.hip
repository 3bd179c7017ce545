// pairwise.hip -- the pairwise mean-squared latent distance of the time-matching loss.
//
// Reference: HiddenStateExtractor/vq_vae.py:324-329 and vae.py:322-326
//     z = z_before.reshape(B, -1);  sim_mat = pow(z.reshape(1, B, n) - z.reshape(B, 1, n), 2).mean(2)
// which materialises a (B, B, n) tensor (n = 4096: 268 MB at B = 128, 68 GB at B = 2048).  Here the (B, B)
// result is formed directly; differences are taken before squaring (no |a|^2 + |b|^2 - 2ab cancellation).
// The weighting / hinge / mean of the (B, B) matrix stays in torch (it is B*B elements); its autograd hands
// g = dL/dsim back to dm_pair_msd_backward:
//     dz[i] = (2/n) * sum_j (g[i][j] + g[j][i]) * (z[i] - z[j])
#include "dm_common.h"

namespace {

constexpr int PM_T = 16;          // pairs block: 16 x 16
constexpr int PM_CH = 64;         // latent elements staged per step

// sim[i][j] = (1/n) sum_d (z[i][d] - z[j][d])^2 ; one workgroup per 16 x 16 block of pairs, thread = one pair
__global__ __launch_bounds__(256) void pair_msd_kernel(const float *__restrict__ z, float *__restrict__ sim, int B, int n)
{
    __shared__ float sI[PM_T][PM_CH + 1], sJ[PM_T][PM_CH + 1];
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    const int i0 = blockIdx.y * PM_T, j0 = blockIdx.x * PM_T;
    double acc = 0.0;
    for (int d0 = 0; d0 < n; d0 += PM_CH) {
        __syncthreads();
        for (int e = threadIdx.x; e < PM_T * PM_CH; e += 256) {
            const int r = e / PM_CH, c = e % PM_CH;
            const int d = d0 + c;
            sI[r][c] = (i0 + r < B && d < n) ? z[(long long)(i0 + r) * n + d] : 0.f;
            sJ[r][c] = (j0 + r < B && d < n) ? z[(long long)(j0 + r) * n + d] : 0.f;
        }
        __syncthreads();
        float part = 0.f;
#pragma unroll 16
        for (int c = 0; c < PM_CH; ++c) {
            const float df = sJ[tj][c] - sI[ti][c];
            part += df * df;
        }
        acc += (double)part;
    }
    if (i0 + ti < B && j0 + tj < B) sim[(long long)(i0 + ti) * B + j0 + tj] = (float)(acc / (double)n);
}

// dz[i][d] = (2/n) * sum_j s_ij * (z[i][d] - z[j][d]),  s_ij = g[i][j] + g[j][i]
// one workgroup per (16 rows i) x (256 elements d); j walks in chunks of 16 through LDS
__global__ __launch_bounds__(256) void pair_msd_backward_kernel(const float *__restrict__ z, const float *__restrict__ g,
                                                                float *__restrict__ dz, int B, int n)
{
    __shared__ float sS[PM_T][PM_T + 1];            // s_ij for the block's 16 rows i and the current 16 columns j
    __shared__ float sZ[PM_T][256];                 // z[j][d chunk]
    const int i0 = blockIdx.y * PM_T, d = blockIdx.x * 256 + threadIdx.x;
    float zi[PM_T];
    double acc[PM_T];
#pragma unroll
    for (int r = 0; r < PM_T; ++r) {
        zi[r] = (i0 + r < B && d < n) ? z[(long long)(i0 + r) * n + d] : 0.f;
        acc[r] = 0.0;
    }
    for (int j0 = 0; j0 < B; j0 += PM_T) {
        __syncthreads();
        {
            const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
            const int i = i0 + r, j = j0 + c;
            sS[r][c] = (i < B && j < B) ? g[(long long)i * B + j] + g[(long long)j * B + i] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < PM_T; ++r) sZ[r][threadIdx.x] = (j0 + r < B && d < n) ? z[(long long)(j0 + r) * n + d] : 0.f;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PM_T; ++r) {
            float part = 0.f;
#pragma unroll
            for (int c = 0; c < PM_T; ++c) part += sS[r][c] * (zi[r] - sZ[c][threadIdx.x]);
            acc[r] += (double)part;
        }
    }
    if (d < n) {
        const double sc = 2.0 / (double)n;
#pragma unroll
        for (int r = 0; r < PM_T; ++r)
            if (i0 + r < B) dz[(long long)(i0 + r) * n + d] = (float)(acc[r] * sc);
    }
}

}  // namespace

extern "C" int dm_pair_msd(const float *z, float *sim, int B, int n, void *stream)
{
    DM_REQUIRE(z && sim && B > 0 && n > 0, "dm_pair_msd: bad argument");
    DM_REQUIRE((long long)B * n < (1LL << 31), "dm_pair_msd: tensor too large for 32-bit offsets");
    const int nb = (B + PM_T - 1) / PM_T;
    hipLaunchKernelGGL(pair_msd_kernel, dim3(nb, nb), dim3(256), 0, (hipStream_t)stream, z, sim, B, n);
    return dm_launch_status("dm_pair_msd");
}

extern "C" int dm_pair_msd_backward(const float *z, const float *g_sim, float *dz, int B, int n, void *stream)
{
    DM_REQUIRE(z && g_sim && dz && B > 0 && n > 0, "dm_pair_msd_backward: bad argument");
    DM_REQUIRE((long long)B * n < (1LL << 31), "dm_pair_msd_backward: tensor too large for 32-bit offsets");
    hipLaunchKernelGGL(pair_msd_backward_kernel, dim3((n + 255) / 256, (B + PM_T - 1) / PM_T), dim3(256), 0,
                       (hipStream_t)stream, z, g_sim, dz, B, n);
    return dm_launch_status("dm_pair_msd_backward");
}

// ================================================================================================================
// The whole time-matching term on the matrix pipe (vq_vae.py:324-332, vae.py:322-336).
//
//   sim_ij = mean_d (z_i - z_j)^2 = (G_ii + G_jj - 2 G_ij) / n,   G = Z Z^T        (B x B x n GEMM, f32 MFMA)
//   loss   = sum_ij sim_ij tm_ij                                                   (mode 0, vq_vae.py:331)
//          = mean_ij v_ij, v = sim * w(tm), tm == 0: v = max(v + margin, 0)        (mode 1, vae.py:327-336)
//   S_ij   = dloss/dsim_ij + dloss/dsim_ji          (formed by the epilogue: the backward needs nothing else)
//   dz_i   = (2/n) (rowsum(S)_i z_i - sum_j S_ij z_j)                              (B x n x B GEMM, f32 MFMA)
//
// The reference materialises a (B, B, n) tensor for this (9.7 GB at its example batch of 768); the first version here
// formed the differences on the VALU (3 B^2 n operations, two LDS reads per multiply).  The Gram form costs 2 B^2 n on
// v_mfma_f32_16x16x4_f32; its cancellation error is ~ c u (|z_i|^2 + |z_j|^2) / n ABSOLUTE on sim (K split into chunks
// whose partial sums are added in double): harmless for a pair of unrelated cells, whose distance is of the order of the
// norms, but the pairs this loss exists for -- adjacent frames of ONE cell, tm in {1, 2}, weight_matching = 100 in the
// reference's example configuration (config_example.yml:164) -- lie close together, where |a|^2 + |b|^2 - 2ab has
// cancelled most of its bits (a pair at 1e-3 relative distance keeps none).  The reference takes differences first
// (vae.py:441-455).  So the Gram value is a FILTER, as in the VectorQuantizer kernel: a pair whose Gram distance is below
// TM_NEAR x (|z_i|^2 + |z_j|^2) (relative distance under 25 %) is re-evaluated from differences -- sum_d (z_i - z_j)^2
// by the whole wave, fp32 products added in double -- in the epilogue, and its gradient term S_ij (z_i - z_j) is taken
// from differences too (tm_near_backward_kernel) instead of the second GEMM, where rowsum(S) z_i - sum_j S_ij z_j
// cancels the same way.  Every other pair keeps a relative error <= c u / TM_NEAR ~ 3e-6 on sim.
//
// Two forms of the forward: the SQUARE one (a whole batch; half the tiles, each pair formed once for both orientations) and
// the ROW-RANGE one (data parallel: one rank's rows r0 .. r0 + R - 1 of a global batch of B against all of it).  They are
// thin kernels around the same pieces -- tm_gram_tile / tm_gram_store, tm_pair and its helpers -- and one host path
// (tm_forward, tm_backward: the square backward is the range (0, B)), so every pair is formed from the same operands by the
// same arithmetic: S and dz of a row range are rows of the square call's, to the bit.
// Layout: state and count kernels; the Gram kernels; the per-pair arithmetic; the epilogues; the backward; the host side.
namespace {

constexpr int TM_T = 64;          // 64 x 64 output tile per workgroup: 4 waves, 32 x 32 each (2 x 2 MFMA tiles)
constexpr int TM_KC = 32;         // K staged per step
constexpr int TM_LDA = TM_KC + 2; // LDS row stride of a K-major tile: == 2 (mod 32) banks, conflict-free operand reads

// ---- the sparse form (mode 0 only).  vq_vae.py:331 sums sim * time_matching_mat: a pair with a zero entry adds nothing to the
// loss or to its gradient, and the relation matrix of a batch holds a handful of entries per row (the frames of one
// trajectory).  state[0] = number of nonzero entries of tm (tm_count_kernel); when it is at most TM_SPARSE_ROW per row
// every kernel below reads that and the two GEMMs fall away: the Gram kernel returns, the epilogue takes EVERY related
// pair from differences (the path of the near pairs: exact, as the reference computes them), the gradient kernel writes its
// `add` operand through, and tm_near_backward_kernel adds the pairs' gradient row by row.  The decision is taken on the
// device: nothing for the host to wait for, the same launches in a captured step whatever the matrix holds.
constexpr int TM_SPARSE_ROW = 32;
__device__ __forceinline__ bool tm_sparse(const int *state, int B) { return state && state[0] <= TM_SPARSE_ROW * B; }
// The state block: 4 header words ([0] = the count above) and a map of the far part of S, one int per (panel of 64 rows,
// chunk of 32 columns), nonzero where the block holds a nonzero -- written by the epilogue (plain stores of 1: every writer
// writes the same value, so no read-modify-write on words that a dense S has thousands of workgroups aiming at), read by the
// gradient product, which only multiplies those chunks.  In the z16 / z32 form (mode 1) every pair has a distance to evaluate
// (the hinge on unrelated pairs), but an unrelated pair beyond the margin carries no gradient: S is as sparse as the relation
// matrix again once training has pushed such pairs apart.  A skipped chunk is all zeros: the sums are the same to the bit.
constexpr int TM_STATE_HDR = 4;
__host__ __device__ inline int tm_map_chunks(int B) { return (B + TM_KC - 1) / TM_KC; }
__device__ __forceinline__ void tm_map_set(int *map, int B, int row, int col)
{
    map[(row / TM_T) * tm_map_chunks(B) + col / TM_KC] = 1;
}

__global__ __launch_bounds__(256) void tm_state_clear_kernel(int *__restrict__ state, int ints)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < ints) state[i] = 0;
}

__global__ __launch_bounds__(256) void tm_count_kernel(const float *__restrict__ tm, long long BB, int *__restrict__ state)
{
    __shared__ int s_cnt[4];
    int c = 0;
    if ((BB & 3) == 0) {                                   // 16 bytes per lane and step
        const f32x4 *__restrict__ t4 = reinterpret_cast<const f32x4 *>(tm);
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < (BB >> 2); e += (long long)gridDim.x * 256) {
            const f32x4 v = t4[e];
            c += (int)(v.x != 0.f) + (int)(v.y != 0.f) + (int)(v.z != 0.f) + (int)(v.w != 0.f);
        }
    } else {
        for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < BB; e += (long long)gridDim.x * 256) c += tm[e] != 0.f;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(state, (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]));      // (integers: any order)
}

// One 64 x 64 tile of Gram partials: acc = sum_{k in [k_lo, k_hi)} z[i] z[j] for the rows i0 .. i0 + 63 (< ilim) against
// the rows j0 .. j0 + 63 (< jlim), in the wave layout of tm_gram_kernel.  Every entry is the same sequence of MFMA steps
// whatever the tile's origin, and a product does not care which of its factors is the A operand: the rectangular form
// (tm_gram_rows_kernel) therefore forms the very values of the square one.
__device__ __forceinline__ void tm_gram_tile(const float *__restrict__ z, int n, int i0, int ilim, int j0, int jlim, int k_lo,
                                             int k_hi, float *sA, float *sB, f32x4 (&acc)[2][2])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int lr = threadIdx.x >> 3, lq = threadIdx.x & 7;     // staging: 8 threads per row, 32 rows per pass
    // register-staged prefetch: the loads of K chunk c + 1 are in flight during the products of chunk c (round 4; the
    // load -> barrier -> products form left every chunk's round trip exposed: 54 TFLOP/s at B = 768, n = 4096)
    f32x4 va[2], vb[2];
    auto issue = [&](int k0) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int r = lr + 32 * pass;
            va[pass] = (f32x4){0.f, 0.f, 0.f, 0.f}; vb[pass] = va[pass];
            if (k0 < k_hi && i0 + r < ilim) va[pass] = *reinterpret_cast<const f32x4 *>(z + (long long)(i0 + r) * n + k0 + 4 * lq);
            if (k0 < k_hi && j0 + r < jlim) vb[pass] = *reinterpret_cast<const f32x4 *>(z + (long long)(j0 + r) * n + k0 + 4 * lq);
        }
    };
    issue(k_lo);
    for (int k0 = k_lo; k0 < k_hi; k0 += TM_KC) {
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int r = lr + 32 * pass;
            *reinterpret_cast<f32x2 *>(sA + r * TM_LDA + 4 * lq) = (f32x2){va[pass].x, va[pass].y};
            *reinterpret_cast<f32x2 *>(sA + r * TM_LDA + 4 * lq + 2) = (f32x2){va[pass].z, va[pass].w};
            *reinterpret_cast<f32x2 *>(sB + r * TM_LDA + 4 * lq) = (f32x2){vb[pass].x, vb[pass].y};
            *reinterpret_cast<f32x2 *>(sB + r * TM_LDA + 4 * lq + 2) = (f32x2){vb[pass].z, vb[pass].w};
        }
        __syncthreads();
        issue(k0 + TM_KC);
        const float *pa = sA + (wr * 32 + (lane & 15)) * TM_LDA + (lane >> 4);
        const float *pb = sB + (wc * 32 + (lane & 15)) * TM_LDA + (lane >> 4);
#pragma unroll
        for (int ks = 0; ks < TM_KC; ks += 4) {
            const float a0 = pa[ks], a1 = pa[16 * TM_LDA + ks], b0 = pb[ks], b1 = pb[16 * TM_LDA + ks];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}

// store(i, j, value) for the 16 entries a thread holds of the tile at (i0, j0) after tm_gram_tile
template <class Store>
__device__ __forceinline__ void tm_gram_store(const f32x4 (&acc)[2][2], int i0, int j0, Store store)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                store(i0 + wr * 32 + a * 16 + (lane >> 4) * 4 + r, j0 + wc * 32 + b * 16 + (lane & 15), acc[a][b][r]);
}

// The square form.  P[ks][i][j] = sum_{d in split ks} z[i][d] z[j][d] for the tiles ON AND ABOVE the diagonal: G is symmetric
// and the epilogue reads one orientation of every entry (P[min][max]), so the nt (nt - 1) / 2 tiles below the diagonal are
// never formed -- at B = 2048 that is 496 of 1024 workgroups (blockIdx.x walks the upper triangle row by row)
__global__ __launch_bounds__(256) void tm_gram_kernel(const float *__restrict__ z, float *__restrict__ P, int B, int n, int klen,
                                                      int nt, const int *__restrict__ state)
{
    __shared__ float sA[TM_T * TM_LDA], sB[TM_T * TM_LDA];
    if (tm_sparse(state, B)) return;                       // (uniform) the epilogue will not read P
    int tcol = blockIdx.x, trow = 0;
    for (int len = nt; tcol >= len; --len) { tcol -= len; ++trow; }    // (uniform: at most nt scalar steps)
    tcol += trow;
    const int i0 = trow * TM_T, j0 = tcol * TM_T;
    const int k_lo = blockIdx.z * klen, k_hi = min(n, k_lo + klen);
    f32x4 acc[2][2];
    tm_gram_tile(z, n, i0, B, j0, B, k_lo, k_hi, sA, sB, acc);
    float *__restrict__ Pk = P + (long long)blockIdx.z * B * B;
    tm_gram_store(acc, i0, j0, [=](int i, int j, float v) {
        if (i < B && j < B) Pk[(long long)i * B + j] = v;
    });
}

// The row-range form (data parallel: one rank's rows r0 .. r0 + R - 1 of a global batch of B).  P[ks][i - r0][j] for the R
// rows against all B columns (tiles of 64 rows from r0, of 64 columns from 0), and behind them one workgroup per 64 x 64
// diagonal tile of the whole batch for the Gram diagonal D[ks][g] (the epilogue needs G_jj of every column; only the
// diagonal of those tiles is stored).  The same K split as the square call's: every entry is the square form's, to the bit.
__global__ __launch_bounds__(256) void tm_gram_rows_kernel(const float *__restrict__ z, float *__restrict__ P, float *__restrict__ D,
                                                           int B, int n, int klen, int r0, int R, int ntr, int nt,
                                                           const int *__restrict__ state)
{
    __shared__ float sA[TM_T * TM_LDA], sB[TM_T * TM_LDA];
    if (tm_sparse(state, B)) return;                       // (uniform) the epilogue will not read P or D
    const int k_lo = blockIdx.z * klen, k_hi = min(n, k_lo + klen);
    const bool diag = (int)blockIdx.x >= ntr * nt;
    const int i0 = diag ? (blockIdx.x - ntr * nt) * TM_T : r0 + (blockIdx.x / nt) * TM_T;
    const int j0 = diag ? i0 : (blockIdx.x % nt) * TM_T;
    f32x4 acc[2][2];
    tm_gram_tile(z, n, i0, diag ? B : r0 + R, j0, B, k_lo, k_hi, sA, sB, acc);
    tm_gram_store(acc, i0, j0, [=](int i, int j, float v) {
        if (diag) {
            if (i == j && i < B) D[(long long)blockIdx.z * B + i] = v;
        } else if (i < r0 + R && j < B) {
            P[((long long)blockIdx.z * R + (i - r0)) * B + j] = v;
        }
    });
}

struct TmParams { int mode; float w_a, w_t, w_n, margin; };

__device__ __forceinline__ void tm_value(const TmParams &p, float sim, float tm, float inv_count, double &val, float &dsim)
{
    if (p.mode == 0) { val = (double)(sim * tm); dsim = tm; return; }
    const float w = tm == 2.f ? p.w_a : (tm == 1.f ? p.w_t : (tm == 0.f ? p.w_n : tm));
    float v = sim * w, live = 1.f;
    if (tm == 0.f) {                                      // hinge on the non-related pairs (vae.py:333-335)
        v = v + p.margin;
        live = v >= 0.f ? 1.f : 0.f;
        v = v > 0.f ? v : 0.f;
    }
    val = (double)v * (double)inv_count;
    dsim = w * live * inv_count;
}

constexpr float TM_NEAR = 1.f / 16.f;   // Gram distance below this share of |z_i|^2 + |z_j|^2: re-evaluate from differences

// The near pairs (i, j0 + l) of a wave's lanes l (`near` set), one at a time, by the whole wave: sum of squared differences,
// 16 bytes per lane and step; lane l's `sim` receives its pair's value.  (z_i - z_j)^2 and (z_j - z_i)^2 are the same
// number: either orientation of a pair gives the same bits.
__device__ __forceinline__ void tm_near_sims(const float *__restrict__ z, int n, int i, int j0, bool near, int lane, float &sim)
{
    unsigned long long todo = __ballot(near);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int pj = j0 + l;                             // (the wave shares i: lane l's pair is (i, j0 + l))
        const float *__restrict__ zi = z + (long long)i * n, *__restrict__ zj = z + (long long)pj * n;
        double acc = 0.0;
        int d = 4 * lane;
        for (; d + 768 < n; d += 1024) {                    // four steps' loads in flight together (the sparse form lives here)
            f32x4 a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = *reinterpret_cast<const f32x4 *>(zi + d + 256 * u);
                b[u] = *reinterpret_cast<const f32x4 *>(zj + d + 256 * u);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {                   // (the same terms in the same order as the single steps below)
                const f32x4 df = a[u] - b[u];
                acc += (double)((df.x * df.x + df.y * df.y) + (df.z * df.z + df.w * df.w));
            }
        }
        for (; d < n; d += 256) {                          // n % 32 == 0: whole float4s
            const f32x4 a = *reinterpret_cast<const f32x4 *>(zi + d), b = *reinterpret_cast<const f32x4 *>(zj + d);
            const f32x4 df = a - b;
            acc += (double)((df.x * df.x + df.y * df.y) + (df.z * df.z + df.w * df.w));
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == l) sim = (float)(acc / (double)n);
    }
}

// ---- the epilogue.  Two kernels, the square form's and the row-range form's, around ONE body per pair and shared pieces:
// every pair (i, j) is formed from the same operands by the same instructions in both, so the rows' S and dz are rows of
// the square call's, to the bit.  The kernels differ in how a tile is found (triangle walk or rectangle), where the Gram
// diagonal is read (P[g][g] or D[g]), whether the mirrored entry is written through LDS, and whether the loss counts one
// orientation of a pair or both.

// sT[r][c] = tm[j0 + r][ib + c], rows i = ib + c below ihi: the pair's other orientation (tm need not be symmetric)
template <int TM_ER>
__device__ __forceinline__ void tm_stage_transposed(float (&sT)[TM_T][TM_ER + 1], const float *__restrict__ tm, int B, int j0,
                                                    int ib, int ihi)
{
#pragma unroll
    for (int k = 0; k < TM_T * TM_ER / 256; ++k) {
        const int e = threadIdx.x + 256 * k, r = e / TM_ER, c = e % TM_ER;
        sT[r][c] = (j0 + r < B && ib + c < ihi) ? tm[(long long)(j0 + r) * B + ib + c] : 0.f;
    }
}

// Gram diagonal of the workgroup's rows ib .. (s_gi) and of the tile's columns j0 .. (s_gj): split ks of G_gg lies at
// diag[ks * ks_stride + g * g_stride]; the chunk sums are added in double, in a fixed order
template <int TM_ER>
__device__ __forceinline__ void tm_gram_diagonal(const float *__restrict__ diag, long long ks_stride, long long g_stride,
                                                 int ksplit, int B, int ib, int j0, double (&s_gi)[TM_ER], double (&s_gj)[TM_T])
{
    if (threadIdx.x < TM_ER + TM_T) {
        const int g = threadIdx.x < TM_ER ? ib + (int)threadIdx.x : j0 + (int)threadIdx.x - TM_ER;
        double d = 0.0;
        if (g < B)
            for (int ks = 0; ks < ksplit; ++ks) d += (double)diag[ks * ks_stride + g * g_stride];
        if (threadIdx.x < TM_ER) s_gi[threadIdx.x] = d; else s_gj[threadIdx.x - TM_ER] = d;
    }
}

struct TmPair { double v_ij, v_ji; float far, near; };    // both orientations' loss terms; S_ij as its far and its near part

// The pair (i, j) of lane j - j0 (`have`: the thread has one; the whole wave calls, its lanes share i): t_ij, t_ji its two
// relation entries, gii / gjj the Gram diagonal, gram_ij(ks) split ks of G_ij.  sim from the Gram partials added in double
// (the sparse form: not at all), the near pairs from differences, the two loss terms, S_ij = dloss/dsim_ij + dloss/dsim_ji.
template <class GramIJ>
__device__ __forceinline__ TmPair tm_pair(const float *__restrict__ z, int n, const TmParams &p, float inv_count, bool sparse,
                                          bool have, int i, int j, int j0, int lane, float t_ij, float t_ji, double gii,
                                          double gjj, int ksplit, GramIJ gram_ij)
{
    float sim = 0.f;
    bool near = false;
    if (have && sparse) {                                  // every related pair from differences, nothing else matters
        near = i != j && (t_ij != 0.f || t_ji != 0.f);
    } else if (have) {
        double gij = 0.0;
        for (int ks = 0; ks < ksplit; ++ks) gij += (double)gram_ij(ks);
        const double d2 = gii + gjj - 2.0 * gij;
        sim = i == j ? 0.f : (float)(d2 / (double)n);
        near = i != j && !(d2 >= (double)TM_NEAR * (gii + gjj));    // (also when the Gram value is not finite)
    }
    tm_near_sims(z, n, i, j0, near, lane, sim);
    TmPair r = {0.0, 0.0, 0.f, 0.f};
    if (have) {
        float d_ij, d_ji;
        tm_value(p, sim, t_ij, inv_count, r.v_ij, d_ij);
        tm_value(p, sim, t_ji, inv_count, r.v_ji, d_ji);
        const float sij = d_ij + d_ji;
        r.far = near ? 0.f : sij;
        r.near = near ? sij : 0.f;
    }
    return r;
}

// The chunks of the far part this wave put a nonzero into, rows of panel `row`: its lanes span two chunks of columns from j0.
// mirror_row >= 0: the mirrored entries as well, rows mirror_row .., columns row ..
__device__ __forceinline__ void tm_map_mark(int *far_map, int B, bool any_far, int lane, int row, int j0, int mirror_row)
{
    if (!far_map) return;
    const unsigned long long bal = __ballot(any_far);
    if (lane == 0) {
        if (bal & 0xffffffffull) tm_map_set(far_map, B, row, j0);
        if (bal >> 32) tm_map_set(far_map, B, row, j0 + 32);
        if (bal && mirror_row >= 0) tm_map_set(far_map, B, mirror_row, row);
    }
}

template <int TM_ER>
__device__ __forceinline__ void tm_store_slab(double val, double *s_red, double *__restrict__ loss_slabs)
{
    const double tot = block_sum(val, s_red);
    if (threadIdx.x == 0) {
        const long long slab = (long long)blockIdx.x * (TM_T / TM_ER) + blockIdx.y;
        loss_slabs[2 * slab] = tot; loss_slabs[2 * slab + 1] = 0.0;
    }
}

// The square form: the 64 x 64 tiles ON OR ABOVE the diagonal (the tiles tm_gram_kernel forms), TM_T / TM_ER workgroups per
// tile (TM_ER rows i each), one thread per TM_ER / 4 of its pairs (i, j), i <= j: BOTH orientations of the loss term -- the
// pair's two entries of tm -- and S_ij = S_ji written to both places, the mirrored entries through LDS.  (The first form, one
// thread per entry of the (B, B) matrix, read P and tm across the diagonal with a stride of B floats between lanes: 0.22 of
// the 0.38 ms forward at B = 2048.)  S: (2, B, B), the far part (for the gradient GEMM) and the near part (for
// tm_near_backward_kernel); loss partials per workgroup.
// TM_ER = 16 rows, or 4 where 16 would leave most of the chip without a workgroup (tm_er: fewer than 64 tiles)
template <int TM_ER>
__global__ __launch_bounds__(256) void tm_epilogue_kernel(const float *__restrict__ z, const float *__restrict__ P, int ksplit,
                                                          const float *__restrict__ tm, int B, int n, TmParams p,
                                                          float *__restrict__ S, double *__restrict__ loss_slabs, int nt,
                                                          const int *__restrict__ state, int *__restrict__ far_map)
{
    __shared__ float sT[TM_T][TM_ER + 1];                // tm[j0 + r][ib + c]
    __shared__ float sF[TM_ER][TM_T + 1], sN[TM_ER][TM_T + 1];   // far / near part of S by (i - ib, j - j0)
    __shared__ double s_gi[TM_ER], s_gj[TM_T];           // Gram diagonal of the workgroup's rows i and the tile's columns j
    __shared__ double s_red[4];
    int tcol = blockIdx.x, trow = 0;
    for (int len = nt; tcol >= len; --len) { tcol -= len; ++trow; }
    tcol += trow;
    const int ib = trow * TM_T + blockIdx.y * TM_ER, j0 = tcol * TM_T;
    const bool diag = trow == tcol;
    const long long BB = (long long)B * B;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, lane = tx;
    tm_stage_transposed<TM_ER>(sT, tm, B, j0, ib, B);
    const bool sparse = tm_sparse(state, B);
    if (!sparse) tm_gram_diagonal<TM_ER>(P, BB, B + 1, ksplit, B, ib, j0, s_gi, s_gj);
    __syncthreads();
    const float inv_count = p.mode == 0 ? 1.f : 1.f / (float)BB;
    const int j = j0 + tx;
    const double gjj = s_gj[tx];
    double val = 0.0;
    bool any_far = false;
#pragma unroll
    for (int q = 0; q < TM_ER / 4; ++q) {
        const int il = ty + 4 * q, i = ib + il;
        const bool have = i < B && j < B && (!diag || i <= j);
        const long long o = (long long)i * B + j;
        const TmPair r = tm_pair(z, n, p, inv_count, sparse, have, i, j, j0, lane, have ? tm[o] : 0.f, sT[tx][il], s_gi[il], gjj,
                                 ksplit, [=](int ks) { return P[ks * BB + o]; });
        if (have) {
            val += i == j ? r.v_ij : r.v_ij + r.v_ji;
            S[o] = r.far;
            S[BB + o] = r.near;
        }
        sF[il][tx] = r.far;
        sN[il][tx] = r.near;
        any_far |= r.far != 0.f;
    }
    tm_map_mark(far_map, B, any_far, lane, ib, j0, j0);    // (the mirrored entries: rows j0 .. j0 + 63, columns ib .. ib + TM_ER - 1)
    __syncthreads();
    // the mirrored entries: S[j][i] = S[i][j] (the loss counts both orientations of a pair, so S is symmetric)
#pragma unroll
    for (int k = 0; k < TM_T * TM_ER / 256; ++k) {
        const int e = threadIdx.x + 256 * k, jl = e / TM_ER, c = e % TM_ER;
        const int jj = j0 + jl, ii = ib + c;               // entry (jj, ii) <- the value at (i = ii, j = jj)
        if (jj < B && ii < B && (!diag || ii < jj)) {
            S[(long long)jj * B + ii] = sF[c][jl];
            S[BB + (long long)jj * B + ii] = sN[c][jl];
        }
    }
    tm_store_slab<TM_ER>(val, s_red, loss_slabs);
}

// The row-range form: one workgroup per (tile of 64 rows i among the R, tile of 64 columns j) and TM_ER rows of it: thread =
// column j, TM_ER / 4 of the rows.  S (2, R, B) for the rows, the far-block map by (panel of 64 of the R rows, chunk of 32
// columns), and the rows' OWN loss terms, sum_{i in rows, j} v_ij (mode 1 normalised by B * B): the shares of a partition
// of the rows add up to the square call's loss.
template <int TM_ER>
__global__ __launch_bounds__(256) void tm_epilogue_rows_kernel(const float *__restrict__ z, const float *__restrict__ P,
                                                               const float *__restrict__ D, int ksplit,
                                                               const float *__restrict__ tm, int B, int n, int r0, int R, TmParams p,
                                                               float *__restrict__ S, double *__restrict__ loss_slabs, int nt,
                                                               const int *__restrict__ state, int *__restrict__ far_map)
{
    __shared__ float sT[TM_T][TM_ER + 1];                // tm[j0 + r][ib + c]
    __shared__ double s_gi[TM_ER], s_gj[TM_T];
    __shared__ double s_red[4];
    const int trow = blockIdx.x / nt, tcol = blockIdx.x % nt;
    const int il0 = trow * TM_T + blockIdx.y * TM_ER;   // first local row of the workgroup
    const int ib = r0 + il0, j0 = tcol * TM_T, rhi = r0 + R;
    const long long RB = (long long)R * B;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, lane = tx;
    tm_stage_transposed<TM_ER>(sT, tm, B, j0, ib, rhi);
    const bool sparse = tm_sparse(state, B);
    if (!sparse) tm_gram_diagonal<TM_ER>(D, B, 1, ksplit, B, ib, j0, s_gi, s_gj);
    __syncthreads();
    const float inv_count = p.mode == 0 ? 1.f : 1.f / (float)((long long)B * B);
    const int j = j0 + tx;
    const double gjj = s_gj[tx];
    double val = 0.0;
    bool any_far = false;
#pragma unroll
    for (int q = 0; q < TM_ER / 4; ++q) {
        const int il = ty + 4 * q, i = ib + il;
        const bool have = i < rhi && j < B;
        const long long o = (long long)(i - r0) * B + j;
        const TmPair r = tm_pair(z, n, p, inv_count, sparse, have, i, j, j0, lane, have ? tm[(long long)i * B + j] : 0.f,
                                 sT[tx][il], s_gi[il], gjj, ksplit, [=](int ks) { return P[ks * RB + o]; });
        if (have) {
            val += r.v_ij;
            S[o] = r.far;
            S[RB + o] = r.near;
        }
        any_far |= r.far != 0.f;
    }
    tm_map_mark(far_map, B, any_far, lane, il0, j0, -1);
    tm_store_slab<TM_ER>(val, s_red, loss_slabs);
}

// dz[i][d] += scale * g * sum_{j near i} S_ij (z[i][d] - z[j][d]): the near pairs' share of the gradient from differences.
// One workgroup per row i; rows without a near pair (the usual case for most of them) leave after reading their S row.
// The row's nonzero columns are compacted first (thread t owns the columns [t c, (t + 1) c): counts, a scan, the list in
// ascending j -- a fixed order), so the sum walks the row's pairs, not its B columns (in the sparse form EVERY related pair
// comes through here).  Dynamic LDS: B floats (the row) + B 16-bit column numbers.
// Rows of Snear and dz are the rows r0 .. r0 + gridDim.x - 1 of the batch (the square form: r0 = 0, all B of them); z is the
// whole batch.
__global__ __launch_bounds__(256) void tm_near_backward_kernel(const float *__restrict__ z, const float *__restrict__ Snear,
                                                               const float *__restrict__ g_dev, float scale,
                                                               float *__restrict__ dz, int B, int n, int r0)
{
    extern __shared__ float s_row[];                       // S_near[i][0..B)
    unsigned short *s_col = reinterpret_cast<unsigned short *>(s_row + B);
    __shared__ int s_cnt[256];
    __shared__ int s_any;
    const int i = blockIdx.x;
    if (threadIdx.x == 0) s_any = 0;
    __syncthreads();
    bool any = false;
    for (int j = threadIdx.x; j < B; j += 256) {
        const float v = Snear[(long long)i * B + j];
        s_row[j] = v;
        any |= v != 0.f;
    }
    if (any) s_any = 1;
    __syncthreads();
    if (!s_any) return;
    const int c = (B + 255) / 256, j_lo = threadIdx.x * c, j_hi = min(B, j_lo + c);
    int mine = 0;
    for (int j = j_lo; j < j_hi; ++j) mine += s_row[j] != 0.f;
    s_cnt[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                     // inclusive scan
        const int v = threadIdx.x >= o ? s_cnt[threadIdx.x - o] : 0;
        __syncthreads();
        s_cnt[threadIdx.x] += v;
        __syncthreads();
    }
    int at = s_cnt[threadIdx.x] - mine;
    const int total = s_cnt[255];
    for (int j = j_lo; j < j_hi; ++j)
        if (s_row[j] != 0.f) s_col[at++] = (unsigned short)j;
    __syncthreads();
    const float sc = scale * (g_dev ? g_dev[0] : 1.f);
    const float *__restrict__ zi = z + (long long)(r0 + i) * n;
    for (int d = 4 * threadIdx.x; d < n; d += 1024) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(zi + d);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < total; ++k) {                   // ascending j: a fixed order
            const int j = s_col[k];
            acc += s_row[j] * (a - *reinterpret_cast<const f32x4 *>(z + (long long)j * n + d));
        }
        // (product and sum rounded separately: what is already in dz may be another gradient of the latents -- the `add` operand
        //  of the call -- and the sum has to come out as the separate elementwise add of the unfused path does)
        f32x4 *o = reinterpret_cast<f32x4 *>(dz + (long long)i * n + d);
        const f32x4 cur = *o;
        *o = (f32x4){__fadd_rn(cur.x, __fmul_rn(sc, acc.x)), __fadd_rn(cur.y, __fmul_rn(sc, acc.y)),
                     __fadd_rn(cur.z, __fmul_rn(sc, acc.z)), __fadd_rn(cur.w, __fmul_rn(sc, acc.w))};
    }
}

// dz[i][d] = scale * g * (rowsum(S)_i z[i][d] - sum_j S_ij z[j][d]);  64 rows x 64 columns per workgroup, K = B
constexpr int TM_LDZ = TM_T + 16;  // LDS row stride of the [j][d] tile: == 16 (mod 32), conflict-free B-operand reads
// add (optional): another gradient of the same latents (the quantiser's), added here instead of in a pass of its own.
// Rows i of S, dz and add are the R rows r0 .. r0 + R - 1 of the batch (the square form: r0 = 0, R = B); z is the whole batch.
__global__ __launch_bounds__(256) void tm_backward_kernel(const float *__restrict__ z, const float *__restrict__ S,
                                                          const float *__restrict__ g_dev, float scale,
                                                          float *__restrict__ dz, int B, int n, const float *__restrict__ add,
                                                          const int *__restrict__ state, int r0, int R)
{
    __shared__ float sS[TM_T * TM_LDA], sZ[TM_KC * TM_LDZ], s_rs[TM_T], s_part[256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wr = wave >> 1, wc = wave & 1;
    const int i0 = blockIdx.y * TM_T, d0 = blockIdx.x * TM_T;
    // the chunks of 32 columns of S to multiply: all of them, or (state) those the epilogue marked for this panel of rows, in
    // ascending order either way
    __shared__ unsigned short s_list[512];                 // (B <= 16384)
    __shared__ int s_scan[256];
    const int nchunks = (B + TM_KC - 1) / TM_KC;
    int nl;
    {
        const int *__restrict__ map = state ? state + TM_STATE_HDR + blockIdx.y * nchunks : nullptr;
        auto live = [&](int c) { return c < nchunks && (!map || map[c] != 0); };
        const int c_lo = 2 * threadIdx.x;                  // thread t owns chunks 2t, 2t + 1
        const int mine = (int)live(c_lo) + (int)live(c_lo + 1);
        s_scan[threadIdx.x] = mine;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int v = threadIdx.x >= o ? s_scan[threadIdx.x - o] : 0;
            __syncthreads();
            s_scan[threadIdx.x] += v;
            __syncthreads();
        }
        int at = s_scan[threadIdx.x] - mine;
        if (live(c_lo)) s_list[at++] = (unsigned short)c_lo;
        if (live(c_lo + 1)) s_list[at] = (unsigned short)(c_lo + 1);
        nl = s_scan[255];
        __syncthreads();
    }
    {   // row sums of S for the tile's 64 rows: 4 threads per row, fixed order (a skipped chunk would have added zeros)
        const int r = threadIdx.x >> 2, q = threadIdx.x & 3;
        float a = 0.f;
        if (i0 + r < R) {
            const float *__restrict__ row = S + (long long)(i0 + r) * B;
            for (int li = 0; li < nl; ++li) {
                const int k0 = TM_KC * s_list[li];
                if ((B & 3) == 0) {                          // 16 bytes per load: a quarter of the round trips of this serial prologue
#pragma unroll
                    for (int h = 0; h < TM_KC; h += 16) {
                        const int j = k0 + h + 4 * q;
                        if (j < B) {
                            const f32x4 v = *reinterpret_cast<const f32x4 *>(row + j);
                            a += (v.x + v.y) + (v.z + v.w);
                        }
                    }
                } else {
                    for (int j = k0 + q; j < min(B, k0 + TM_KC); j += 4) a += row[j];
                }
            }
        }
        s_part[threadIdx.x] = a;
        __syncthreads();
        if (q == 0) s_rs[r] = (s_part[threadIdx.x] + s_part[threadIdx.x + 1]) + (s_part[threadIdx.x + 2] + s_part[threadIdx.x + 3]);
        __syncthreads();                                    // (with no chunk to multiply nothing else stands before their use)
    }
    if (nl == 0 && ((((uintptr_t)dz | (uintptr_t)add) & 15) == 0)) {
        // (uniform) nothing marked for these rows -- the sparse form, or a panel of unrelated samples: dz = add + 0 * z, the
        // value the general path below would store (a zero row sum times a finite latent), 16 bytes per lane, z not read
        for (int e = threadIdx.x; e < TM_T * (TM_T / 4); e += 256) {
            const int i = i0 + e / (TM_T / 4), d = d0 + 4 * (e % (TM_T / 4));
            if (i < R && d < n) {
                const long long o = (long long)i * n + d;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (add) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4 *>(add + o);
                    v = (f32x4){__fadd_rn(a4.x, 0.f), __fadd_rn(a4.y, 0.f), __fadd_rn(a4.z, 0.f), __fadd_rn(a4.w, 0.f)};
                }
                *reinterpret_cast<f32x4 *>(dz + o) = v;
            }
        }
        return;
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int lr = threadIdx.x >> 3, lq = threadIdx.x & 7;     // S tile staging: 8 threads per row (32 columns j)
    const int zr = threadIdx.x >> 4, zq = threadIdx.x & 15;    // Z tile staging: 16 threads per row (64 columns d)
    // register-staged prefetch of the next K chunk, as in tm_gram_kernel
    float sv[2][4];
    f32x4 zv[2];
    const bool s_vec = (B & 3) == 0;                           // rows of S are 16-byte aligned: one load instead of four
    auto issue = [&](int k0) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int r = lr + 32 * pass;
            if (s_vec) {
                f32x4 t = {0.f, 0.f, 0.f, 0.f};
                if (i0 + r < R && k0 + 4 * lq < B) t = *reinterpret_cast<const f32x4 *>(S + (long long)(i0 + r) * B + k0 + 4 * lq);
                sv[pass][0] = t.x; sv[pass][1] = t.y; sv[pass][2] = t.z; sv[pass][3] = t.w;
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int j = k0 + 4 * lq + u;
                    sv[pass][u] = (i0 + r < R && j < B) ? S[(long long)(i0 + r) * B + j] : 0.f;
                }
            }
            const int jr = zr + 16 * pass;
            zv[pass] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (k0 + jr < B && d0 + 4 * zq < n) zv[pass] = *reinterpret_cast<const f32x4 *>(z + (long long)(k0 + jr) * n + d0 + 4 * zq);
        }
    };
    if (nl > 0) issue(TM_KC * s_list[0]);
    for (int li = 0; li < nl; ++li) {
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int r = lr + 32 * pass;
            *reinterpret_cast<f32x2 *>(sS + r * TM_LDA + 4 * lq) = (f32x2){sv[pass][0], sv[pass][1]};
            *reinterpret_cast<f32x2 *>(sS + r * TM_LDA + 4 * lq + 2) = (f32x2){sv[pass][2], sv[pass][3]};
            *reinterpret_cast<f32x4 *>(sZ + (zr + 16 * pass) * TM_LDZ + 4 * zq) = zv[pass];
        }
        __syncthreads();
        issue(li + 1 < nl ? TM_KC * s_list[li + 1] : B);    // (past the end: every lane's guard fails, nothing is loaded)
        const float *pa = sS + (wr * 32 + (lane & 15)) * TM_LDA + (lane >> 4);
        const float *pb = sZ + (lane >> 4) * TM_LDZ + wc * 32 + (lane & 15);
#pragma unroll
        for (int ks = 0; ks < TM_KC; ks += 4) {
            const float a0 = pa[ks], a1 = pa[16 * TM_LDA + ks], b0 = pb[ks * TM_LDZ], b1 = pb[ks * TM_LDZ + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    const float sc = scale * (g_dev ? g_dev[0] : 1.f);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int il = wr * 32 + a * 16 + (lane >> 4) * 4 + r, i = i0 + il, d = d0 + wc * 32 + b * 16 + (lane & 15);
                if (i < R && d < n) {
                    const long long o = (long long)i * n + d;
                    const float t = sc * (s_rs[il] * z[(long long)(r0 + i) * n + d] - acc[a][b][r]);
                    dz[o] = add ? __fadd_rn(add[o], t) : t;            // (rounded like the separate elementwise add it replaces)
                }
            }
}

// ---- the host side: ONE forward launch and ONE backward launch behind the seven entry points
constexpr int tm_tiles(int rows) { return (rows + TM_T - 1) / TM_T; }
int tm_square_tiles(int B) { return tm_tiles(B) * (tm_tiles(B) + 1) / 2; }      // the upper triangle of tiles
int tm_rows_tiles(int B, int R) { return tm_tiles(R) * tm_tiles(B); }
// rows per epilogue workgroup: 16, or 4 where 16 would leave most of the chip without a workgroup
int tm_er(int tiles) { return 4 * tiles >= 256 ? 16 : 4; }

int tm_ksplit(int B, int n)                               // of the square call, whichever form asks: the same partial sums
{
    int ks = 1024 / tm_square_tiles(B);
    const int maxks = n / 256 > 0 ? n / 256 : 1;
    if (ks > maxks) ks = maxks;
    if (ks > 64) ks = 64;
    if (ks < 1) ks = 1;
    return ks;
}

// What an entry point asks of the shared launch
struct TmCall {
    const char *name;               // the entry point, for messages
    int r0, R;                      // rows r0 .. r0 + R - 1 of the batch (the square form: 0, B)
    bool square;                    // the triangle walk over the whole batch; else the R x B rectangle
    bool need_state, need_add;      // optional operands this entry point requires
};

int tm_forward(const TmCall &c, const float *z, const float *tm, int B, int n, int mode, float w_a, float w_t, float w_n,
               float margin, float *workspace, int64_t workspace_floats, float *S, double *loss_slabs, int32_t *state,
               void *stream)
{
    DM_REQUIRE(B > 0 && c.R >= 0 && c.r0 >= 0 && c.r0 + c.R <= B, "%s: rows [%d, %d) outside a batch of %d", c.name, c.r0,
               c.r0 + c.R, B);
    if (c.R == 0) return 0;                                // an empty shard: no rows, no loss terms, nothing launched
    DM_REQUIRE(z && tm && workspace && S && loss_slabs && (state || !c.need_state), "%s: NULL pointer", c.name);
    DM_REQUIRE(dm_time_matching_supported(B, n), "%s: latent length %d is not a multiple of %d", c.name, n, TM_KC);
    DM_REQUIRE(mode == 0 || mode == 1, "%s: mode %d", c.name, mode);
    DM_REQUIRE((long long)B * n < (1LL << 31) && (long long)B * B < (1LL << 31), "%s: tensor too large", c.name);
    DM_REQUIRE(workspace_floats >= (c.square ? dm_time_matching_workspace_floats(B, n)
                                             : dm_time_matching_rows_workspace_floats(B, c.R, n)),
               "%s: workspace too small", c.name);
    // (tm_count_kernel and the epilogue read tm 16 bytes at a time where B * B is a multiple of four)
    DM_REQUIRE((((uintptr_t)tm | (uintptr_t)z | (uintptr_t)S) & 15) == 0, "%s: z, tm and S must be 16-byte aligned", c.name);
    hipStream_t s = (hipStream_t)stream;
    const int ks = tm_ksplit(B, n), nt = tm_tiles(B), ntr = tm_tiles(c.R);
    const int tiles = c.square ? tm_square_tiles(B) : tm_rows_tiles(B, c.R);
    int klen = (n + ks - 1) / ks;
    klen = (klen + TM_KC - 1) / TM_KC * TM_KC;
    // the sparse form: mode 0 only (in mode 1 the unrelated pairs carry the hinge term), and only where the caller keeps a state
    // word for the backward call to read; the count always starts from zero
    const int *st = nullptr;
    int *far_map = nullptr;
    if (state) {
        // (cleared by a kernel of this stream, ordered like every other launch of the call)
        const int ints = dm_time_matching_rows_state_ints(B, c.R);
        hipLaunchKernelGGL(tm_state_clear_kernel, dim3((ints + 255) / 256), dim3(256), 0, s, (int *)state, ints);
        far_map = (int *)state + TM_STATE_HDR;
        if (mode == 0) {
            // the count is of the WHOLE relation block, in the row-range form too: every rank decides alike
            const long long BB = (long long)B * B;
            const long long units = (BB & 3) == 0 ? BB >> 2 : BB;
            const int grid = (int)((units + 255) / 256 < 2048 ? (units + 255) / 256 : 2048);
            hipLaunchKernelGGL(tm_count_kernel, dim3(grid), dim3(256), 0, s, tm, BB, (int *)state);
            st = (const int *)state;
        }
    }
    float *P = workspace, *D = workspace + (long long)ks * c.R * B;      // (D: the row-range form's)
    if (c.square)
        hipLaunchKernelGGL(tm_gram_kernel, dim3(tiles, 1, ks), dim3(256), 0, s, z, P, B, n, klen, nt, st);
    else
        hipLaunchKernelGGL(tm_gram_rows_kernel, dim3(tiles + nt, 1, ks), dim3(256), 0, s, z, P, D, B, n, klen, c.r0, c.R, ntr, nt, st);
    const TmParams p{mode, w_a, w_t, w_n, margin};
    auto epilogue = [&](auto er) {
        constexpr int ER = decltype(er)::value;
        const dim3 grid(tiles, TM_T / ER);
        if (c.square)
            hipLaunchKernelGGL(tm_epilogue_kernel<ER>, grid, dim3(256), 0, s, z, P, ks, tm, B, n, p, S, loss_slabs, nt, st, far_map);
        else
            hipLaunchKernelGGL(tm_epilogue_rows_kernel<ER>, grid, dim3(256), 0, s, z, P, D, ks, tm, B, n, c.r0, c.R, p, S,
                               loss_slabs, nt, st, far_map);
    };
    if (tm_er(tiles) == 16) epilogue(std::integral_constant<int, 16>()); else epilogue(std::integral_constant<int, 4>());
    return dm_launch_status(c.name);
}

// Rows of S, dz and add are the rows of the call; the square entry points are the range (0, B)
int tm_backward(const TmCall &c, const float *z, const float *S, const float *g_loss_dev, float scale, const float *add,
                float *dz, int B, int n, const int32_t *state, void *stream)
{
    DM_REQUIRE(B > 0 && c.R >= 0 && c.r0 >= 0 && c.r0 + c.R <= B, "%s: rows [%d, %d) outside a batch of %d", c.name, c.r0,
               c.r0 + c.R, B);
    if (c.R == 0) return 0;
    DM_REQUIRE(z && S && dz && (state || !c.need_state) && (add || !c.need_add), "%s: NULL pointer", c.name);
    DM_REQUIRE(dm_time_matching_supported(B, n), "%s: latent length %d is not a multiple of %d", c.name, n, TM_KC);
    DM_REQUIRE((long long)B * n < (1LL << 31), "%s: tensor too large", c.name);
    DM_REQUIRE(B <= 16384, "%s: batch %d too large (a row of S is staged in LDS)", c.name, B);
    // (rows of S are read as 16-byte vectors where B is a multiple of four; z tiles always are)
    DM_REQUIRE((((uintptr_t)S | (uintptr_t)z) & 15) == 0, "%s: z and S must be 16-byte aligned", c.name);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(tm_backward_kernel, dim3(tm_tiles(n), tm_tiles(c.R)), dim3(256), 0, s, z, S, g_loss_dev,
                       scale * 2.f / (float)n, dz, B, n, add, (const int *)state, c.r0, c.R);
    const size_t near_lds = (size_t)B * (sizeof(float) + sizeof(unsigned short));
    if (near_lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void *)tm_near_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)near_lds);
        if (e != hipSuccess) {
            dm_set_error("%s: cannot reserve %zu bytes of LDS: %s", c.name, near_lds, hipGetErrorString(e));
            return (int)e;
        }
    }
    hipLaunchKernelGGL(tm_near_backward_kernel, dim3((unsigned)c.R), dim3(256), near_lds, s, z, S + (long long)c.R * B, g_loss_dev,
                       scale * 2.f / (float)n, dz, B, n, c.r0);
    return dm_launch_status(c.name);
}

}  // namespace

extern "C" int dm_time_matching_supported(int B, int n) { return (B > 0 && n > 0 && n % TM_KC == 0) ? 1 : 0; }

extern "C" int64_t dm_time_matching_workspace_floats(int B, int n)
{
    // Gram slabs.  The 4 * blocks + 4 floats behind them held the epilogue's loss partials before those got a buffer of
    // their own (loss_slabs); nothing reads them now, the reported size is kept as callers know it.
    const long long blocks = ((long long)B * B + 255) / 256;
    return (long long)tm_ksplit(B, n) * B * B + 4 * blocks + 4;
}

extern "C" int64_t dm_time_matching_rows_workspace_floats(int B, int R, int n)
{
    // Gram partials of the rows + the Gram diagonal of the whole batch, per K split (the square call's split of B)
    return (long long)tm_ksplit(B, n) * ((long long)R * B + B);
}

// the state block: the header and one map word per (panel of 64 rows, chunk of 32 columns)
extern "C" int dm_time_matching_state_ints(int B) { return dm_time_matching_rows_state_ints(B, B); }
extern "C" int dm_time_matching_rows_state_ints(int B, int R) { return TM_STATE_HDR + tm_tiles(R) * tm_map_chunks(B); }

// one slab per epilogue workgroup
extern "C" int dm_time_matching_num_slabs(int B) { return (TM_T / tm_er(tm_square_tiles(B))) * tm_square_tiles(B); }
extern "C" int dm_time_matching_rows_num_slabs(int B, int R)
{
    return R <= 0 ? 0 : (TM_T / tm_er(tm_rows_tiles(B, R))) * tm_rows_tiles(B, R);
}

extern "C" int dm_time_matching_forward(const float *z, const float *tm, int B, int n, int mode, float w_a, float w_t,
                                        float w_n, float margin, float *workspace, int64_t workspace_floats, float *S,
                                        double *loss_slabs, void *stream)
{
    return tm_forward({"dm_time_matching_forward", 0, B, true, false, false}, z, tm, B, n, mode, w_a, w_t, w_n, margin, workspace,
                      workspace_floats, S, loss_slabs, nullptr, stream);
}

extern "C" int dm_time_matching_forward_state(const float *z, const float *tm, int B, int n, int mode, float w_a, float w_t,
                                              float w_n, float margin, float *workspace, int64_t workspace_floats, float *S,
                                              double *loss_slabs, int32_t *state, void *stream)
{
    return tm_forward({"dm_time_matching_forward_state", 0, B, true, true, false}, z, tm, B, n, mode, w_a, w_t, w_n, margin,
                      workspace, workspace_floats, S, loss_slabs, state, stream);
}

extern "C" int dm_time_matching_forward_rows(const float *z, const float *tm, int B, int r0, int R, int n, int mode, float w_a,
                                             float w_t, float w_n, float margin, float *workspace, int64_t workspace_floats,
                                             float *S, double *loss_slabs, int32_t *state, void *stream)
{
    return tm_forward({"dm_time_matching_forward_rows", r0, R, false, true, false}, z, tm, B, n, mode, w_a, w_t, w_n, margin,
                      workspace, workspace_floats, S, loss_slabs, state, stream);
}

extern "C" int dm_time_matching_backward(const float *z, const float *S, const float *g_loss_dev, float scale, float *dz,
                                         int B, int n, void *stream)
{
    return tm_backward({"dm_time_matching_backward", 0, B, true, false, false}, z, S, g_loss_dev, scale, nullptr, dz, B, n, nullptr,
                       stream);
}

extern "C" int dm_time_matching_backward_add(const float *z, const float *S, const float *g_loss_dev, float scale,
                                             const float *add, float *dz, int B, int n, void *stream)
{
    return tm_backward({"dm_time_matching_backward_add", 0, B, true, false, true}, z, S, g_loss_dev, scale, add, dz, B, n, nullptr,
                       stream);
}

extern "C" int dm_time_matching_backward_state(const float *z, const float *S, const float *g_loss_dev, float scale,
                                               const float *add, float *dz, int B, int n, const int32_t *state, void *stream)
{
    return tm_backward({"dm_time_matching_backward_state", 0, B, true, true, false}, z, S, g_loss_dev, scale, add, dz, B, n, state,
                       stream);
}

extern "C" int dm_time_matching_backward_rows(const float *z, const float *S, const float *g_loss_dev, float scale,
                                              const float *add, float *dz, int B, int r0, int R, int n, const int32_t *state,
                                              void *stream)
{
    return tm_backward({"dm_time_matching_backward_rows", r0, R, false, true, false}, z, S, g_loss_dev, scale, add, dz, B, n, state,
                       stream);
}
