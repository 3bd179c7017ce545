// pca.hip -- the latent PCA of run_dim_reduction.py on the device: column sums, the centred Gram matrix and the projection.
//
// Reference: run_dim_reduction.py:14-50 (fit_PCA: sklearn PCA(0.5, svd_solver='auto').fit_transform of the pooled latents)
// and :52-92 (process_PCA: pca.transform of one well's latents).  scikit-learn's covariance route forms X^T X and subtracts
// n mu mu^T afterwards; here the data are centred in the operand load instead, so the fp32 products never see the 30-sigma
// offsets latents carry, and the fp64 finalisation (dynamorph_amd/pca.py) only corrects for the fp32 rounding of the shift.
//
// Every kernel reads X (N x F, fp32, row-major, leading dimension ld) as it lies; F <= DM_PCA_MAX_FEATURES.
//   colsum     per-column fp64 sums, rows split into a fixed number of ranges, the ranges added in order (bit-stable).
//   gram       G = (X - s)^T (X - s), upper-triangular 128 x 128 tile pairs on v_mfma_f32_32x32x2_f32; fp32 within a slab of
//              DM_PCA_GRAM_SLAB_ROWS rows, slabs added in fp64 registers in row order, row splits reduced in order from an
//              fp64 workspace and mirrored into the full F x F matrix (no atomics anywhere: repeated launches are bit-equal).
//   transform  Y = (X - s) V^T for V (k x F), k <= DM_PCA_MAX_COMPONENTS, 64-row tiles on v_mfma_f32_16x16x4_f32.
#include "dm_common.h"

namespace {

// ------------------------------------------------------------------------------------------------- column sums
constexpr int CS_BLOCK = 256;           // one column per thread, 256 consecutive columns per workgroup
constexpr int CS_TARGET_BLOCKS = 2048;  // row ranges: enough workgroups to keep every CU's loads in flight

struct ColsumPlan { int bx; int P; long long rows_per; };

ColsumPlan colsum_plan(long long N, int F)
{
    ColsumPlan p;
    p.bx = (F + CS_BLOCK - 1) / CS_BLOCK;
    long long P = (CS_TARGET_BLOCKS + p.bx - 1) / p.bx;
    const long long max_p = (N + 255) / 256;            // at least 256 rows per range
    if (P > max_p) P = max_p;
    if (P < 1) P = 1;
    p.rows_per = (N + P - 1) / P;
    p.P = (int)((N + p.rows_per - 1) / p.rows_per);
    return p;
}

__global__ __launch_bounds__(CS_BLOCK) void colsum_partial_kernel(const float *__restrict__ X, long long N, int F, long long ld,
                                                                  long long rows_per, double *__restrict__ part)
{
    const int col = blockIdx.x * CS_BLOCK + threadIdx.x;
    if (col >= F) return;
    const long long r0 = (long long)blockIdx.y * rows_per;
    const long long r1 = r0 + rows_per < N ? r0 + rows_per : N;
    const float *p = X + col;
    double s = 0.0;
    long long r = r0;
    for (; r + 8 <= r1; r += 8) {       // eight loads in flight, added in row order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(p + (r + u) * ld);
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)v[u];
    }
    for (; r < r1; ++r) s += (double)p[r * ld];
    part[(long long)blockIdx.y * F + col] = s;
}

__global__ __launch_bounds__(CS_BLOCK) void colsum_final_kernel(const double *__restrict__ part, int P, int F,
                                                                double *__restrict__ sums)
{
    const int col = blockIdx.x * CS_BLOCK + threadIdx.x;
    if (col >= F) return;
    double s = 0.0;
    for (int q = 0; q < P; ++q) s += part[(long long)q * F + col];
    sums[col] = s;
}

// ----------------------------------------------------------------------------------------------- Gram matrix
constexpr int GT = 128;                 // tile edge: a workgroup computes one 128 x 128 block of G
constexpr int GCH = 16;                 // rows per LDS stage (8 k-steps of the 32x32x2 instruction)
constexpr int GLW = GT + 32;            // LDS row stride: the two lane halves of a read (rows k, k+1) land 32 banks apart
constexpr int GR = DM_PCA_GRAM_SLAB_ROWS;
static_assert(GR % GCH == 0, "a slab is a whole number of LDS stages");
constexpr int G_SLOTS = 256;            // workgroups resident at once on a 256-CU part (one per CU: 316 registers per lane)

struct GramPlan { int T; long long pairs; long long nslabs; int S; long long slabs_per; };

// The row split depends on (N, F) only, never on the device, so the summation order -- and the result -- is a function of
// the data alone.  S is the split whose last wave of workgroups is fullest (ties: the smaller S), capped by the slabs there
// are and by a 2 GiB workspace.
GramPlan gram_plan(long long N, int F)
{
    GramPlan p;
    p.T = (F + GT - 1) / GT;
    p.pairs = (long long)p.T * (p.T + 1) / 2;
    p.nslabs = (N + GR - 1) / GR;
    const long long tile_bytes = (long long)GT * GT * 8;
    int best = 1;
    double best_eff = 0.0;
    for (int s = 1; s <= 64 && s <= p.nslabs; ++s) {
        if (s > 1 && (long long)s * p.pairs * tile_bytes > (2LL << 30)) break;
        const long long blocks = (long long)s * p.pairs;
        const double eff = (double)blocks / (double)(((blocks + G_SLOTS - 1) / G_SLOTS) * G_SLOTS);
        if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
    }
    p.slabs_per = (p.nslabs + best - 1) / best;
    p.S = (int)((p.nslabs + p.slabs_per - 1) / p.slabs_per);
    return p;
}

__device__ __forceinline__ void pair_of(int p, int T, int &ti, int &tj)
{
    ti = 0;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    tj = ti + p;
}

// Four consecutive columns c .. c+3 of row r, centred; zero outside the matrix (never -shift: padding adds nothing).
template <bool V4>
__device__ __forceinline__ f32x4 load_centred4(const float *__restrict__ X, long long r, int c, long long N, int F,
                                               long long ld, f32x4 sh)
{
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < N) {
        const float *p = X + r * ld + c;
        if (V4 && c + 3 < F) {
            v = *(const f32x4 *)p;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < F) v[e] = p[e];
        }
        v -= sh;
    }
    return v;
}

__device__ __forceinline__ f32x4 shift4(const float *__restrict__ shift, int c, int F)
{
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (shift) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < F) s[e] = shift[c + e];
    }
    return s;
}

// Workgroup (pair, split): 4 waves, wave w owns the 64 x 64 quarter (w >> 1, w & 1) of the tile as 2 x 2 accumulators of
// the 32x32x2 instruction.  A thread stages columns 4 * (tid & 31) .. +3 of rows (tid >> 5) and (tid >> 5) + 8 of both
// operands; the next stage's rows are loaded into registers before the current stage's products are issued.
template <bool V4>
__global__ __launch_bounds__(256) void gram_kernel(const float *__restrict__ X, long long N, int F, long long ld,
                                                   const float *__restrict__ shift, int T, long long slabs_per,
                                                   double *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) float lds[2][2][GCH * GLW];
    int ti, tj;
    pair_of(blockIdx.x, T, ti, tj);
    const int I = ti * GT, J = tj * GT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int c4 = (tid & 31) * 4, rr = tid >> 5;
    const f32x4 sa = shift4(shift, I + c4, F), sb = shift4(shift, J + c4, F);

    const long long row_begin = (long long)blockIdx.y * slabs_per * GR;
    long long row_end = row_begin + slabs_per * GR;
    if (row_end > N) row_end = N;
    const long long nstages = (row_end - row_begin + GCH - 1) / GCH;

    f32x4 ra[2], rb[2];
    auto fetch = [&](long long stage) {
        const long long r = row_begin + stage * GCH + rr;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const long long rq = r + 8 * q;
            ra[q] = load_centred4<V4>(X, rq < row_end ? rq : N, I + c4, N, F, ld, sa);
            rb[q] = load_centred4<V4>(X, rq < row_end ? rq : N, J + c4, N, F, ld, sb);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            *(f32x4 *)&lds[buf][0][(rr + 8 * q) * GLW + c4] = ra[q];
            *(f32x4 *)&lds[buf][1][(rr + 8 * q) * GLW + c4] = rb[q];
        }
    };

    typedef float f32x16 __attribute__((ext_vector_type(16)));
    f32x16 acc[2][2];
    double dacc[2][2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            acc[i][j] = (f32x16){};
#pragma unroll
            for (int e = 0; e < 16; ++e) dacc[i][j][e] = 0.0;
        }

    fetch(0);
    stash(0);
    __syncthreads();
    constexpr int STAGES_PER_SLAB = GR / GCH;
    for (long long st = 0; st < nstages; ++st) {
        const int buf = (int)(st & 1);
        if (st + 1 < nstages) fetch(st + 1);
        const float *A = lds[buf][0], *B = lds[buf][1];
        const int koff = (lane >> 5) * GLW + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < GCH / 2; ++kk) {
            const int o = 2 * kk * GLW + koff;
            const float a0 = A[o + wm * 64], a1 = A[o + wm * 64 + 32];
            const float b0 = B[o + wn * 64], b1 = B[o + wn * 64 + 32];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (st + 1 < nstages) stash(buf ^ 1);
        __syncthreads();
        if ((st + 1) % STAGES_PER_SLAB == 0 || st + 1 == nstages) {     // slab done: fold it into fp64, row order
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) dacc[i][j][e] += (double)acc[i][j][e];
                    acc[i][j] = (f32x16){};
                }
        }
    }
    // C/D map of the 32x32 instructions: column lane & 31, row (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    double *out = ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (GT * GT);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                const int col = wn * 64 + j * 32 + (lane & 31);
                out[row * GT + col] = dacc[i][j][e];
            }
}

// G[i][j] (+)= sum over splits, in order, of tile pair (min, max) -- the lower triangle read transposed.
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double *__restrict__ ws, int S, long long pairs, int T, int F,
                                                          double *__restrict__ G, int accumulate)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= F || j >= F) return;
    int a = i, b = j;
    if (a / GT > b / GT) { a = j; b = i; }
    const int ta = a / GT, tb = b / GT;
    const long long p = (long long)ta * T - (long long)ta * (ta - 1) / 2 + (tb - ta);
    const long long off = p * (GT * GT) + (a % GT) * GT + (b % GT);
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += ws[(long long)s * pairs * (GT * GT) + off];
    double *g = G + (long long)i * F + j;
    *g = accumulate ? *g + v : v;
}

// ------------------------------------------------------------------------------------------------- transform
constexpr int TR_ROWS = 64;             // rows of X per workgroup (16 per wave)
constexpr int TR_FC = 64;               // features per LDS stage (16 k-steps of the 16x16x4 instruction)
constexpr int TR_LW = TR_FC + 4;        // LDS row stride: lane (row l & 15, k l >> 4) -> bank 4 (l & 15) + (l >> 4), all 64 distinct

// Workgroup (row tile, component tile of KT): X and V stages in LDS, each wave 16 rows x KT components as KT / 16
// accumulators of v_mfma_f32_16x16x4_f32 (B[k][j] = V[j][f]); the next stage is loaded into registers before the products.
template <int KT, bool V4>
__global__ __launch_bounds__(256) void transform_kernel(const float *__restrict__ X, long long N, int F, long long ld,
                                                        const float *__restrict__ shift, const float *__restrict__ V, int k,
                                                        float *__restrict__ Y)
{
    __shared__ __attribute__((aligned(16))) float xs[TR_ROWS * TR_LW];
    __shared__ __attribute__((aligned(16))) float vs[KT * TR_LW];
    constexpr int XQ = TR_ROWS * TR_FC / 4 / 256;       // float4 per thread: X stage
    constexpr int VQ = KT * TR_FC / 4 / 256;            // V stage
    const long long row0 = (long long)blockIdx.x * TR_ROWS;
    const int j0 = blockIdx.y * KT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c4 = (tid & 15) * 4, rr = tid >> 4;       // 16 threads per 64-feature row segment

    f32x4 rx[XQ], rv[VQ];
    auto fetch = [&](int f0) {
        const f32x4 sh = shift4(shift, f0 + c4, F);
#pragma unroll
        for (int q = 0; q < XQ; ++q) rx[q] = load_centred4<V4>(X, row0 + rr + 16 * q, f0 + c4, N, F, ld, sh);
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < VQ; ++q) {                      // components past k: zero rows
            const int j = j0 + rr + 16 * q;
            rv[q] = load_centred4<false>(V, j, f0 + c4, k, F, F, z);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < XQ; ++q) *(f32x4 *)&xs[(rr + 16 * q) * TR_LW + c4] = rx[q];
#pragma unroll
        for (int q = 0; q < VQ; ++q) *(f32x4 *)&vs[(rr + 16 * q) * TR_LW + c4] = rv[q];
    };

    f32x4 acc[KT / 16];
#pragma unroll
    for (int t = 0; t < KT / 16; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int f0 = 0; f0 < F; f0 += TR_FC) {
        stash();
        __syncthreads();
        if (f0 + TR_FC < F) fetch(f0 + TR_FC);
        const int ao = (w * 16 + (lane & 15)) * TR_LW + (lane >> 4);
        const int bo = (lane & 15) * TR_LW + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < TR_FC / 4; ++kk) {
            const float a = xs[ao + 4 * kk];
#pragma unroll
            for (int t = 0; t < KT / 16; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, vs[bo + t * 16 * TR_LW + 4 * kk], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map of the 16x16 instructions: column lane & 15, row 4 (lane >> 4) + e
#pragma unroll
    for (int t = 0; t < KT / 16; ++t) {
        const int j = j0 + t * 16 + (lane & 15);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long r = row0 + w * 16 + 4 * (lane >> 4) + e;
            if (r < N && j < k) Y[r * k + j] = acc[t][e];
        }
    }
}

int check_x(const char *who, const float *X, long long N, int F, long long ld)
{
    DM_REQUIRE(X, "%s: X is NULL", who);
    DM_REQUIRE(N >= 1, "%s: N = %lld rows, need >= 1", who, N);
    DM_REQUIRE(F >= 1 && F <= DM_PCA_MAX_FEATURES, "%s: F = %d features, supported 1 .. %d", who, F, DM_PCA_MAX_FEATURES);
    DM_REQUIRE(ld >= F, "%s: leading dimension %lld < F = %d", who, ld, F);
    return 0;
}

bool vec4_ok(const float *X, long long ld) { return ld % 4 == 0 && ((uintptr_t)X & 15) == 0; }

template <int KT>
void launch_transform(bool v4, unsigned gx, hipStream_t s, const float *X, long long N, int F, long long ld,
                      const float *shift, const float *V, int k, float *Y)
{
    const dim3 grid(gx, (k + KT - 1) / KT);
    if (v4) hipLaunchKernelGGL((transform_kernel<KT, true>), grid, dim3(256), 0, s, X, N, F, ld, shift, V, k, Y);
    else hipLaunchKernelGGL((transform_kernel<KT, false>), grid, dim3(256), 0, s, X, N, F, ld, shift, V, k, Y);
}

}  // namespace

extern "C" int64_t dm_pca_colsum_workspace_bytes(int64_t N, int F)
{
    if (N < 1 || F < 1 || F > DM_PCA_MAX_FEATURES) return -1;
    const ColsumPlan p = colsum_plan(N, F);
    return (int64_t)p.P * F * (int64_t)sizeof(double);
}

extern "C" int dm_pca_colsum(const float *X, int64_t N, int F, int64_t ld, double *sums, void *workspace,
                             int64_t workspace_bytes, void *stream)
{
    if (check_x("dm_pca_colsum", X, N, F, ld)) return -1;
    DM_REQUIRE(sums && workspace, "dm_pca_colsum: sums / workspace is NULL");
    DM_REQUIRE(workspace_bytes >= dm_pca_colsum_workspace_bytes(N, F), "dm_pca_colsum: workspace of %lld bytes, need %lld",
               (long long)workspace_bytes, (long long)dm_pca_colsum_workspace_bytes(N, F));
    const ColsumPlan p = colsum_plan(N, F);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(p.bx, p.P), dim3(CS_BLOCK), 0, s, X, (long long)N, F, (long long)ld,
                       p.rows_per, (double *)workspace);
    hipLaunchKernelGGL(colsum_final_kernel, dim3(p.bx), dim3(CS_BLOCK), 0, s, (const double *)workspace, p.P, F, sums);
    return dm_launch_status("dm_pca_colsum");
}

extern "C" int64_t dm_pca_gram_workspace_bytes(int64_t N, int F)
{
    if (N < 1 || F < 1 || F > DM_PCA_MAX_FEATURES) return -1;
    const GramPlan p = gram_plan(N, F);
    return (int64_t)p.S * p.pairs * GT * GT * (int64_t)sizeof(double);
}

extern "C" int dm_pca_gram(const float *X, int64_t N, int F, int64_t ld, const float *shift, double *G, int accumulate,
                           void *workspace, int64_t workspace_bytes, void *stream)
{
    if (check_x("dm_pca_gram", X, N, F, ld)) return -1;
    DM_REQUIRE(G && workspace, "dm_pca_gram: G / workspace is NULL");
    DM_REQUIRE(workspace_bytes >= dm_pca_gram_workspace_bytes(N, F), "dm_pca_gram: workspace of %lld bytes, need %lld",
               (long long)workspace_bytes, (long long)dm_pca_gram_workspace_bytes(N, F));
    const GramPlan p = gram_plan(N, F);
    hipStream_t s = (hipStream_t)stream;
    double *ws = (double *)workspace;
    if (vec4_ok(X, ld))
        hipLaunchKernelGGL(gram_kernel<true>, dim3((unsigned)p.pairs, p.S), dim3(256), 0, s, X, (long long)N, F,
                           (long long)ld, shift, p.T, p.slabs_per, ws);
    else
        hipLaunchKernelGGL(gram_kernel<false>, dim3((unsigned)p.pairs, p.S), dim3(256), 0, s, X, (long long)N, F,
                           (long long)ld, shift, p.T, p.slabs_per, ws);
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((F + 63) / 64, (F + 3) / 4), dim3(256), 0, s, (const double *)ws, p.S,
                       p.pairs, p.T, F, G, accumulate ? 1 : 0);
    return dm_launch_status("dm_pca_gram");
}

extern "C" int dm_pca_transform(const float *X, int64_t N, int F, int64_t ld, const float *shift, const float *V, int k,
                                float *Y, void *stream)
{
    if (check_x("dm_pca_transform", X, N, F, ld)) return -1;
    DM_REQUIRE(V && Y, "dm_pca_transform: V / Y is NULL");
    DM_REQUIRE(k >= 1 && k <= DM_PCA_MAX_COMPONENTS, "dm_pca_transform: k = %d components, supported 1 .. %d", k,
               DM_PCA_MAX_COMPONENTS);
    hipStream_t s = (hipStream_t)stream;
    const unsigned gx = (unsigned)((N + TR_ROWS - 1) / TR_ROWS);
    const bool v4 = vec4_ok(X, ld);
    if (k <= 16) launch_transform<16>(v4, gx, s, X, N, F, ld, shift, V, k, Y);
    else if (k <= 32) launch_transform<32>(v4, gx, s, X, N, F, ld, shift, V, k, Y);
    else launch_transform<64>(v4, gx, s, X, N, F, ld, shift, V, k, Y);
    return dm_launch_status("dm_pca_transform");
}
