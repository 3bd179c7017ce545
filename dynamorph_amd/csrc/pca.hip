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
// Wider latents (VQ_VAE_z32: 65536 features), N <= DM_PCA_WIDE_MAX_SAMPLES rows, F <= DM_PCA_WIDE_MAX_FEATURES:
//   rowgram    K = (X - s)(X - s)^T (N x N), knn_gram_kernel's loop on upper-triangular tile pairs of the rows; fp32 within
//              a slab of DM_PCA_ROWGRAM_SLAB_FEATURES features, slabs in fp64 registers in feature order, the work split over
//              feature ranges that are reduced in order from an fp64 workspace (or, one range, stored directly and mirrored).
//   components V = W (X - s) (k x F float64) for W (k x N): the transform turned round, fp32 within slabs of
//              DM_PCA_COMPONENTS_SLAB_ROWS rows, fp64 across them.
#include "dm_common.h"
#include "gram_tile.h"

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
constexpr int GR = DM_PCA_GRAM_SLAB_ROWS;   // gram_kernel stages ROWS: its slab is its own (gram_tile.h: the tile, the stage)
static_assert(GR % GT_CH == 0, "a slab is a whole number of LDS stages");
constexpr long long RG_DIRECT_PAIRS = 4 * GT_SLOTS; // rowgram: from here on the tile pairs fill the part, no feature split

// Tile pairs of an `extent`-wide symmetric matrix, the inner dimension `depth` in slabs of `slab` (gram_tile.h: split_plan).
struct GramPlan { int T; long long pairs; int S; long long slabs_per; };

GramPlan tile_pair_plan(long long extent, long long depth, int slab, long long direct_pairs)
{
    GramPlan p;
    p.T = (int)((extent + GT - 1) / GT);
    p.pairs = (long long)p.T * (p.T + 1) / 2;
    const SplitPlan sp = split_plan(p.pairs, (depth + slab - 1) / slab, direct_pairs);
    p.S = sp.S;
    p.slabs_per = sp.slabs_per;
    return p;
}

// G (F x F): the rows are split.
GramPlan gram_plan(long long N, int F) { return tile_pair_plan(F, N, GR, 0); }
// K (N x N): the features are split.  Few tile pairs (N = 2000: 136 for 256 CUs) need the split; RG_DIRECT_PAIRS or more:
// S = 1, which needs no workspace: the kernel stores its tile into K and rowgram_mirror_kernel completes K.
GramPlan rowgram_plan(long long N, long long F) { return tile_pair_plan(N, F, GT_SLAB, RG_DIRECT_PAIRS); }

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
    __shared__ __attribute__((aligned(16))) float lds[2][2][GT_CH * GT_LW];
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
    const long long nstages = (row_end - row_begin + GT_CH - 1) / GT_CH;

    f32x4 ra[2], rb[2];
    auto fetch = [&](long long stage) {
        const long long r = row_begin + stage * GT_CH + rr;
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
            *(f32x4 *)&lds[buf][0][(rr + 8 * q) * GT_LW + c4] = ra[q];
            *(f32x4 *)&lds[buf][1][(rr + 8 * q) * GT_LW + c4] = rb[q];
        }
    };

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
    constexpr int STAGES_PER_SLAB = GR / GT_CH;
    for (long long st = 0; st < nstages; ++st) {
        const int buf = (int)(st & 1);
        if (st + 1 < nstages) fetch(st + 1);
        const float *A = lds[buf][0], *B = lds[buf][1];
        const int koff = (lane >> 5) * GT_LW + (lane & 31);
#pragma unroll
        for (int kk = 0; kk < GT_CH / 2; ++kk) {
            const int o = 2 * kk * GT_LW + koff;
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
    double *out = ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (GT * GT);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = gt_row(wm * 64 + i * 32, e, lane);
                const int col = gt_col(wn * 64 + j * 32, lane);
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
    const long long off = pair_index(ta, tb, T) * (GT * GT) + (a % GT) * GT + (b % GT);
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

template <int KT>
void launch_transform(bool v4, unsigned gx, hipStream_t s, const float *X, long long N, int F, long long ld,
                      const float *shift, const float *V, int k, float *Y)
{
    const dim3 grid(gx, (k + KT - 1) / KT);
    if (v4) hipLaunchKernelGGL((transform_kernel<KT, true>), grid, dim3(256), 0, s, X, N, F, ld, shift, V, k, Y);
    else hipLaunchKernelGGL((transform_kernel<KT, false>), grid, dim3(256), 0, s, X, N, F, ld, shift, V, k, Y);
}

// ------------------------------------------------------------------------------- row Gram matrix (sample space)
// K = (X - s)(X - s)^T for latents wider than DM_PCA_MAX_FEATURES: the N x N side of the matrix the covariance route squares.

// Workgroup (tile pair ti <= tj of the rows, feature range y): knn_gram_kernel's loop with both operands taken from X.
// 4 waves, wave w owns the 64 x 64 quarter (w >> 1, w & 1) as 2 x 2 accumulators of the 32x32x2 instruction.  A thread stages
// features 4 (tid >> 6) .. + 3 of rows (tid & 63) and (tid & 63) + 64 of both tiles and stores them transposed
// ([feature][row]).  Two stages of loads are in flight during a stage's products: a fetch only loads -- the shift is
// subtracted when the registers go to LDS -- and it is unconditional and free of branches (past the range it repeats the
// last stage; SHIFT is a template parameter, and the 16-byte form V4 is launched on a multiple of four features, the host
// sends the one to three left over through the scalar form).  Rows past N repeat row N - 1 (their products are never
// stored); features past the range go to LDS as zeros.
// ws != NULL: the tile goes to ws[y][pair] (rowgram_reduce_kernel adds the ranges).  ws == NULL (one range): the entries
// with row <= column go straight into K, (+)=.
template <bool V4, bool SHIFT>
__global__ __launch_bounds__(256) void rowgram_kernel(const float *__restrict__ X, int N, int F, long long ld,
                                                      const float *__restrict__ shift, int T, long long slabs_per,
                                                      double *__restrict__ ws, double *__restrict__ K, int accumulate)
{
    __shared__ __attribute__((aligned(16))) float lds[2][2][GT_CH * GT_LW];
    int ti, tj;
    pair_of(blockIdx.x, T, ti, tj);
    const int I = ti * GT, J = tj * GT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int sr = tid & 63, sf = 4 * (tid >> 6);

    const long long fb = (long long)blockIdx.y * slabs_per * GT_SLAB;
    const int f_begin = (int)fb;
    const int f_end = (int)(fb + slabs_per * GT_SLAB < F ? fb + slabs_per * GT_SLAB : F);
    const int nstages = (f_end - f_begin + GT_CH - 1) / GT_CH;

    const float *arow[2], *brow[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int ra_ = I + sr + 64 * q, rb_ = J + sr + 64 * q;
        arow[q] = X + (long long)(ra_ < N ? ra_ : N - 1) * ld;
        brow[q] = X + (long long)(rb_ < N ? rb_ : N - 1) * ld;
    }

    f32x4 ra[2][2], rb[2][2], rs[2];
    auto fetch = [&](int stage, int slot) {
        const int f = f_begin + (stage < nstages ? stage : nstages - 1) * GT_CH + sf;
        rs[slot] = SHIFT ? row_load4_clamped<false>(shift, f, F) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            ra[slot][q] = row_load4_clamped<V4>(arow[q], f, F);
            rb[slot][q] = row_load4_clamped<V4>(brow[q], f, F);
        }
    };
    auto stash = [&](int stage, int slot, int buf) {
        const int f = f_begin + stage * GT_CH + sf;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const f32x4 va = ra[slot][q] - rs[slot], vb = rb[slot][q] - rs[slot];
#pragma unroll
            for (int e = 0; e < 4; ++e) {       // features past the range: zeros
                lds[buf][0][(sf + e) * GT_LW + sr + 64 * q] = f + e < f_end ? va[e] : 0.f;
                lds[buf][1][(sf + e) * GT_LW + sr + 64 * q] = f + e < f_end ? vb[e] : 0.f;
            }
        }
    };

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

    fetch(0, 0);
    fetch(1, 1);
    stash(0, 0, 0);
    __syncthreads();
    constexpr int STAGES_PER_SLAB = GT_SLAB / GT_CH;
    for (int st0 = 0; st0 < nstages; st0 += 2) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {           // stage st lives in register slot u and LDS buffer u
            const int st = st0 + u;
            if (st >= nstages) break;
            fetch(st + 2, u);                   // (slot u went to LDS one stage ago)
            __builtin_amdgcn_sched_barrier(0);  // the loads are issued here, not after the products
            const float *A = lds[u][0], *B = lds[u][1];
            const int koff = (lane >> 5) * GT_LW + (lane & 31);
#pragma unroll
            for (int kk = 0; kk < GT_CH / 2; ++kk) {
                const int o = 2 * kk * GT_LW + koff;
                const float a0 = A[o + wm * 64], a1 = A[o + wm * 64 + 32];
                const float b0 = B[o + wn * 64], b1 = B[o + wn * 64 + 32];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
            stash(st + 1, u ^ 1, u ^ 1);        // (unconditional like the fetch: past the end it stores zeros nobody reads)
            __syncthreads();
            if ((st + 1) % STAGES_PER_SLAB == 0 || st + 1 == nstages) {     // slab done: fold it into fp64, feature order
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
    }
    double *tile = ws ? ws + ((long long)blockIdx.y * gridDim.x + blockIdx.x) * (GT * GT) : nullptr;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = gt_row(wm * 64 + i * 32, e, lane);
                const int col = gt_col(wn * 64 + j * 32, lane);
                if (tile) {
                    tile[row * GT + col] = dacc[i][j][e];
                } else if (I + row <= J + col && J + col < N) {
                    double *k = K + (long long)(I + row) * N + (J + col);
                    *k = accumulate ? *k + dacc[i][j][e] : dacc[i][j][e];
                }
            }
}

// K[i][j] (+)= sum over the feature ranges, in order, of the entry (min, max) of the pair's tile.
__global__ __launch_bounds__(256) void rowgram_reduce_kernel(const double *__restrict__ ws, int S, long long pairs, int T, int N,
                                                             double *__restrict__ K, int accumulate)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= N || j >= N) return;
    const int a = i < j ? i : j, b = i < j ? j : i;
    const int ta = a / GT, tb = b / GT;
    const long long off = pair_index(ta, tb, T) * (GT * GT) + (a % GT) * GT + (b % GT);
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += ws[(long long)s * pairs * (GT * GT) + off];
    double *k = K + (long long)i * N + j;
    *k = accumulate ? *k + v : v;
}

// One range: the entries below the diagonal are copies of the ones the kernel stored above it.
__global__ __launch_bounds__(256) void rowgram_mirror_kernel(int N, double *__restrict__ K)
{
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= N || j >= i) return;
    K[(long long)i * N + j] = K[(long long)j * N + i];
}

// ------------------------------------------------------------------------------------------- components (sample space)
constexpr int CP_FT = 64;               // features per workgroup (16 per wave)
constexpr int CP_RC = 64;               // rows of X per LDS stage (16 k-steps of the 16x16x4 instruction)
constexpr int CP_XLW = CP_FT + 16;      // X stage [row][feature]: lane (feature l & 15, k l >> 4) -> bank 16 (l >> 4) + (l & 15)
constexpr int CP_WLW = CP_RC + 4;       // W stage [component][row]: lane (comp. l & 15, k l >> 4) -> bank 4 (l & 15) + (l >> 4)
constexpr int CP_SLAB = DM_PCA_COMPONENTS_SLAB_ROWS;
static_assert(CP_SLAB % CP_RC == 0, "a slab is a whole number of LDS stages");

// transform_kernel turned round: V = W (X - s), the rows of X are the inner dimension.  Workgroup (feature tile, component
// tile of KT): stages of 64 rows of X and of W in LDS, each wave 16 features x KT components as KT / 16 accumulators of
// v_mfma_f32_16x16x4_f32 (A[i][k] = W[j][n], B[k][j] = X[n][f] - s[f]); the next stage is loaded into registers before the
// products.  fp32 within a slab of CP_SLAB rows, the slabs added in float64 in row order and stored as they are.
template <int KT, bool V4>
__global__ __launch_bounds__(256) void components_kernel(const float *__restrict__ X, int N, int F, long long ld,
                                                         const float *__restrict__ shift, const float *__restrict__ W, int k,
                                                         double *__restrict__ V)
{
    __shared__ __attribute__((aligned(16))) float xs[CP_RC * CP_XLW];
    __shared__ __attribute__((aligned(16))) float wl[KT * CP_WLW];
    constexpr int XQ = CP_RC * CP_FT / 4 / 256;         // float4 per thread: X stage
    constexpr int WQ = KT * CP_RC / 256;                // floats per thread: W stage
    const int f0 = blockIdx.x * CP_FT, j0 = blockIdx.y * KT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c4 = (tid & 15) * 4, rr = tid >> 4;       // 16 threads per 64-feature row segment
    const f32x4 sh = shift4(shift, f0 + c4, F);

    f32x4 rx[XQ];
    float rw[WQ];
    auto fetch = [&](int n0) {
#pragma unroll
        for (int q = 0; q < XQ; ++q) rx[q] = load_centred4<V4>(X, n0 + rr + 16 * q, f0 + c4, N, F, ld, sh);
#pragma unroll
        for (int q = 0; q < WQ; ++q) {                      // components past k, rows past N: zeros
            const int j = j0 + w + 4 * q, n = n0 + lane;
            rw[q] = j < k && n < N ? W[(long long)j * N + n] : 0.f;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < XQ; ++q) *(f32x4 *)&xs[(rr + 16 * q) * CP_XLW + c4] = rx[q];
#pragma unroll
        for (int q = 0; q < WQ; ++q) wl[(w + 4 * q) * CP_WLW + lane] = rw[q];
    };

    f32x4 acc[KT / 16];
    double dacc[KT / 16][4];
#pragma unroll
    for (int t = 0; t < KT / 16; ++t) {
        acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) dacc[t][e] = 0.0;
    }
    fetch(0);
    for (int n0 = 0; n0 < N; n0 += CP_RC) {
        stash();
        __syncthreads();
        if (n0 + CP_RC < N) fetch(n0 + CP_RC);
        const int ao = (lane & 15) * CP_WLW + (lane >> 4);
        const int bo = (lane >> 4) * CP_XLW + w * 16 + (lane & 15);
#pragma unroll
        for (int kk = 0; kk < CP_RC / 4; ++kk) {
            const float b = xs[bo + 4 * kk * CP_XLW];
#pragma unroll
            for (int t = 0; t < KT / 16; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[ao + t * 16 * CP_WLW + 4 * kk], b, acc[t], 0, 0, 0);
        }
        __syncthreads();
        if ((n0 + CP_RC) % CP_SLAB == 0 || n0 + CP_RC >= N) {           // slab done: fold it into fp64, row order
#pragma unroll
            for (int t = 0; t < KT / 16; ++t) {
#pragma unroll
                for (int e = 0; e < 4; ++e) dacc[t][e] += (double)acc[t][e];
                acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    // C/D map of the 16x16 instructions: column (feature) lane & 15, row (component) 4 (lane >> 4) + e
    const int f = f0 + w * 16 + (lane & 15);
    if (f >= F) return;
#pragma unroll
    for (int t = 0; t < KT / 16; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j0 + t * 16 + 4 * (lane >> 4) + e;
            if (j < k) V[(long long)j * F + f] = dacc[t][e];
        }
}

template <int KT>
void launch_components(bool v4, hipStream_t s, const float *X, int N, int F, long long ld, const float *shift, const float *W,
                       int k, double *V)
{
    const dim3 grid((F + CP_FT - 1) / CP_FT, (k + KT - 1) / KT);
    if (v4) hipLaunchKernelGGL((components_kernel<KT, true>), grid, dim3(256), 0, s, X, N, F, ld, shift, W, k, V);
    else hipLaunchKernelGGL((components_kernel<KT, false>), grid, dim3(256), 0, s, X, N, F, ld, shift, W, k, V);
}

int check_wide_x(const char *who, const float *X, long long N, int F, long long ld)
{
    DM_REQUIRE(X, "%s: X is NULL", who);
    DM_REQUIRE(N >= 1 && N <= DM_PCA_WIDE_MAX_SAMPLES, "%s: N = %lld rows, supported 1 .. %d", who, N, DM_PCA_WIDE_MAX_SAMPLES);
    DM_REQUIRE(F >= 1 && F <= DM_PCA_WIDE_MAX_FEATURES, "%s: F = %d features, supported 1 .. %d", who, F,
               DM_PCA_WIDE_MAX_FEATURES);
    DM_REQUIRE(ld >= F, "%s: leading dimension %lld < F = %d", who, ld, F);
    return 0;
}

// One launch of the row Gram kernel and of what completes K behind it, on features [0, F) of X.
template <bool V4>
void launch_rowgram(hipStream_t s, const float *X, int N, int F, long long ld, const float *shift, double *K, int accumulate,
                    double *workspace)
{
    const GramPlan p = rowgram_plan(N, F);
    double *ws = p.S > 1 ? workspace : nullptr;
    const dim3 grid((unsigned)p.pairs, p.S), red((unsigned)((N + 63) / 64), (unsigned)((N + 3) / 4));
    if (shift)
        hipLaunchKernelGGL((rowgram_kernel<V4, true>), grid, dim3(256), 0, s, X, N, F, ld, shift, p.T, p.slabs_per, ws, K,
                           accumulate);
    else
        hipLaunchKernelGGL((rowgram_kernel<V4, false>), grid, dim3(256), 0, s, X, N, F, ld, shift, p.T, p.slabs_per, ws, K,
                           accumulate);
    if (ws)
        hipLaunchKernelGGL(rowgram_reduce_kernel, red, dim3(256), 0, s, (const double *)ws, p.S, p.pairs, p.T, N, K, accumulate);
    else
        hipLaunchKernelGGL(rowgram_mirror_kernel, red, dim3(256), 0, s, N, K);
}

int64_t rowgram_ws_bytes(long long N, int F)
{
    const GramPlan p = rowgram_plan(N, F);
    return p.S > 1 ? (int64_t)p.S * p.pairs * GT * GT * (int64_t)sizeof(double) : 0;
}

}  // namespace

// (the 16-byte form runs on F & ~3 features, the scalar form on all F or on the F & 3 left over: the larger need)
extern "C" int64_t dm_pca_rowgram_workspace_bytes(int64_t N, int F)
{
    if (N < 1 || N > DM_PCA_WIDE_MAX_SAMPLES || F < 1 || F > DM_PCA_WIDE_MAX_FEATURES) return -1;
    const int64_t a = rowgram_ws_bytes(N, F), b = F >= 4 ? rowgram_ws_bytes(N, F & ~3) : 0;
    return a > b ? a : b;
}

extern "C" int dm_pca_rowgram(const float *X, int64_t N, int F, int64_t ld, const float *shift, double *K, int accumulate,
                              void *workspace, int64_t workspace_bytes, void *stream)
{
    if (check_wide_x("dm_pca_rowgram", X, N, F, ld)) return -1;
    DM_REQUIRE(K, "dm_pca_rowgram: K is NULL");
    const int64_t need = dm_pca_rowgram_workspace_bytes(N, F);
    DM_REQUIRE(need == 0 || workspace, "dm_pca_rowgram: workspace is NULL");
    DM_REQUIRE(workspace_bytes >= need, "dm_pca_rowgram: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
               (long long)need);
    hipStream_t s = (hipStream_t)stream;
    double *ws = (double *)workspace;
    int acc = accumulate ? 1 : 0;
    const int Fv = vec4_ok(X, ld) ? F & ~3 : 0;         // the features the 16-byte form takes
    if (Fv) {
        launch_rowgram<true>(s, X, (int)N, Fv, ld, shift, K, acc, ws);
        acc = 1;
    }
    if (F > Fv) launch_rowgram<false>(s, X + Fv, (int)N, F - Fv, ld, shift ? shift + Fv : nullptr, K, acc, ws);
    return dm_launch_status("dm_pca_rowgram");
}

extern "C" int dm_pca_components(const float *X, int64_t N, int F, int64_t ld, const float *shift, const float *W, int k,
                                 double *V, void *stream)
{
    if (check_wide_x("dm_pca_components", X, N, F, ld)) return -1;
    DM_REQUIRE(W && V, "dm_pca_components: W / V is NULL");
    DM_REQUIRE(k >= 1 && k <= DM_PCA_MAX_COMPONENTS, "dm_pca_components: k = %d components, supported 1 .. %d", k,
               DM_PCA_MAX_COMPONENTS);
    hipStream_t s = (hipStream_t)stream;
    const bool v4 = vec4_ok(X, ld);
    if (k <= 16) launch_components<16>(v4, s, X, (int)N, F, ld, shift, W, k, V);
    else if (k <= 32) launch_components<32>(v4, s, X, (int)N, F, ld, shift, W, k, V);
    else launch_components<64>(v4, s, X, (int)N, F, ld, shift, W, k, V);
    return dm_launch_status("dm_pca_components");
}

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
