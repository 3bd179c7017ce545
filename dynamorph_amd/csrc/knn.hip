// knn.hip -- the exact k-nearest-neighbour graph of the latents (the n_neighbors graph umap.UMAP takes as precomputed_knn;
// run_dim_reduction.py:143-207 fit_umap builds it inside umap-learn on the CPU).
//
// X (M x F fp32, row-major, leading dimension ldx) is the point set, Q (R x F) the queries -- foreign rows, or rows
// r0 .. r0 + R - 1 of X itself (the pair (i, i) is then excluded by index).  One call handles one panel of R queries:
//   norms     |x - s|^2 of every row in float64 (the squares of fp32 numbers are exact there), and their maximum.
//   gram      g = |q - s|^2 + |x - s|^2 - 2 (q - s).(x - s): 128 x 128 tiles on v_mfma_f32_32x32x2_f32, fp32 within a slab of
//             GT_SLAB features, slabs added in float64 registers, the result rounded to the fp32 panel (R x M).  A FILTER.
//   select    per panel row: the K = k + slack smallest by radix select on the value's bits (ties: the lowest columns), and
//             the smallest value left out.
//   refine    per row: the candidates' distances in the exact form -- differences and squares in fp32, four squares added in
//             fp32, those sums in float64 in a fixed order, one wave per pair, the root rounded to fp32 once -- sorted by
//             (distance, column); the first k are written.  The row is CERTIFIED when the k-th distance squared, times
//             1 + 2^-20, lies below (smallest rejected - A)(1 - rho), A the proven error bound of the filter (DESIGN.md
//             section 3.5b): then every row left out has a strictly larger fp32 distance.  The other rows go onto a list.
//   fallback  the listed rows, KN_FB_ROWS at a time: exact-form distances to all M columns, the same select (K = k: ties by
//             the lowest column, the order of the result) and the same refine without a certificate.  The host does not
//             know how many rows are listed: the launches are always made and leave at once when the list is shorter (no
//             read-back, capture-free).
// Latents of more than DM_KNN_MAX_FEATURES features: dm_knn_wide is the foreign form with the wide
// feature cap; dm_knn_wide_self computes the whole graph of at most DM_PCA_WIDE_MAX_SAMPLES rows from their row Gram matrix
// (dm_pca_rowgram) -- a streaming panel kernel instead of the Gram product, and a refine that evaluates a pair once.
// No atomics on floating-point data and no dependence on the launch shape in any value: results are a function of the inputs.
#include "dm_common.h"
#include "exact_form.h"
#include <math.h>

namespace {

constexpr int KN_CAND = DM_KNN_MAX_K + DM_KNN_MAX_SLACK;        // 512 candidates at most: the sort's LDS
constexpr int KN_FB_ROWS = 256;         // rows of the fallback panel

// The norms and their maximum: row_norms_kernel and norms_max_kernel of gram_tile.h.

// ---------------------------------------------------------------------------------------------------- Gram panel
// Workgroup id = column tile * row_tiles + row tile: the workgroups resident together share a few column tiles of X, which
// crosses HBM once per panel, and the panel's queries stay in the caches.  4 waves, wave w owns the 64 x 64 quarter
// (w >> 1, w & 1) as 2 x 2 accumulators of the 32x32x2 instruction.  A thread stages features 4 (tid >> 6) .. + 3 of rows
// (tid & 63) and (tid & 63) + 64 of both operands and stores them transposed ([feature][row]: a wave's 64 rows are 64
// consecutive words of one LDS row).  `shift` is never NULL here (the host passes zeros).  Two stages of loads are in flight during a stage's products: a fetch only loads -- the
// shift is subtracted when the registers go to LDS, so nothing waits for a load before the products are issued -- and it is
// unconditional (past the end it repeats the last stage), so the wait in front of the LDS stores counts one fetch as
// outstanding.  Rows past the matrices repeat the last row: their products are never stored.
template <bool V4>
__global__ __launch_bounds__(256) void knn_gram_kernel(const float *__restrict__ Q, int R, long long ldq,
                                                       const float *__restrict__ X, int M, long long ldx, int F,
                                                       const float *__restrict__ shift, const double *__restrict__ nq,
                                                       const double *__restrict__ nx, int self_r0,
                                                       float *__restrict__ panel, long long ldp, int row_tiles)
{
    __shared__ __attribute__((aligned(16))) float lds[2][2][GT_CH * GT_LW];
    const int I = (int)(blockIdx.x % row_tiles) * GT, J = (int)(blockIdx.x / row_tiles) * GT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int sr = tid & 63, sf = 4 * (tid >> 6);

    const float *qrow[2], *xrow[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int rq = I + sr + 64 * q, rx = J + sr + 64 * q;
        qrow[q] = Q + (long long)(rq < R ? rq : R - 1) * ldq;
        xrow[q] = X + (long long)(rx < M ? rx : M - 1) * ldx;
    }
    const int nstages = (F + GT_CH - 1) / GT_CH;

    f32x4 ra[2][2], rb[2][2], rs[2];
    auto fetch = [&](int stage, int slot) {
        const int f = (stage < nstages ? stage : nstages - 1) * GT_CH + sf;
        rs[slot] = row_load4_clamped<V4>(shift, f, F);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            ra[slot][q] = row_load4_clamped<V4>(qrow[q], f, F);
            rb[slot][q] = row_load4_clamped<V4>(xrow[q], f, F);
        }
    };
    auto stash = [&](int stage, int slot, int buf) {
        const int f = stage * GT_CH + sf;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const f32x4 va = ra[slot][q] - rs[slot], vb = rb[slot][q] - rs[slot];
#pragma unroll
            for (int e = 0; e < 4; ++e) {       // features past F: zeros
                lds[buf][0][(sf + e) * GT_LW + sr + 64 * q] = f + e < F ? va[e] : 0.f;
                lds[buf][1][(sf + e) * GT_LW + sr + 64 * q] = f + e < F ? vb[e] : 0.f;
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
            stash(st + 1, u ^ 1, u ^ 1);        // (unconditional like the fetch: past the end nobody reads it)
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
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = gt_col(J + wn * 64 + j * 32, lane);
        if (col >= M) continue;
        const double ncol = nx[col];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = gt_row(I + wm * 64 + i * 32, e, lane);
                if (row >= R) continue;
                float g = (float)(nq[row] + ncol - 2.0 * dacc[i][j][e]);
                if (self_r0 >= 0 && self_r0 + row == col) g = INFINITY;      // the pair (i, i): excluded by index
                panel[(long long)row * ldp + col] = g;
            }
    }
}

// The exact form of a pair (knn_exact_d2, knn_dist_of): exact_form.h, shared with kmeans.hip.

// The rows a workgroup serves: slot s is row s of the panel, or (fallback) entry base + s of the list of uncertified rows.
struct RowList { const int *rows; const int *count; int base; };

__device__ __forceinline__ int row_of_slot(const RowList &rl, int slot)
{
    if (!rl.rows) return slot;
    return rl.base + slot < *rl.count ? rl.rows[rl.base + slot] : -1;
}

// Fallback panel: D[slot][j] = exact-form distance of the slot's row to every column j, one wave per pair.
template <bool V4>
__global__ __launch_bounds__(256) void knn_exact_panel_kernel(const float *__restrict__ Q, long long ldq,
                                                              const float *__restrict__ X, int M, long long ldx, int F,
                                                              int self_r0, float *__restrict__ D, long long ldd, RowList rl)
{
    const int slot = blockIdx.y;
    const int row = row_of_slot(rl, slot);
    if (row < 0) return;
    const int lane = threadIdx.x & 63;
    const float *__restrict__ q = Q + (long long)row * ldq;
    for (long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); j < M; j += (long long)gridDim.x * 4) {
        float d = knn_dist_of(knn_exact_d2<V4>(q, X + j * ldx, F, lane));
        if (self_r0 >= 0 && self_r0 + row == j) d = INFINITY;
        if (lane == 0) D[(long long)slot * ldd + j] = d;
    }
}

// ----------------------------------------------------------------------------------------------------- selection
// Order-preserving unsigned key of an fp32 value (negative numbers below positive ones, +inf above every finite one).
typedef unsigned int KnnKey;
__device__ __forceinline__ KnnKey knn_key(float v)
{
    const KnnKey b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float knn_key_value(KnnKey k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// One workgroup per panel row: the K smallest of its M values by (value, column), K <= M.  Radix select, most significant
// byte first: a pass counts the byte among the values that share the prefix found so far (integer LDS counters) and fixes
// the byte in which the K-th smallest lies.  Afterwards T is the K-th smallest key: every value below T is a candidate, and
// of those equal to T the `need` lowest columns.  cand[slot][0 .. K) (unordered below T), rej[slot] = the smallest value
// not taken (+inf when none is left).
__global__ __launch_bounds__(256) void knn_select_kernel(const float *__restrict__ panel, long long ldp, int M, int K,
                                                         int *__restrict__ cand, int ldc, double *__restrict__ rej, RowList rl)
{
    typedef KnnKey U;
    constexpr int NB = (int)sizeof(U);
    __shared__ int hist[256];
    __shared__ int s_digit, s_need, s_ties, s_nlt, s_neq;
    __shared__ U s_rejmin;
    const int slot = blockIdx.x, tid = threadIdx.x;
    if (row_of_slot(rl, slot) < 0) return;
    const float *__restrict__ row = panel + (long long)slot * ldp;
    int *__restrict__ out = cand + (long long)slot * ldc;

    // the row in 16-byte steps (rows start on 128 bytes); fn(column, key) for every column below M
    auto scan = [&](auto fn) {
        for (int j = 4 * tid; j < M; j += 1024) {
            if (j + 3 < M) {
                const f32x4 v = *(const f32x4 *)(row + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) fn(j + e, knn_key(v[e]));
            } else {
                for (int e = 0; j + e < M; ++e) fn(j + e, knn_key(row[j + e]));
            }
        }
    };

    U prefix = 0;
    int need = K;                       // the need-th smallest among the values that share the prefix
    for (int p = NB - 1; p >= 0; --p) {
        hist[tid] = 0;
        __syncthreads();
        const int sh = 8 * p;
        // a thread adds a run of equal bytes at once: in the first pass nearly every value of a row has the same byte
        // (sign and exponent), and 256 threads adding ones to one LDS word would take turns
        int cur = -1, run = 0;
        scan([&](int, U u) {
            if (p != NB - 1 && (u >> (sh + 8)) != (prefix >> (sh + 8))) return;
            const int d = (int)((u >> sh) & 255);
            if (d == cur) { ++run; return; }
            if (run) atomicAdd(&hist[cur], run);
            cur = d;
            run = 1;
        });
        if (run) atomicAdd(&hist[cur], run);
        __syncthreads();
        if (tid == 0) {
            int c = 0, d = 0;
            for (; d < 255; ++d) {
                if (c + hist[d] >= need) break;
                c += hist[d];
            }
            s_digit = d;
            s_need = need - c;
            s_ties = hist[d];
        }
        __syncthreads();
        prefix |= (U)s_digit << sh;
        need = s_need;
    }
    const int ties = s_ties;            // values equal to T; `need` of them (>= 1) are taken
    const bool all_ties = ties == need;
    if (tid == 0) { s_nlt = 0; s_neq = 0; s_rejmin = ~(U)0; }
    __syncthreads();
    const int eq0 = K - need;           // the values below T fill cand[0 .. eq0)
    U mymin = ~(U)0;
    scan([&](int j, U u) {
        if (u < prefix) out[atomicAdd(&s_nlt, 1)] = j;
        else if (u > prefix) mymin = u < mymin ? u : mymin;
        else if (all_ties) out[eq0 + atomicAdd(&s_neq, 1)] = j;
    });
    if (mymin != ~(U)0) atomicMin(&s_rejmin, mymin);
    if (!all_ties && tid < 64) {        // more ties than places: one wave walks the row in column order
        int taken = 0;
        for (int j0 = 0; j0 < M && taken < need; j0 += 64) {
            const int j = j0 + tid;
            const bool is = j < M && knn_key(row[j]) == prefix;
            const unsigned long long b = __ballot(is);
            const int rank = taken + __popcll(b & ((1ull << tid) - 1ull));
            if (is && rank < need) out[eq0 + rank] = j;
            taken += __popcll(b);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const U r = all_ties ? s_rejmin : prefix;
        rej[slot] = r == ~(U)0 ? (double)INFINITY : (double)knn_key_value(r);
    }
}

// ------------------------------------------------------------------------------------------ refine and certificate
__device__ __forceinline__ bool pair_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

// The LDS sorts work on a power of two >= K entries (at least 2), padded with (+inf, INT_MAX).
__device__ __forceinline__ int knn_sort_size(int K)
{
    int P = 2;
    while (P < K) P <<= 1;
    return P;
}

// The tail of a refine, by the whole workgroup of 256 threads once s_d / s_i hold the row's P (distance, column) pairs and a
// barrier has passed: bitonic sort by (distance, column) in LDS, the first kk written behind the optional self column, and
// (certify) the row listed unless the certificate stated at knn_refine_kernel holds.  (distance, column) is a total order
// -- a row names no column twice -- so the result does not depend on the order the pairs arrived in.
__device__ __forceinline__ void knn_sort_write_certify(float *s_d, int *s_i, int P, int kk, int include_self, int self_r0, int row,
                                                       const double *__restrict__ rej_slot, const double *__restrict__ nq,
                                                       const double *__restrict__ nxmax, double cbound, int certify,
                                                       int *__restrict__ idx_out, float *__restrict__ dist_out,
                                                       int *__restrict__ fail_list, int *__restrict__ n_fail)
{
    const int tid = threadIdx.x;
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int pos = 2 * tid - (tid & (stride - 1));
            if (pos + stride < P) {
                const bool up = (pos & size) == 0;
                const float da = s_d[pos], db = s_d[pos + stride];
                const int ia = s_i[pos], ib = s_i[pos + stride];
                if (pair_less(db, ib, da, ia) == up) {
                    s_d[pos] = db; s_i[pos] = ib;
                    s_d[pos + stride] = da; s_i[pos + stride] = ia;
                }
            }
            __syncthreads();
        }
    const int k = kk + include_self;
    int *__restrict__ io = idx_out + (long long)row * k;
    float *__restrict__ dn = dist_out + (long long)row * k;
    if (include_self && tid == 0) { io[0] = self_r0 + row; dn[0] = 0.f; }
    for (int c = tid; c < kk; c += 256) {
        io[include_self + c] = s_i[c];
        dn[include_self + c] = s_d[c];
    }
    if (certify && tid == 0) {
        const double a = cbound * (nq[row] + *nxmax) + 1e-30;
        const double dk = (double)s_d[kk - 1];
        const bool ok = dk * dk * (1.0 + 0x1p-20) < (*rej_slot - a) * (1.0 - 0x1p-21);
        if (!ok) fail_list[atomicAdd(n_fail, 1)] = row;
    }
}

// One workgroup per row: exact-form distances of its K candidates (a wave per pair), bitonic sort by (distance, column) in
// LDS, the first kk written behind the optional self column.  certify: the row goes onto the list unless
//     d[kk - 1]^2 (1 + 2^-20) < (rej - cbound (|q|^2 + max |x|^2) - tiny) (1 - 2^-21):
// the right side is a lower bound of the float64 sum of every row left out, and a sum above d^2 (1 + 2^-20) has a root above
// d (1 + 2^-22), more than one fp32 step past d: its rounded distance is strictly larger.
template <bool V4>
__global__ __launch_bounds__(256) void knn_refine_kernel(const float *__restrict__ Q, long long ldq, const float *__restrict__ X,
                                                         long long ldx, int F, const int *__restrict__ cand, int ldc, int K,
                                                         int kk, int include_self, int self_r0, const double *__restrict__ rej,
                                                         const double *__restrict__ nq, const double *__restrict__ nxmax,
                                                         double cbound, int certify, int *__restrict__ idx_out,
                                                         float *__restrict__ dist_out, int *__restrict__ fail_list,
                                                         int *__restrict__ n_fail, RowList rl)
{
    __shared__ float s_d[KN_CAND];
    __shared__ int s_i[KN_CAND];
    const int slot = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row = row_of_slot(rl, slot);
    if (row < 0) return;
    const int P = knn_sort_size(K);
    const float *__restrict__ q = Q + (long long)row * ldq;
    for (int c = w; c < P; c += 4) {
        float d = INFINITY;
        int j = 0x7fffffff;
        if (c < K) {
            j = cand[(long long)slot * ldc + c];
            d = knn_dist_of(knn_exact_d2<V4>(q, X + (long long)j * ldx, F, lane));
        }
        if (lane == 0) { s_d[c] = d; s_i[c] = j; }
    }
    __syncthreads();
    knn_sort_write_certify(s_d, s_i, P, kk, include_self, self_r0, row, rej + slot, nq, nxmax, cbound, certify, idx_out,
                           dist_out, fail_list, n_fail);
}

// include_self with k = 1: the graph is the self column alone.
__global__ __launch_bounds__(256) void knn_self_only_kernel(int R, int self_r0, int *__restrict__ idx_out,
                                                            float *__restrict__ dist_out, int *__restrict__ counter)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0) *counter = 0;
    if (r < R) { idx_out[r] = self_r0 + r; dist_out[r] = 0.f; }
}

// ---------------------------------------------------------------- the wide self form: panel from a row Gram matrix
// g[i][j] = fp32(n_i + n_j - 2 K[i][j]) for K = (X - s)(X - s)^T as dm_pca_rowgram wrote it (float64, N x N, full), the
// diagonal +inf.  A stream: a thread takes four consecutive columns of one row, 32 bytes of K in and 16 bytes of the panel
// out.  V2 (N even, K on 16 bytes): every row of K starts on 16 bytes and is read in 16-byte steps.
template <bool V2>
__global__ __launch_bounds__(256) void knn_wide_panel_kernel(const double *__restrict__ K, int N, const double *__restrict__ nx,
                                                             float *__restrict__ panel, long long ldp)
{
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    const int i = blockIdx.y;
    const int j = 4 * (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= N) return;
    const double *__restrict__ krow = K + (long long)i * N;
    float *__restrict__ prow = panel + (long long)i * ldp;
    const double ni = nx[i];
    if (V2 && j + 3 < N) {
        const f64x2 ka = *(const f64x2 *)(krow + j), kb = *(const f64x2 *)(krow + j + 2);
        const f64x2 na = *(const f64x2 *)(nx + j), nb = *(const f64x2 *)(nx + j + 2);
        f32x4 g;
        g.x = (float)(ni + na.x - 2.0 * ka.x);
        g.y = (float)(ni + na.y - 2.0 * ka.y);
        g.z = (float)(ni + nb.x - 2.0 * kb.x);
        g.w = (float)(ni + nb.y - 2.0 * kb.y);
        if (i == j) g.x = INFINITY;
        if (i == j + 1) g.y = INFINITY;
        if (i == j + 2) g.z = INFINITY;
        if (i == j + 3) g.w = INFINITY;
        *(f32x4 *)(prow + j) = g;
    } else {
        for (int e = 0; e < 4 && j + e < N; ++e)
            prow[j + e] = i == j + e ? INFINITY : (float)(ni + nx[j + e] - 2.0 * krow[j + e]);
    }
}

// ------------------------------------------------------------------------------- the wide self form: pair-once refine
// The exact-form distance is symmetric to the bit (fl(a - b) = -fl(b - a), equal squares, the same order of sums), so a
// pair that is on both rows' candidate lists is evaluated once.  Three launches replace knn_refine_kernel:
//   sort      every row's K candidates ascending by column (bitonic in LDS), so that a row can be searched;
//   evaluate  workgroup = row i, wave = candidate j: i is looked up in row j's list; a mutual pair belongs to the smaller row
//             and the other skips it; the owner's lane 0 writes the distance into row i's slot and, when mutual, into row j's
//             slot at the position found.  Every slot is written exactly once;
//   certify   knn_refine_kernel's tail on those distances.
// One workgroup per row; block 0 also clears the pair counter.
__global__ __launch_bounds__(256) void knn_cand_sort_kernel(int *__restrict__ cand, int K, int *__restrict__ n_pairs)
{
    __shared__ int s[KN_CAND];
    const int tid = threadIdx.x;
    const int P = knn_sort_size(K);
    int *__restrict__ row = cand + (long long)blockIdx.x * K;
    if (blockIdx.x == 0 && tid == 0 && n_pairs) *n_pairs = 0;
    for (int c = tid; c < P; c += 256) s[c] = c < K ? row[c] : 0x7fffffff;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int pos = 2 * tid - (tid & (stride - 1));
            if (pos + stride < P) {
                const bool up = (pos & size) == 0;
                const int a = s[pos], b = s[pos + stride];
                if ((b < a) == up) { s[pos] = b; s[pos + stride] = a; }
            }
            __syncthreads();
        }
    for (int c = tid; c < K; c += 256) row[c] = s[c];
}

template <bool V4>
__global__ __launch_bounds__(256) void knn_pair_eval_kernel(const float *__restrict__ X, long long ldx, int F,
                                                            const int *__restrict__ cand, int K, float *__restrict__ dsts,
                                                            int *__restrict__ n_pairs)
{
    const int i = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float *__restrict__ q = X + (long long)i * ldx;
    const int *__restrict__ mine = cand + (long long)i * K;
    int done = 0;
    for (int c = w; c < K; c += 4) {
        const int j = mine[c];
        const int *__restrict__ theirs = cand + (long long)j * K;
        int lo = 0, hi = K;                     // the first position of row j's list that holds i or more
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (theirs[mid] < i) lo = mid + 1;
            else hi = mid;
        }
        const bool mutual = lo < K && theirs[lo] == i;
        if (mutual && j < i) continue;          // row j owns the pair
        const float d = knn_dist_of(knn_exact_d2<V4>(q, X + (long long)j * ldx, F, lane));
        if (lane == 0) {
            dsts[(long long)i * K + c] = d;
            if (mutual) dsts[(long long)j * K + lo] = d;
        }
        ++done;
    }
    if (n_pairs && lane == 0 && done) atomicAdd(n_pairs, done);
}

__global__ __launch_bounds__(256) void knn_sort_certify_kernel(const int *__restrict__ cand, const float *__restrict__ dsts, int K,
                                                               int kk, int include_self, const double *__restrict__ rej,
                                                               const double *__restrict__ nx, const double *__restrict__ nxmax,
                                                               double cbound, int *__restrict__ idx_out,
                                                               float *__restrict__ dist_out, int *__restrict__ fail_list,
                                                               int *__restrict__ n_fail)
{
    __shared__ float s_d[KN_CAND];
    __shared__ int s_i[KN_CAND];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int P = knn_sort_size(K);
    for (int c = tid; c < P; c += 256) {
        s_d[c] = c < K ? dsts[(long long)row * K + c] : INFINITY;
        s_i[c] = c < K ? cand[(long long)row * K + c] : 0x7fffffff;
    }
    __syncthreads();
    knn_sort_write_certify(s_d, s_i, P, kk, include_self, 0, row, rej + row, nx, nxmax, cbound, 1, idx_out, dist_out, fail_list,
                           n_fail);
}

// ------------------------------------------------------------------------------------------------------- host
// The filter's error bound per unit of |q - s|^2 + |x - s|^2 (exact_form.h) for the loop's slabs.
double filter_bound() { return exact_form_filter_bound(GT_SLAB); }

struct KnnPlan {
    int kk, K, fb_rows, rounds;
    long long ldp, ldd;
    size_t o_panel, o_nx, o_nq, o_max, o_zero, o_cand, o_rej, o_list, o_fb, o_dst, total;
};

// 0, or the reason the shape is refused.  wide: the feature cap of the dm_knn_wide entries.
const char *knn_plan(long long R, long long M, int F, int k, int slack, int self_form, int include_self, bool wide, KnnPlan *p)
{
    if (R < 1 || M < 1) return "R and M must be >= 1";
    if (R > 0x7fffffffLL || M > 0x7fffffffLL) return "R and M must fit 31 bits";
    if (((R + GT - 1) / GT) * ((M + GT - 1) / GT) > 0x7fffffffLL) return "more than 2^31 tiles in one panel: split R";
    if (!wide && (F < 1 || F > DM_KNN_MAX_FEATURES)) return "F outside 1 .. DM_KNN_MAX_FEATURES";
    if (wide && (F < 1 || F > DM_KNN_WIDE_MAX_FEATURES)) return "F outside 1 .. DM_KNN_WIDE_MAX_FEATURES";
    if (wide && M > DM_PCA_WIDE_MAX_SAMPLES) return "more than DM_PCA_WIDE_MAX_SAMPLES rows of X";
    if (k < 1 || k > DM_KNN_MAX_K) return "k outside 1 .. DM_KNN_MAX_K";
    if (slack < 0 || slack > DM_KNN_MAX_SLACK) return "slack outside 0 .. DM_KNN_MAX_SLACK";
    if (include_self && !self_form) return "include_self needs the self form";
    const long long eligible = M - (self_form ? 1 : 0);
    p->kk = k - (include_self ? 1 : 0);
    if (p->kk > eligible) return "k exceeds the number of eligible rows";
    p->K = (int)(p->kk + slack < eligible ? p->kk + slack : eligible);
    p->fb_rows = (int)(R < KN_FB_ROWS ? R : KN_FB_ROWS);
    p->rounds = (int)((R + p->fb_rows - 1) / p->fb_rows);
    p->ldp = (M + 31) / 32 * 32;
    p->ldd = p->ldp;
    const int ldc = p->K > 0 ? p->K : 1;
    size_t o = 0;
    p->o_panel = o; o += align256((size_t)R * p->ldp * sizeof(float));
    p->o_nx = o;    o += align256((size_t)M * sizeof(double));
    p->o_nq = o;    o += align256((size_t)R * sizeof(double));
    p->o_max = o;   o += 256;
    p->o_zero = o;  o += align256((size_t)F * sizeof(float));
    p->o_cand = o;  o += align256((size_t)R * ldc * sizeof(int));
    p->o_rej = o;   o += align256((size_t)R * sizeof(double));
    p->o_list = o;  o += align256((size_t)R * sizeof(int));
    p->o_fb = o;    o += align256((size_t)p->fb_rows * p->ldd * sizeof(float));
    p->o_dst = o;   o += wide && self_form ? align256((size_t)R * ldc * sizeof(float)) : 0;     // (pair-once distances)
    p->total = o;
    return nullptr;
}

// The fallback rounds: the listed rows, fb_rows at a time, from exact-form distances to all M columns.
template <bool V4>
void knn_fallback_rounds(const KnnPlan &p, const float *X, int M, int F, long long ldx, const float *Q, long long ldq,
                         int self_r0, int include_self, int *idx, float *dist, int *n_fallback, char *ws, hipStream_t s)
{
    double *nmax = (double *)(ws + p.o_max), *rej = (double *)(ws + p.o_rej);
    const double *nq = self_r0 >= 0 ? (const double *)(ws + p.o_nx) + self_r0 : (const double *)(ws + p.o_nq);
    int *cand = (int *)(ws + p.o_cand), *list = (int *)(ws + p.o_list);
    float *fb = (float *)(ws + p.o_fb);
    const unsigned gx = (unsigned)(M / 4 + 1 < 64 ? M / 4 + 1 : 64);      // (a round without listed rows costs a launch, not a grid)
    for (int b = 0; b < p.rounds; ++b) {
        const RowList rl = {list, n_fallback, b * p.fb_rows};
        hipLaunchKernelGGL(knn_exact_panel_kernel<V4>, dim3(gx, p.fb_rows), dim3(256), 0, s, Q, ldq, X, M, ldx, F, self_r0, fb,
                           p.ldd, rl);
        hipLaunchKernelGGL(knn_select_kernel, dim3(p.fb_rows), dim3(256), 0, s, (const float *)fb, p.ldd, M, p.kk,
                           cand, p.K, rej, rl);
        hipLaunchKernelGGL(knn_refine_kernel<V4>, dim3(p.fb_rows), dim3(256), 0, s, Q, ldq, X, ldx, F, (const int *)cand, p.K,
                           p.kk, p.kk, include_self, self_r0, (const double *)rej, nq, (const double *)nmax,
                           0.0, 0, idx, dist, list, n_fallback, rl);
    }
}

template <bool V4>
void knn_launch(const KnnPlan &p, const float *X, int M, int F, long long ldx, const float *Q, int R, long long ldq,
                int self_r0, int include_self, const float *shift, const float *gram_shift, int *idx, float *dist,
                int *n_fallback, char *ws, hipStream_t s)
{
    float *panel = (float *)(ws + p.o_panel);
    double *nx = (double *)(ws + p.o_nx), *nq = (double *)(ws + p.o_nq), *nmax = (double *)(ws + p.o_max);
    int *cand = (int *)(ws + p.o_cand), *list = (int *)(ws + p.o_list);
    double *rej = (double *)(ws + p.o_rej);
    const RowList all = {nullptr, nullptr, 0};

    hipLaunchKernelGGL(row_norms_kernel<V4>, dim3((M + 3) / 4), dim3(256), 0, s, X, (long long)M, F, ldx, shift, nx);
    if (self_r0 >= 0) nq = nx + self_r0;
    else hipLaunchKernelGGL(row_norms_kernel<V4>, dim3((R + 3) / 4), dim3(256), 0, s, Q, (long long)R, F, ldq, shift, nq);
    hipLaunchKernelGGL(norms_max_kernel<256>, dim3(1), dim3(256), 0, s, (const double *)nx, (long long)M, nmax, n_fallback);
    const int row_tiles = (R + GT - 1) / GT;
    hipLaunchKernelGGL(knn_gram_kernel<V4>, dim3((unsigned)((long long)row_tiles * ((M + GT - 1) / GT))), dim3(256), 0, s,
                       Q, R, ldq, X, M, ldx, F, gram_shift, (const double *)nq, (const double *)nx, self_r0, panel, p.ldp, row_tiles);
    hipLaunchKernelGGL(knn_select_kernel, dim3(R), dim3(256), 0, s, (const float *)panel, p.ldp, M, p.K, cand, p.K, rej,
                       all);
    hipLaunchKernelGGL(knn_refine_kernel<V4>, dim3(R), dim3(256), 0, s, Q, ldq, X, ldx, F, (const int *)cand, p.K, p.K, p.kk,
                       include_self, self_r0, (const double *)rej, (const double *)nq, (const double *)nmax, filter_bound(), 1,
                       idx, dist, list, n_fallback, all);
    knn_fallback_rounds<V4>(p, X, M, F, ldx, Q, ldq, self_r0, include_self, idx, dist, n_fallback, ws, s);
}

// The wide self form: the panel comes from the row Gram matrix, each candidate pair is evaluated
// once (pair_once) or by knn_refine_kernel on the same lists; the norms, the selection, the certificate and the fallback are
// dm_knn's.  The filter's operands are dm_pca_rowgram's: the same fl(x - s), the same loop (gram_tile.h).
template <bool V4>
void knn_wide_self_launch(const KnnPlan &p, const float *X, int N, int F, long long ldx, const float *shift, const double *K,
                          int include_self, int pair_once, int *idx, float *dist, int *n_fallback, int *n_pairs, char *ws,
                          hipStream_t s)
{
    float *panel = (float *)(ws + p.o_panel), *dsts = (float *)(ws + p.o_dst);
    double *nx = (double *)(ws + p.o_nx), *nmax = (double *)(ws + p.o_max), *rej = (double *)(ws + p.o_rej);
    int *cand = (int *)(ws + p.o_cand), *list = (int *)(ws + p.o_list);
    const RowList all = {nullptr, nullptr, 0};

    hipLaunchKernelGGL(row_norms_kernel<V4>, dim3((N + 3) / 4), dim3(256), 0, s, X, (long long)N, F, ldx, shift, nx);
    hipLaunchKernelGGL(norms_max_kernel<256>, dim3(1), dim3(256), 0, s, (const double *)nx, (long long)N, nmax, n_fallback);
    const dim3 pg((unsigned)((N + 1023) / 1024), (unsigned)N);
    if (N % 2 == 0 && ((uintptr_t)K & 15) == 0)
        hipLaunchKernelGGL(knn_wide_panel_kernel<true>, pg, dim3(256), 0, s, K, N, (const double *)nx, panel, p.ldp);
    else
        hipLaunchKernelGGL(knn_wide_panel_kernel<false>, pg, dim3(256), 0, s, K, N, (const double *)nx, panel, p.ldp);
    hipLaunchKernelGGL(knn_select_kernel, dim3(N), dim3(256), 0, s, (const float *)panel, p.ldp, N, p.K, cand, p.K, rej, all);
    if (pair_once) {
        hipLaunchKernelGGL(knn_cand_sort_kernel, dim3(N), dim3(256), 0, s, cand, p.K, n_pairs);
        hipLaunchKernelGGL(knn_pair_eval_kernel<V4>, dim3(N), dim3(256), 0, s, X, ldx, F, (const int *)cand, p.K, dsts, n_pairs);
        hipLaunchKernelGGL(knn_sort_certify_kernel, dim3(N), dim3(256), 0, s, (const int *)cand, (const float *)dsts, p.K, p.kk,
                           include_self, (const double *)rej, (const double *)nx, (const double *)nmax, filter_bound(), idx,
                           dist, list, n_fallback);
    } else {
        hipLaunchKernelGGL(knn_refine_kernel<V4>, dim3(N), dim3(256), 0, s, X, ldx, X, ldx, F, (const int *)cand, p.K, p.K, p.kk,
                           include_self, 0, (const double *)rej, (const double *)nx, (const double *)nmax, filter_bound(), 1,
                           idx, dist, list, n_fallback, all);
    }
    knn_fallback_rounds<V4>(p, X, N, F, ldx, X, ldx, 0, include_self, idx, dist, n_fallback, ws, s);
}

// dm_knn and dm_knn_wide (foreign form): one body, the feature cap and the name in the error texts differ.
int knn_call(const char *who, bool wide, const float *X, int64_t M, int F, int64_t ldx, const float *Q, int64_t R, int64_t ldq,
             int64_t self_r0, int k, int slack, int include_self, const float *shift, int32_t *indices, float *distances,
             int32_t *n_fallback, void *workspace, int64_t workspace_bytes, void *stream)
{
    DM_REQUIRE(X, "%s: X is NULL", who);
    DM_REQUIRE(indices && distances && n_fallback, "%s: indices / distances / n_fallback is NULL", who);
    DM_REQUIRE(workspace, "%s: workspace is NULL", who);
    const int self_form = Q == nullptr;
    KnnPlan p;
    const char *why = knn_plan(R, M, F, k, slack, self_form, include_self, wide, &p);
    DM_REQUIRE(!why, "%s: R = %lld, M = %lld, F = %d, k = %d, slack = %d, %s form: %s", who, (long long)R, (long long)M, F, k,
               slack, self_form ? "self" : "foreign", why ? why : "");
    DM_REQUIRE(ldx >= F, "%s: leading dimension of X %lld < F = %d", who, (long long)ldx, F);
    if (self_form) {
        DM_REQUIRE(self_r0 >= 0 && self_r0 + R <= M, "%s: rows %lld .. %lld of the self form lie outside X (M = %lld)", who,
                   (long long)self_r0, (long long)(self_r0 + R - 1), (long long)M);
        Q = X + self_r0 * ldx;
        ldq = ldx;
    } else {
        DM_REQUIRE(ldq >= F, "%s: leading dimension of Q %lld < F = %d", who, (long long)ldq, F);
        self_r0 = -1;
    }
    DM_REQUIRE(workspace_bytes >= (int64_t)p.total, "%s: workspace of %lld bytes, need %lld", who, (long long)workspace_bytes,
               (long long)p.total);
    DM_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace is not 256-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    if (p.kk == 0) {
        hipLaunchKernelGGL(knn_self_only_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, s, (int)R, (int)self_r0,
                           indices, distances, n_fallback);
        return dm_launch_status(who);
    }
    const float *gram_shift;
    if (const int e = shift_or_zeros(who, shift, (char *)workspace + p.o_zero, F, s, &gram_shift)) return e;
    if (vec4_ok(X, ldx, F) && vec4_ok(Q, ldq, F) && ((uintptr_t)shift & 15) == 0)
        knn_launch<true>(p, X, (int)M, F, ldx, Q, (int)R, ldq, (int)self_r0, include_self ? 1 : 0, shift, gram_shift, indices,
                         distances, n_fallback, (char *)workspace, s);
    else
        knn_launch<false>(p, X, (int)M, F, ldx, Q, (int)R, ldq, (int)self_r0, include_self ? 1 : 0, shift, gram_shift, indices,
                          distances, n_fallback, (char *)workspace, s);
    return dm_launch_status(who);
}

}  // namespace

extern "C" int64_t dm_knn_workspace_bytes(int64_t R, int64_t M, int F, int k, int slack)
{
    KnnPlan p;
    // the larger of the two forms: the foreign form keeps K = k + slack up to M
    if (knn_plan(R, M, F, k, slack, 0, 0, false, &p)) return -1;
    return (int64_t)p.total;
}

extern "C" int dm_knn(const float *X, int64_t M, int F, int64_t ldx, const float *Q, int64_t R, int64_t ldq, int64_t self_r0,
                      int k, int slack, int include_self, const float *shift, int32_t *indices, float *distances,
                      int32_t *n_fallback, void *workspace, int64_t workspace_bytes, void *stream)
{
    return knn_call("dm_knn", false, X, M, F, ldx, Q, R, ldq, self_r0, k, slack, include_self, shift, indices, distances,
                    n_fallback, workspace, workspace_bytes, stream);
}

extern "C" int64_t dm_knn_wide_workspace_bytes(int64_t R, int64_t M, int F, int k, int slack)
{
    KnnPlan p;
    if (knn_plan(R, M, F, k, slack, 0, 0, true, &p)) return -1;
    return (int64_t)p.total;
}

extern "C" int dm_knn_wide(const float *X, int64_t M, int F, int64_t ldx, const float *Q, int64_t R, int64_t ldq, int k,
                           int slack, const float *shift, int32_t *indices, float *distances, int32_t *n_fallback,
                           void *workspace, int64_t workspace_bytes, void *stream)
{
    DM_REQUIRE(Q, "dm_knn_wide: Q is NULL (the self form is dm_knn_wide_self)");
    return knn_call("dm_knn_wide", true, X, M, F, ldx, Q, R, ldq, -1, k, slack, 0, shift, indices, distances, n_fallback,
                    workspace, workspace_bytes, stream);
}

extern "C" int64_t dm_knn_wide_self_workspace_bytes(int64_t N, int F, int k, int slack)
{
    KnnPlan p;
    // the larger of include_self or not: k others, K = k + slack up to N, and the pair-once distances beside the candidates
    if (knn_plan(N, N, F, k, slack, 0, 0, true, &p)) return -1;
    return (int64_t)(p.total + align256((size_t)N * (p.K > 0 ? p.K : 1) * sizeof(float)));
}

extern "C" int dm_knn_wide_self(const float *X, int64_t N, int F, int64_t ldx, const float *shift, const double *K, int k,
                                int slack, int include_self, int pair_once, int32_t *indices, float *distances,
                                int32_t *n_fallback, int32_t *n_pairs, void *workspace, int64_t workspace_bytes, void *stream)
{
    DM_REQUIRE(X, "dm_knn_wide_self: X is NULL");
    DM_REQUIRE(K, "dm_knn_wide_self: K is NULL");
    DM_REQUIRE(indices && distances && n_fallback, "dm_knn_wide_self: indices / distances / n_fallback is NULL");
    DM_REQUIRE(workspace, "dm_knn_wide_self: workspace is NULL");
    KnnPlan p;
    const char *why = knn_plan(N, N, F, k, slack, 1, include_self, true, &p);
    DM_REQUIRE(!why, "dm_knn_wide_self: N = %lld, F = %d, k = %d, slack = %d: %s", (long long)N, F, k, slack, why ? why : "");
    DM_REQUIRE(ldx >= F, "dm_knn_wide_self: leading dimension of X %lld < F = %d", (long long)ldx, F);
    DM_REQUIRE(((uintptr_t)K & 7) == 0, "dm_knn_wide_self: K is not 8-byte aligned");
    DM_REQUIRE(workspace_bytes >= (int64_t)p.total, "dm_knn_wide_self: workspace of %lld bytes, need %lld",
               (long long)workspace_bytes, (long long)p.total);
    DM_REQUIRE(((uintptr_t)workspace & 255) == 0, "dm_knn_wide_self: workspace is not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (n_pairs) {                          // (the plain refine and the self-only graph evaluate no pair once)
        const hipError_t e = hipMemsetAsync(n_pairs, 0, sizeof(int32_t), s);
        if (e != hipSuccess) {
            dm_set_error("dm_knn_wide_self: hipMemsetAsync: %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    if (p.kk == 0) {
        hipLaunchKernelGGL(knn_self_only_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (int)N, 0, indices,
                           distances, n_fallback);
        return dm_launch_status("dm_knn_wide_self");
    }
    if (vec4_ok(X, ldx, F) && ((uintptr_t)shift & 15) == 0)
        knn_wide_self_launch<true>(p, X, (int)N, F, ldx, shift, K, include_self ? 1 : 0, pair_once, indices, distances,
                                   n_fallback, n_pairs, (char *)workspace, s);
    else
        knn_wide_self_launch<false>(p, X, (int)N, F, ldx, shift, K, include_self ? 1 : 0, pair_once, indices, distances,
                                    n_fallback, n_pairs, (char *)workspace, s);
    return dm_launch_status("dm_knn_wide_self");
}

// ============================================================================== ranks of given targets
// The rank of target j for row i of X: 1 + #{ l != i : (d(i, l), l) < (d(i, j), j) }, d the exact-form fp32 distance above
// (0 for j == i).  Per panel of R rows: the norms, the Gram panel and the fallback panel are the graph's kernels; here
//   thresholds  the exact-form sums D of the row's c targets (a wave per pair), sorted by (D, index) with the permutation;
//   count       one workgroup per panel row, the row read ONCE: a panel value g is placed among the sorted D by binary search
//               in LDS with the filter's bound A on BOTH sides.  Certain against every threshold: one of c + 1 integer LDS
//               bins.  Ambiguous against any: its column goes onto the row's list (cap entries); a list that overflows
//               sends the row onto the fallback list;
//   resolve     the listed columns' exact-form distances, each once, compared by (distance, index) with every threshold;
//               rank = 1 + prefix sum of the bins + those comparisons, written in the caller's target order;
//   fallback    listed rows, KN_FB_ROWS at a time: knn_exact_panel_kernel, then the same count by plain comparison.
// Integer atomics only (a sum of ones does not depend on the order); no value depends on the launch shape, cap or the path.
namespace {

constexpr int KR_MAX_C = DM_KNN_MAX_K;
constexpr double KR_RHO = 0x1p-21, KR_STEP = 0x1p-20;

template <bool V4>
__global__ __launch_bounds__(256) void rank_thresholds_kernel(const float *__restrict__ X, int M, long long ldx, int F, int self_r0,
                                                              const int *__restrict__ targets, int c, double *__restrict__ tD,
                                                              float *__restrict__ td, int *__restrict__ tj, int *__restrict__ tp)
{
    __shared__ double s_D[KR_MAX_C];
    __shared__ int s_j[KR_MAX_C], s_p[KR_MAX_C];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int me = self_r0 + row;
    const int P = knn_sort_size(c);
    const float *__restrict__ q = X + (long long)me * ldx;
    for (int t = w; t < P; t += 4) {
        double D = INFINITY;                    // padding, the row itself (rank 0) and a target outside X: above everything
        int j = 0x7fffffff;
        if (t < c) {
            j = targets[(long long)row * c + t];
            if (j >= 0 && j < M && j != me) D = knn_exact_d2<V4>(q, X + (long long)j * ldx, F, lane);
        }
        if (lane == 0) { s_D[t] = D; s_j[t] = j; s_p[t] = t; }
    }
    __syncthreads();
    // (D, index, position) is a total order: repeated targets stay apart, and the result does not depend on the sort's path
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const int pos = 2 * tid - (tid & (stride - 1));
            if (pos + stride < P) {
                const bool up = (pos & size) == 0;
                const double Da = s_D[pos], Db = s_D[pos + stride];
                const int ja = s_j[pos], jb = s_j[pos + stride], pa = s_p[pos], pb = s_p[pos + stride];
                const bool b_less = Db < Da || (Db == Da && (jb < ja || (jb == ja && pb < pa)));
                if (b_less == up) {
                    s_D[pos] = Db; s_j[pos] = jb; s_p[pos] = pb;
                    s_D[pos + stride] = Da; s_j[pos + stride] = ja; s_p[pos + stride] = pa;
                }
            }
            __syncthreads();
        }
    for (int t = tid; t < c; t += 256) {
        const long long o = (long long)row * c + t;
        tD[o] = s_D[t];
        td[o] = knn_dist_of(s_D[t]);
        tj[o] = s_j[t];
        tp[o] = s_p[t];
    }
}

// One workgroup per panel row.  lo = (g + A)(1 + rho)(1 + 2^-20) and hi = (g - A)(1 - rho): D_l lies in [hi, lo / (1 + 2^-20)]
// (DESIGN.md 3.5i), so l is certainly below threshold t when lo < D_t and certainly above it when hi > D_t (1 + 2^-20) = E_t.
// p = #{t : D_t <= lo}: l is certainly below the thresholds p .. c - 1, and certain against all of them when E_{p-1} < hi.
// Most of a row lies above every threshold: those are counted in a register and added once.  The next two 16-byte steps of
// the row are requested before the current two are searched.
__global__ __launch_bounds__(256) void rank_count_kernel(const float *__restrict__ panel, long long ldp, int M, int self_r0,
                                                         const double *__restrict__ tD, int c, const double *__restrict__ nq,
                                                         const double *__restrict__ nxmax, double cbound, int cap,
                                                         int *__restrict__ hist, int *__restrict__ namb, int *__restrict__ amb,
                                                         int *__restrict__ fail_list, int *__restrict__ n_fail)
{
    __shared__ double s_D[KR_MAX_C], s_E[KR_MAX_C];
    __shared__ int s_hist[KR_MAX_C + 1];
    __shared__ int s_namb;
    const int row = blockIdx.x, tid = threadIdx.x;
    const int me = self_r0 + row;
    for (int t = tid; t < c; t += 256) {
        const double D = tD[(long long)row * c + t];
        s_D[t] = D;
        s_E[t] = D * (1.0 + KR_STEP);
    }
    for (int t = tid; t <= c; t += 256) s_hist[t] = 0;
    if (tid == 0) s_namb = 0;
    __syncthreads();
    const double A = cbound * (nq[row] + *nxmax) + 1e-30;
    const double Emax = s_E[c - 1];
    const float *__restrict__ prow = panel + (long long)row * ldp;
    int *__restrict__ arow = amb + (long long)row * cap;
    int above = 0;

    auto place = [&](int col, float gv) {
        if (col >= M || col == me) return;
        const double g = (double)gv;
        const double hi = (g - A) * (1.0 - KR_RHO);
        if (hi > Emax) { ++above; return; }
        const double lo = (g + A) * ((1.0 + KR_RHO) * (1.0 + KR_STEP));
        int p = 0, n = c;
        while (n > 0) {
            const int h = n >> 1;
            if (s_D[p + h] <= lo) { p += h + 1; n -= h + 1; }
            else n = h;
        }
        if (p == 0 || s_E[p - 1] < hi) atomicAdd(&s_hist[p], 1);
        else {
            const int pos = atomicAdd(&s_namb, 1);
            if (pos < cap) arow[pos] = col;
        }
    };

    // rows of the panel start on 128 bytes and ldp is a multiple of 32: every 16-byte step below M lies inside the row
    const int nvec = (M + 3) >> 2;
    auto fetch = [&](int v) { return *(const f32x4 *)(prow + 4 * (v < nvec ? v : nvec - 1)); };     // (unconditional, clamped)
    f32x4 c0 = fetch(tid), c1 = fetch(tid + 256);
    for (int v = tid; v < nvec; v += 512) {
        const f32x4 n0 = fetch(v + 512), n1 = fetch(v + 768);
        __builtin_amdgcn_sched_barrier(0);      // the requests go out before the searches
#pragma unroll
        for (int e = 0; e < 4; ++e) place(4 * v + e, c0[e]);
        if (v + 256 < nvec) {
#pragma unroll
            for (int e = 0; e < 4; ++e) place(4 * (v + 256) + e, c1[e]);
        }
        c0 = n0;
        c1 = n1;
    }
    if (above) atomicAdd(&s_hist[c], above);
    __syncthreads();
    for (int t = tid; t <= c; t += 256) hist[(long long)row * (c + 1) + t] = s_hist[t];
    if (tid == 0) {
        namb[row] = s_namb;
        if (s_namb > cap) fail_list[atomicAdd(n_fail, 1)] = row;
    }
}

// The tail of resolve and of the fallback count, by the whole workgroup after a barrier: s_hist holds the row's c + 1 bins,
// s_cnt the comparisons decided one by one.  rank of the sorted threshold t = 1 + s_hist[0] + .. + s_hist[t] + s_cnt[t].
__device__ __forceinline__ void rank_write(int *s_hist, const int *s_cnt, const int *s_j, const int *__restrict__ tp, int c,
                                           int me, int *__restrict__ out)
{
    const int tid = threadIdx.x;
    if (tid == 0)
        for (int t = 1; t < c; ++t) s_hist[t] += s_hist[t - 1];
    __syncthreads();
    for (int t = tid; t < c; t += 256) out[tp[t]] = s_j[t] == me ? 0 : 1 + s_hist[t] + s_cnt[t];
}

template <bool V4>
__global__ __launch_bounds__(256) void rank_resolve_kernel(const float *__restrict__ X, long long ldx, int F, int self_r0, int c,
                                                           const float *__restrict__ td, const int *__restrict__ tj,
                                                           const int *__restrict__ tp, const int *__restrict__ hist,
                                                           const int *__restrict__ namb, const int *__restrict__ amb, int cap,
                                                           int *__restrict__ ranks, int *__restrict__ n_ambiguous)
{
    __shared__ float s_d[KR_MAX_C];
    __shared__ int s_j[KR_MAX_C], s_cnt[KR_MAX_C], s_hist[KR_MAX_C + 1];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = namb[row];
    if (n > cap) return;                        // the fallback's row
    const int me = self_r0 + row;
    const long long o = (long long)row * c;
    for (int t = tid; t < c; t += 256) {
        s_d[t] = td[o + t];
        s_j[t] = tj[o + t];
        s_cnt[t] = 0;
        s_hist[t] = hist[(long long)row * (c + 1) + t];
    }
    __syncthreads();
    const float *__restrict__ q = X + (long long)me * ldx;
    const int *__restrict__ arow = amb + (long long)row * cap;
    for (int a = w; a < n; a += 4) {
        const int l = arow[a];
        const float d = knn_dist_of(knn_exact_d2<V4>(q, X + (long long)l * ldx, F, lane));
        for (int t = lane; t < c; t += 64)
            if (pair_less(d, l, s_d[t], s_j[t])) atomicAdd(&s_cnt[t], 1);
    }
    if (tid == 0 && n) atomicAdd(n_ambiguous, n);
    __syncthreads();
    rank_write(s_hist, s_cnt, s_j, tp + o, c, me, ranks + o);
}

// Fallback: the slot's row of exact-form distances (knn_exact_panel_kernel) against the thresholds' fp32 distances, which
// are non-decreasing in the sorted order.  p = #{t : d_t <= v}: l is below the thresholds p .. c - 1; those equal to v are
// decided by the index.
__global__ __launch_bounds__(256) void rank_exact_count_kernel(const float *__restrict__ D, long long ldd, int M, int self_r0,
                                                               int c, const float *__restrict__ td, const int *__restrict__ tj,
                                                               const int *__restrict__ tp, int *__restrict__ ranks, RowList rl)
{
    __shared__ float s_d[KR_MAX_C];
    __shared__ int s_j[KR_MAX_C], s_cnt[KR_MAX_C], s_hist[KR_MAX_C + 1];
    const int slot = blockIdx.x, tid = threadIdx.x;
    const int row = row_of_slot(rl, slot);
    if (row < 0) return;
    const int me = self_r0 + row;
    const long long o = (long long)row * c;
    for (int t = tid; t < c; t += 256) {
        s_d[t] = td[o + t];
        s_j[t] = tj[o + t];
        s_cnt[t] = 0;
    }
    for (int t = tid; t <= c; t += 256) s_hist[t] = 0;
    __syncthreads();
    const float dmax = s_d[c - 1];
    const float *__restrict__ drow = D + (long long)slot * ldd;
    int above = 0;
    auto place = [&](int col, float v) {
        if (col >= M || col == me) return;
        if (v > dmax) { ++above; return; }
        int p = 0, n = c;
        while (n > 0) {
            const int h = n >> 1;
            if (s_d[p + h] <= v) { p += h + 1; n -= h + 1; }
            else n = h;
        }
        atomicAdd(&s_hist[p], 1);
        for (int t = p - 1; t >= 0 && s_d[t] == v; --t)
            if (col < s_j[t]) atomicAdd(&s_cnt[t], 1);
    };
    const int nvec = (M + 3) >> 2;
    for (int v = tid; v < nvec; v += 256) {
        const f32x4 x = *(const f32x4 *)(drow + 4 * v);
#pragma unroll
        for (int e = 0; e < 4; ++e) place(4 * v + e, x[e]);
    }
    if (above) atomicAdd(&s_hist[c], above);
    __syncthreads();
    rank_write(s_hist, s_cnt, s_j, tp + o, c, me, ranks + o);
}

struct RankPlan {
    int fb_rows, rounds, cap;
    long long ldp;
    size_t o_panel, o_nx, o_max, o_zero, o_tD, o_td, o_tj, o_tp, o_hist, o_namb, o_amb, o_list, o_fb, total;
};

// 0, or the reason the shape is refused.
const char *rank_plan(long long R, long long M, int F, int c, long long cap, RankPlan *p)
{
    if (R < 1 || M < 2) return "R must be >= 1 and M >= 2";
    if (R > 0x7fffffffLL || M > 0x7fffffffLL) return "R and M must fit 31 bits";
    if (((R + GT - 1) / GT) * ((M + GT - 1) / GT) > 0x7fffffffLL) return "more than 2^31 tiles in one panel: split R";
    if (F < 1 || F > DM_KNN_MAX_FEATURES) return "F outside 1 .. DM_KNN_MAX_FEATURES";
    if (c < 1 || c > KR_MAX_C) return "c outside 1 .. DM_KNN_MAX_K";
    if (cap < 1) return "cap must be >= 1";
    p->cap = (int)(cap < M ? cap : M);
    p->fb_rows = (int)(R < KN_FB_ROWS ? R : KN_FB_ROWS);
    p->rounds = (int)((R + p->fb_rows - 1) / p->fb_rows);
    p->ldp = (M + 31) / 32 * 32;
    size_t o = 0;
    p->o_panel = o; o += align256((size_t)R * p->ldp * sizeof(float));
    p->o_nx = o;    o += align256((size_t)M * sizeof(double));
    p->o_max = o;   o += 256;
    p->o_zero = o;  o += align256((size_t)F * sizeof(float));
    p->o_tD = o;    o += align256((size_t)R * c * sizeof(double));
    p->o_td = o;    o += align256((size_t)R * c * sizeof(float));
    p->o_tj = o;    o += align256((size_t)R * c * sizeof(int));
    p->o_tp = o;    o += align256((size_t)R * c * sizeof(int));
    p->o_hist = o;  o += align256((size_t)R * (c + 1) * sizeof(int));
    p->o_namb = o;  o += align256((size_t)R * sizeof(int));
    p->o_amb = o;   o += align256((size_t)R * p->cap * sizeof(int));
    p->o_list = o;  o += align256((size_t)R * sizeof(int));
    p->o_fb = o;    o += align256((size_t)p->fb_rows * p->ldp * sizeof(float));
    p->total = o;
    return nullptr;
}

template <bool V4>
void rank_launch(const RankPlan &p, const float *X, int M, int F, long long ldx, int r0, int R, const int *targets, int c,
                 const float *shift, const float *gram_shift, int *ranks, int *n_ambiguous, int *n_redone, char *ws, hipStream_t s)
{
    float *panel = (float *)(ws + p.o_panel), *td = (float *)(ws + p.o_td), *fb = (float *)(ws + p.o_fb);
    double *nx = (double *)(ws + p.o_nx), *nmax = (double *)(ws + p.o_max), *tD = (double *)(ws + p.o_tD);
    int *tj = (int *)(ws + p.o_tj), *tp = (int *)(ws + p.o_tp), *hist = (int *)(ws + p.o_hist), *namb = (int *)(ws + p.o_namb);
    int *amb = (int *)(ws + p.o_amb), *list = (int *)(ws + p.o_list);
    const float *Q = X + (long long)r0 * ldx;
    const double *nq = nx + r0;

    hipLaunchKernelGGL(row_norms_kernel<V4>, dim3((M + 3) / 4), dim3(256), 0, s, X, (long long)M, F, ldx, shift, nx);
    hipLaunchKernelGGL(norms_max_kernel<256>, dim3(1), dim3(256), 0, s, (const double *)nx, (long long)M, nmax, n_redone);
    const int row_tiles = (R + GT - 1) / GT;
    hipLaunchKernelGGL(knn_gram_kernel<V4>, dim3((unsigned)((long long)row_tiles * ((M + GT - 1) / GT))), dim3(256), 0, s,
                       Q, R, ldx, X, M, ldx, F, gram_shift, nq, (const double *)nx, r0, panel, p.ldp, row_tiles);
    hipLaunchKernelGGL(rank_thresholds_kernel<V4>, dim3(R), dim3(256), 0, s, X, M, ldx, F, r0, targets, c, tD, td, tj, tp);
    hipLaunchKernelGGL(rank_count_kernel, dim3(R), dim3(256), 0, s, (const float *)panel, p.ldp, M, r0, (const double *)tD, c,
                       nq, (const double *)nmax, filter_bound(), p.cap, hist, namb, amb, list, n_redone);
    hipLaunchKernelGGL(rank_resolve_kernel<V4>, dim3(R), dim3(256), 0, s, X, ldx, F, r0, c, (const float *)td, (const int *)tj,
                       (const int *)tp, (const int *)hist, (const int *)namb, (const int *)amb, p.cap, ranks, n_ambiguous);
    const unsigned gx = (unsigned)(M / 4 + 1 < 64 ? M / 4 + 1 : 64);
    for (int b = 0; b < p.rounds; ++b) {        // always launched: a round without listed rows leaves at once
        const RowList rl = {list, n_redone, b * p.fb_rows};
        hipLaunchKernelGGL(knn_exact_panel_kernel<V4>, dim3(gx, p.fb_rows), dim3(256), 0, s, Q, ldx, X, M, ldx, F, r0, fb, p.ldp,
                           rl);
        hipLaunchKernelGGL(rank_exact_count_kernel, dim3(p.fb_rows), dim3(256), 0, s, (const float *)fb, p.ldp, M, r0, c,
                           (const float *)td, (const int *)tj, (const int *)tp, ranks, rl);
    }
}

}  // namespace

extern "C" int64_t dm_knn_ranks_workspace_bytes(int64_t R, int64_t M, int F, int c, int64_t cap)
{
    RankPlan p;
    if (rank_plan(R, M, F, c, cap, &p)) return -1;
    return (int64_t)p.total;
}

extern "C" int dm_knn_ranks(const float *X, int64_t M, int F, int64_t ldx, int64_t r0, int64_t R, const int32_t *targets, int c,
                            const float *shift, int64_t cap, int32_t *ranks, int32_t *n_ambiguous, int32_t *n_redone,
                            void *workspace, int64_t workspace_bytes, void *stream)
{
    DM_REQUIRE(X, "dm_knn_ranks: X is NULL");
    DM_REQUIRE(targets && ranks, "dm_knn_ranks: targets / ranks is NULL");
    DM_REQUIRE(n_ambiguous && n_redone, "dm_knn_ranks: n_ambiguous / n_redone is NULL");
    DM_REQUIRE(workspace, "dm_knn_ranks: workspace is NULL");
    RankPlan p;
    const char *why = rank_plan(R, M, F, c, cap, &p);
    DM_REQUIRE(!why, "dm_knn_ranks: R = %lld, M = %lld, F = %d, c = %d, cap = %lld: %s", (long long)R, (long long)M, F, c,
               (long long)cap, why ? why : "");
    DM_REQUIRE(ldx >= F, "dm_knn_ranks: leading dimension of X %lld < F = %d", (long long)ldx, F);
    DM_REQUIRE(r0 >= 0 && r0 + R <= M, "dm_knn_ranks: rows %lld .. %lld lie outside X (M = %lld)", (long long)r0,
               (long long)(r0 + R - 1), (long long)M);
    DM_REQUIRE(workspace_bytes >= (int64_t)p.total, "dm_knn_ranks: workspace of %lld bytes, need %lld", (long long)workspace_bytes,
               (long long)p.total);
    DM_REQUIRE(((uintptr_t)workspace & 255) == 0, "dm_knn_ranks: workspace is not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(n_ambiguous, 0, sizeof(int32_t), s);
    if (e != hipSuccess) {
        dm_set_error("dm_knn_ranks: hipMemsetAsync: %s", hipGetErrorString(e));
        return (int)e;
    }
    const float *gram_shift;
    if (const int e2 = shift_or_zeros("dm_knn_ranks", shift, (char *)workspace + p.o_zero, F, s, &gram_shift)) return e2;
    if (vec4_ok(X, ldx, F) && ((uintptr_t)shift & 15) == 0)
        rank_launch<true>(p, X, (int)M, F, ldx, (int)r0, (int)R, targets, c, shift, gram_shift, ranks, n_ambiguous, n_redone,
                          (char *)workspace, s);
    else
        rank_launch<false>(p, X, (int)M, F, ldx, (int)r0, (int)R, targets, c, shift, gram_shift, ranks, n_ambiguous, n_redone,
                           (char *)workspace, s);
    return dm_launch_status("dm_knn_ranks");
}
