// kmeans.hip -- exact Lloyd k-means of the latents (sklearn.cluster.KMeans in HiddenStateExtractor's morphology_clustering.py /
// movement_clustering.py): the labelling pass, the per-cluster sums and the per-row distance.
//
// X is N x F fp32 (row-major, leading dimension ldx), the centres C are K x F fp32 (contiguous).  The distance of a row and a
// centre is the exact form of the k-NN graph (exact_form.h: knn_exact_d2, knn_dist_of), the label the centre of smallest
// (fp32 distance, index) -- what dm_knn(C, X, k = 1) returns, to the bit.
//   assign   row_norms_kernel + norms_max_kernel (gram_tile.h): |c - s|^2 of every centre in float64, their maximum; clears the counter of rechecked rows.
//            km_filter_kernel: a workgroup takes 128 rows of X and walks all centres in column tiles of 32, 64 or 128:
//            g = |x - s|^2 + |c - s|^2 - 2 (x - s).(c - s) on v_mfma_f32_32x32x2_f32, fp32 within a slab of 256 features, slabs
//            added in float64 registers (the filter of knn_gram_kernel, the same error bound); the row norms are summed in
//            float64 from the staged operands of the first tile.  Per row the two smallest g over all K are kept in registers:
//            the candidate and the smallest value rejected.  A FILTER.
//            km_certify_kernel, one wave per row: the candidate's exact-form distance and the certificate of section 3.5b for
//            k = 1, M = K; a row that fails it is redone from exact-form distances to all K centres by the same wave, in the
//            same call, and counted.  Labels and distances are exact-form.
//   sums     labels -> a stable grouping of the rows by cluster (integer histograms per block of 256 rows, their scan, the rank
//            of a row among its block's rows of the same label), clusters cut into segments of 128 rows, float64 segment sums
//            (4 waves interleaved, added in a fixed order), segments added in order.  No floating-point atomics: the order of
//            every sum depends on (N, F, K) and the labels only.
//   row_d2   the exact-form d^2 (float64) of every row to its labelled centre, one wave per row.
#include "dm_common.h"
#include "exact_form.h"
#include <math.h>

namespace {

constexpr int KM_BLK = 256;             // rows per block of the grouping kernels
constexpr int KM_SEG = 128;             // rows per segment of a cluster's sum

// The centre norms and their maximum: row_norms_kernel and norms_max_kernel of gram_tile.h.

// ------------------------------------------------------------------------------------------------ labelling pass
// 4 waves; wave w owns rows 32 w .. 32 w + 31 of the workgroup's 128 and all TN = 32 NT centres of the current tile as NT
// accumulators of the 32x32x2 instruction (A = rows of X, B = centres: the result's column, a centre, is on the lane and its
// 16 rows are in the registers).  Staging, the two fetches in flight and the slab folding are knn_gram_kernel's: a thread
// stages features 4 (tid >> 6) .. + 3 of rows (tid & 63) and (tid & 63) + 64 of X, and its share of the centre tile, stored
// transposed ([feature][row]).  `shift` is never NULL here (the host passes zeros).  Rows past N repeat the last row and
// centres past K the last centre: nothing of theirs is kept.
template <bool V4, int NT>
__global__ __launch_bounds__(256, NT == 1 ? 2 : 1) void km_filter_kernel(const float *__restrict__ X, int N, long long ldx,
                                                        const float *__restrict__ C, int K, int F,
                                                        const float *__restrict__ shift, const double *__restrict__ nc,
                                                        double *__restrict__ nq, int *__restrict__ cand,
                                                        float *__restrict__ rej)
{
    constexpr int TN = 32 * NT;                 // centres per tile
    constexpr int CR = TN < 64 ? TN : 64;       // centre rows one staging step of the workgroup covers
    constexpr int CQ = NT == 4 ? 2 : 1;         // centre rows per thread
    constexpr int CLW = TN + 32;                // LDS row stride of the centre operand
    constexpr int BUF = GT_CH * GT_LW + GT_CH * CLW;
    __shared__ __attribute__((aligned(16))) float lds[2][BUF];
    __shared__ double s_part[4][GT];         // the row norms by feature quarter, then s_nq: their sum
    __shared__ double s_nq[GT];

    const int I = (int)blockIdx.x * GT;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int sr = tid & 63, sf = 4 * (tid >> 6);
    const int cr = tid % CR, csf = 4 * (tid / CR);
    const bool cact = csf < GT_CH;              // (32 centres: waves 0 and 1 stage them)

    const float *xrow[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int rx = I + sr + 64 * q;
        xrow[q] = X + (long long)(rx < N ? rx : N - 1) * ldx;
    }
    const int nstages = (F + GT_CH - 1) / GT_CH;
    constexpr int STAGES_PER_SLAB = GT_SLAB / GT_CH;

    float m1[16], m2[16];
    int i1[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) { m1[e] = INFINITY; m2[e] = INFINITY; i1[e] = 0x7fffffff; }

    const int ntiles = (K + TN - 1) / TN;
    for (int ct = 0; ct < ntiles; ++ct) {
        const int J = ct * TN;
        const float *crow[CQ];
#pragma unroll
        for (int q = 0; q < CQ; ++q) {
            const int rc = J + cr + 64 * q;
            crow[q] = C + (long long)(rc < K ? rc : K - 1) * F;
        }
        f32x4 ra[2][2], rb[2][CQ], rs[2], rcs[2];
        double nacc[2] = {0.0, 0.0};
        auto fetch = [&](int stage, int slot) {
            const int st = stage < nstages ? stage : nstages - 1;
            rs[slot] = row_load4_clamped<V4>(shift, st * GT_CH + sf, F);
#pragma unroll
            for (int q = 0; q < 2; ++q) ra[slot][q] = row_load4_clamped<V4>(xrow[q], st * GT_CH + sf, F);
            if (cact) {
                rcs[slot] = row_load4_clamped<V4>(shift, st * GT_CH + csf, F);
#pragma unroll
                for (int q = 0; q < CQ; ++q) rb[slot][q] = row_load4_clamped<V4>(crow[q], st * GT_CH + csf, F);
            }
        };
        auto stash = [&](int stage, int slot, int buf) {
            float *A = lds[buf], *B = lds[buf] + GT_CH * GT_LW;
            const int f = stage * GT_CH + sf;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const f32x4 va = ra[slot][q] - rs[slot];
#pragma unroll
                for (int e = 0; e < 4; ++e) {       // features past F: zeros
                    const float v = f + e < F ? va[e] : 0.f;
                    A[(sf + e) * GT_LW + sr + 64 * q] = v;
                    if (ct == 0) nacc[q] += (double)v * (double)v;
                }
            }
            if (cact) {
                const int fc = stage * GT_CH + csf;
#pragma unroll
                for (int q = 0; q < CQ; ++q) {
                    const f32x4 vb = rb[slot][q] - rcs[slot];
#pragma unroll
                    for (int e = 0; e < 4; ++e) B[(csf + e) * CLW + cr + 64 * q] = fc + e < F ? vb[e] : 0.f;
                }
            }
        };

        f32x16 acc[NT];
        double dacc[NT][16];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            acc[j] = (f32x16){};
#pragma unroll
            for (int e = 0; e < 16; ++e) dacc[j][e] = 0.0;
        }

        fetch(0, 0);
        fetch(1, 1);
        stash(0, 0, 0);
        __syncthreads();
        for (int st0 = 0; st0 < nstages; st0 += 2) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {           // stage st lives in register slot u and LDS buffer u
                const int st = st0 + u;
                if (st >= nstages) break;
                fetch(st + 2, u);                   // (slot u went to LDS one stage ago)
                __builtin_amdgcn_sched_barrier(0);  // the loads are issued here, not after the products
                const float *A = lds[u], *B = lds[u] + GT_CH * GT_LW;
                const int oa = (lane >> 5) * GT_LW + (lane & 31) + 32 * w;
                const int ob = (lane >> 5) * CLW + (lane & 31);
#pragma unroll
                for (int kk = 0; kk < GT_CH / 2; ++kk) {
                    const float a = A[2 * kk * GT_LW + oa];
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, B[2 * kk * CLW + ob + 32 * j], acc[j], 0, 0, 0);
                }
                stash(st + 1, u ^ 1, u ^ 1);        // (unconditional like the fetch: past the end it stores zeros nobody reads)
                __syncthreads();
                if ((st + 1) % STAGES_PER_SLAB == 0 || st + 1 == nstages) {     // slab done: fold it into fp64, feature order
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) dacc[j][e] += (double)acc[j][e];
                        acc[j] = (f32x16){};
                    }
                }
            }
        }
        if (ct == 0) {                              // the row norms: the four feature quarters in order
#pragma unroll
            for (int q = 0; q < 2; ++q) s_part[w][sr + 64 * q] = nacc[q];
            __syncthreads();
            if (tid < GT) {
                const double n2 = ((s_part[0][tid] + s_part[1][tid]) + s_part[2][tid]) + s_part[3][tid];
                s_nq[tid] = n2;
                if (I + tid < N) nq[I + tid] = n2;
            }
            __syncthreads();
        }
        // C/D map of the 32x32 instruction: column (centre) lane & 31, row (e & 3) + 8 (e >> 2) + 4 (lane >> 5).  A lane meets
        // its centres in ascending order, so a strict comparison keeps the lowest index of equal values.
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int col = J + 32 * j + (lane & 31);
            const bool valid = col < K;
            const double ncol = valid ? nc[col] : 0.0;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int rl = 32 * w + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
                const float g = valid ? (float)(s_nq[rl] + ncol - 2.0 * dacc[j][e]) : INFINITY;
                const bool lt = g < m1[e];
                m2[e] = lt ? m1[e] : fminf(m2[e], g);
                i1[e] = lt ? col : i1[e];
                m1[e] = lt ? g : m1[e];
            }
        }
    }

    // the 32 lanes of a half hold one row's centres: the smallest by (value, index) and the smallest of all the others
#pragma unroll
    for (int e = 0; e < 16; ++e) {
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const float om1 = __shfl_xor(m1[e], o, 64), om2 = __shfl_xor(m2[e], o, 64);
            const int oi1 = __shfl_xor(i1[e], o, 64);
            const bool other = om1 < m1[e] || (om1 == m1[e] && oi1 < i1[e]);
            m2[e] = fminf(other ? m1[e] : om1, fminf(m2[e], om2));
            m1[e] = other ? om1 : m1[e];
            i1[e] = other ? oi1 : i1[e];
        }
        if ((lane & 31) == 0) {
            const int row = I + 32 * w + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
            if (row < N) { cand[row] = i1[e]; rej[row] = m2[e]; }
        }
    }
}

// One wave per row: the candidate's exact-form distance d and the certificate (DESIGN.md section 3.5b with k = 1, M = K):
//     d^2 (1 + 2^-20) < (rej - cbound (|x - s|^2 + max |c - s|^2) - tiny) (1 - 2^-21)
// proves that every other centre's fp32 distance is strictly larger.  Otherwise: all K exact-form distances, the smallest
// by (distance, index), and the row is counted.  Every lane holds the same numbers (the butterfly of knn_exact_d2), so the
// branch is the wave's.
template <bool V4>
__global__ __launch_bounds__(256) void km_certify_kernel(const float *__restrict__ X, int N, long long ldx,
                                                         const float *__restrict__ C, int K, int F,
                                                         const double *__restrict__ nq, const int *__restrict__ cand,
                                                         const float *__restrict__ rej, const double *__restrict__ ncmax,
                                                         double cbound, int *__restrict__ labels, float *__restrict__ dist,
                                                         int *__restrict__ rechecked)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float *__restrict__ x = X + row * ldx;
    int c = cand[row];
    float d = knn_dist_of(knn_exact_d2<V4>(x, C + (long long)c * F, F, lane));
    const double a = cbound * (nq[row] + *ncmax) + 1e-30;
    const double dk = (double)d;
    const bool ok = dk * dk * (1.0 + 0x1p-20) < ((double)rej[row] - a) * (1.0 - 0x1p-21);
    if (!ok) {
        d = INFINITY;
        c = 0;
        for (int j = 0; j < K; ++j) {
            const float dj = knn_dist_of(knn_exact_d2<V4>(x, C + (long long)j * F, F, lane));
            if (dj < d) { d = dj; c = j; }
        }
        if (lane == 0) atomicAdd(rechecked, 1);
    }
    if (lane == 0) {
        labels[row] = c;
        if (dist) dist[row] = d;
    }
}

// ---------------------------------------------------------------------------------------------- per-cluster sums
// hist[b][k]: rows of block b (KM_BLK consecutive rows) with label k.  Integer LDS counters; a label outside 0 .. K - 1
// belongs to no cluster.
__global__ __launch_bounds__(KM_BLK) void km_hist_kernel(const int *__restrict__ labels, int N, int K, int *__restrict__ hist)
{
    __shared__ int s[DM_KMEANS_MAX_CLUSTERS];
    const int tid = threadIdx.x;
    for (int k = tid; k < K; k += KM_BLK) s[k] = 0;
    __syncthreads();
    const long long r = (long long)blockIdx.x * KM_BLK + tid;
    if (r < N) {
        const int l = labels[r];
        if (l >= 0 && l < K) atomicAdd(&s[l], 1);
    }
    __syncthreads();
    for (int k = tid; k < K; k += KM_BLK) hist[(long long)blockIdx.x * K + k] = s[k];
}

// One wave per cluster: base[b][k] = rows of label k in the blocks before b; counts[k] = all of them.
__global__ __launch_bounds__(64) void km_scan_kernel(const int *__restrict__ hist, int nb, int K, int *__restrict__ base,
                                                     long long *__restrict__ counts)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    int run = 0;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int b = b0 + lane;
        const int v = b < nb ? hist[(long long)b * K + k] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        if (b < nb) base[(long long)b * K + k] = run + inc - v;
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0) counts[k] = run;
}

// row_start[k]: where cluster k's rows begin in the grouped order; seg_start[k]: its first segment (KM_SEG rows each, the
// last one shorter); entry K of both: the totals.  One thread: K <= 1024.
__global__ void km_offsets_kernel(const long long *__restrict__ counts, int K, int *__restrict__ row_start,
                                  int *__restrict__ seg_start)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int r = 0, s = 0;
    for (int k = 0; k < K; ++k) {
        row_start[k] = r;
        seg_start[k] = s;
        const int c = (int)counts[k];
        r += c;
        s += (c + KM_SEG - 1) / KM_SEG;
    }
    row_start[K] = r;
    seg_start[K] = s;
}

// perm: the rows grouped by label, each group in ascending row order (a stable counting sort).
__global__ __launch_bounds__(KM_BLK) void km_perm_kernel(const int *__restrict__ labels, int N, int K,
                                                         const int *__restrict__ base, const int *__restrict__ row_start,
                                                         int *__restrict__ perm)
{
    __shared__ int s_lab[KM_BLK];
    const int tid = threadIdx.x;
    const long long r = (long long)blockIdx.x * KM_BLK + tid;
    int l = -1;
    if (r < N) {
        l = labels[r];
        if (l < 0 || l >= K) l = -1;
    }
    s_lab[tid] = l;
    __syncthreads();
    if (l < 0) return;
    int rank = 0;
    for (int j = 0; j < tid; ++j) rank += s_lab[j] == l;
    perm[row_start[l] + base[(long long)blockIdx.x * K + l] + rank] = (int)r;
}

// Workgroup = (segment, 256 features): wave w adds rows w, w + 4, ... of the segment in float64, lane l features 4 l .. + 3;
// the four waves' sums are added in order.  part[segment][feature], rows of FP doubles.
template <bool V4>
__global__ __launch_bounds__(256) void km_segsum_kernel(const float *__restrict__ X, long long ldx, int F, int FP, int K,
                                                        const int *__restrict__ perm, const int *__restrict__ row_start,
                                                        const int *__restrict__ seg_start, double *__restrict__ part)
{
    __shared__ double s[4][256];
    const int sg = blockIdx.x;
    if (sg >= seg_start[K]) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int lo = 0, hi = K;                         // the last cluster whose first segment is <= sg
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seg_start[mid] <= sg) lo = mid;
        else hi = mid;
    }
    const int k = lo;
    const int first = row_start[k] + (sg - seg_start[k]) * KM_SEG;
    const int last = first + KM_SEG < row_start[k + 1] ? first + KM_SEG : row_start[k + 1];
    const int f = blockIdx.y * 256 + 4 * lane;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (f < F) {
#pragma unroll 4
        for (int p = first + w; p < last; p += 4) {
            const f32x4 v = row_load4<V4>(X + (long long)perm[p] * ldx, f, F);
            a0 += (double)v.x; a1 += (double)v.y; a2 += (double)v.z; a3 += (double)v.w;
        }
    }
    s[w][4 * lane + 0] = a0; s[w][4 * lane + 1] = a1; s[w][4 * lane + 2] = a2; s[w][4 * lane + 3] = a3;
    __syncthreads();
    const int fo = blockIdx.y * 256 + tid;
    if (fo < FP) part[(long long)sg * FP + fo] = ((s[0][tid] + s[1][tid]) + s[2][tid]) + s[3][tid];
}

// Workgroup = (cluster, 256 features): the cluster's segment sums, wave w segments w, w + 4, ..., the waves in order.
__global__ __launch_bounds__(256) void km_final_kernel(const double *__restrict__ part, int F, int FP,
                                                       const int *__restrict__ seg_start, double *__restrict__ sums)
{
    __shared__ double s[4][64];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int f = blockIdx.y * 64 + lane;
    const int s0 = seg_start[k], s1 = seg_start[k + 1];
    double a = 0.0;
    if (f < F) {
#pragma unroll 8
        for (int sg = s0 + w; sg < s1; sg += 4) a += part[(long long)sg * FP + f];
    }
    s[w][lane] = a;
    __syncthreads();
    if (w == 0 && f < F) sums[(long long)k * F + f] = ((s[0][lane] + s[1][lane]) + s[2][lane]) + s[3][lane];
}

// ------------------------------------------------------------------------------------------------------- row d^2
template <bool V4>
__global__ __launch_bounds__(256) void km_row_d2_kernel(const float *__restrict__ X, int N, int F, long long ldx,
                                                        const float *__restrict__ C, int K, const int *__restrict__ labels,
                                                        double *__restrict__ d2)
{
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= N) return;
    const int l = labels ? labels[r] : 0;
    if (l < 0 || l >= K) {
        if (lane == 0) d2[r] = (double)INFINITY;
        return;
    }
    const double v = knn_exact_d2<V4>(X + r * ldx, C + (long long)l * F, F, lane);
    if (lane == 0) d2[r] = v;
}

// ------------------------------------------------------------------------------------------------------- host
struct KmPlan {
    int nb, nseg, FP;
    size_t o_nc, o_max, o_zero, o_nq, o_cand, o_rej;            // the labelling pass
    size_t o_hist, o_base, o_rows, o_segs, o_perm, o_part;      // the sums (the same bytes: the passes follow each other)
    size_t total;
};

// 0, or the reason the shape is refused.
const char *km_plan(long long N, int F, int K, KmPlan *p)
{
    if (N < 1 || N > 0x7fffffffLL - GT) return "N outside 1 .. 2^31 - 129";
    if (F < 1 || F > DM_KNN_MAX_FEATURES) return "F outside 1 .. DM_KNN_MAX_FEATURES (reduce wider latents with the PCA first)";
    if (K < 1 || K > DM_KMEANS_MAX_CLUSTERS) return "K outside 1 .. DM_KMEANS_MAX_CLUSTERS";
    p->nb = (int)((N + KM_BLK - 1) / KM_BLK);
    p->nseg = (int)(N / KM_SEG) + K;            // >= sum over clusters of ceil(count / KM_SEG)
    p->FP = (F + 3) / 4 * 4;
    size_t a = 0;
    p->o_nc = a;   a += align256((size_t)K * sizeof(double));
    p->o_max = a;  a += 256;
    p->o_zero = a; a += align256((size_t)F * sizeof(float));
    p->o_nq = a;   a += align256((size_t)N * sizeof(double));
    p->o_cand = a; a += align256((size_t)N * sizeof(int));
    p->o_rej = a;  a += align256((size_t)N * sizeof(float));
    size_t b = 0;
    p->o_hist = b; b += align256((size_t)p->nb * K * sizeof(int));
    p->o_base = b; b += align256((size_t)p->nb * K * sizeof(int));
    p->o_rows = b; b += align256((size_t)(K + 1) * sizeof(int));
    p->o_segs = b; b += align256((size_t)(K + 1) * sizeof(int));
    p->o_perm = b; b += align256((size_t)N * sizeof(int));
    p->o_part = b; b += align256((size_t)p->nseg * p->FP * sizeof(double));
    p->total = a > b ? a : b;
    return nullptr;
}

template <bool V4>
void km_assign_launch(const KmPlan &p, const float *X, int N, int F, long long ldx, const float *C, int K, const float *shift,
                      const float *gs, int *labels, float *dist, int *rechecked, char *ws, hipStream_t s)
{
    double *nc = (double *)(ws + p.o_nc), *ncmax = (double *)(ws + p.o_max);
    hipLaunchKernelGGL(row_norms_kernel<V4>, dim3((K + 3) / 4), dim3(256), 0, s, C, (long long)K, F, (long long)F, shift, nc);
    hipLaunchKernelGGL(norms_max_kernel<256>, dim3(1), dim3(256), 0, s, (const double *)nc, (long long)K, ncmax, rechecked);
    double *nq = (double *)(ws + p.o_nq);
    int *cand = (int *)(ws + p.o_cand);
    float *rej = (float *)(ws + p.o_rej);
    const dim3 grid((unsigned)((N + GT - 1) / GT));
    if (K <= 32)
        hipLaunchKernelGGL((km_filter_kernel<V4, 1>), grid, dim3(256), 0, s, X, N, ldx, C, K, F, gs, (const double *)nc, nq, cand, rej);
    else if (K <= 64)
        hipLaunchKernelGGL((km_filter_kernel<V4, 2>), grid, dim3(256), 0, s, X, N, ldx, C, K, F, gs, (const double *)nc, nq, cand, rej);
    else
        hipLaunchKernelGGL((km_filter_kernel<V4, 4>), grid, dim3(256), 0, s, X, N, ldx, C, K, F, gs, (const double *)nc, nq, cand, rej);
    hipLaunchKernelGGL(km_certify_kernel<V4>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, X, N, ldx, C, K, F,
                       (const double *)nq, (const int *)cand, (const float *)rej, (const double *)ncmax,
                       exact_form_filter_bound(GT_SLAB), labels, dist, rechecked);
}

template <bool V4>
void km_sums_launch(const KmPlan &p, const float *X, int N, int F, long long ldx, const int *labels, int K, double *sums,
                    long long *counts, char *ws, hipStream_t s)
{
    int *hist = (int *)(ws + p.o_hist), *base = (int *)(ws + p.o_base), *rows = (int *)(ws + p.o_rows);
    int *segs = (int *)(ws + p.o_segs), *perm = (int *)(ws + p.o_perm);
    double *part = (double *)(ws + p.o_part);
    hipLaunchKernelGGL(km_hist_kernel, dim3(p.nb), dim3(KM_BLK), 0, s, labels, N, K, hist);
    hipLaunchKernelGGL(km_scan_kernel, dim3(K), dim3(64), 0, s, (const int *)hist, p.nb, K, base, counts);
    hipLaunchKernelGGL(km_offsets_kernel, dim3(1), dim3(64), 0, s, (const long long *)counts, K, rows, segs);
    hipLaunchKernelGGL(km_perm_kernel, dim3(p.nb), dim3(KM_BLK), 0, s, labels, N, K, (const int *)base, (const int *)rows, perm);
    hipLaunchKernelGGL(km_segsum_kernel<V4>, dim3(p.nseg, (F + 255) / 256), dim3(256), 0, s, X, ldx, F, p.FP, K,
                       (const int *)perm, (const int *)rows, (const int *)segs, part);
    hipLaunchKernelGGL(km_final_kernel, dim3(K, (F + 63) / 64), dim3(256), 0, s, (const double *)part, F, p.FP,
                       (const int *)segs, sums);
}

}  // namespace

extern "C" int64_t dm_kmeans_workspace_bytes(int64_t N, int F, int K)
{
    KmPlan p;
    if (km_plan(N, F, K, &p)) return -1;
    return (int64_t)p.total;
}

extern "C" int dm_kmeans_assign(const float *X, int64_t N, int F, int64_t ldx, const float *C, int K, const float *shift,
                                int32_t *labels, float *dist, int32_t *rechecked, void *workspace, int64_t workspace_bytes,
                                void *stream)
{
    DM_REQUIRE(X && C, "dm_kmeans_assign: X / C is NULL");
    DM_REQUIRE(labels && rechecked, "dm_kmeans_assign: labels / rechecked is NULL");
    DM_REQUIRE(workspace, "dm_kmeans_assign: workspace is NULL");
    KmPlan p;
    const char *why = km_plan(N, F, K, &p);
    DM_REQUIRE(!why, "dm_kmeans_assign: N = %lld, F = %d, K = %d: %s", (long long)N, F, K, why ? why : "");
    DM_REQUIRE(ldx >= F, "dm_kmeans_assign: leading dimension of X %lld < F = %d", (long long)ldx, F);
    DM_REQUIRE(workspace_bytes >= (int64_t)p.total, "dm_kmeans_assign: workspace of %lld bytes, need %lld",
               (long long)workspace_bytes, (long long)p.total);
    DM_REQUIRE(((uintptr_t)workspace & 255) == 0, "dm_kmeans_assign: workspace is not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const float *gs;
    if (const int e = shift_or_zeros("dm_kmeans_assign", shift, (char *)workspace + p.o_zero, F, s, &gs)) return e;
    if (vec4_ok(X, ldx, F) && vec4_ok(C, F, F) && ((uintptr_t)shift & 15) == 0)
        km_assign_launch<true>(p, X, (int)N, F, ldx, C, K, shift, gs, labels, dist, rechecked, (char *)workspace, s);
    else
        km_assign_launch<false>(p, X, (int)N, F, ldx, C, K, shift, gs, labels, dist, rechecked, (char *)workspace, s);
    return dm_launch_status("dm_kmeans_assign");
}

extern "C" int dm_kmeans_sums(const float *X, int64_t N, int F, int64_t ldx, const int32_t *labels, int K, double *sums,
                              int64_t *counts, void *workspace, int64_t workspace_bytes, void *stream)
{
    DM_REQUIRE(X && labels, "dm_kmeans_sums: X / labels is NULL");
    DM_REQUIRE(sums && counts, "dm_kmeans_sums: sums / counts is NULL");
    DM_REQUIRE(workspace, "dm_kmeans_sums: workspace is NULL");
    KmPlan p;
    const char *why = km_plan(N, F, K, &p);
    DM_REQUIRE(!why, "dm_kmeans_sums: N = %lld, F = %d, K = %d: %s", (long long)N, F, K, why ? why : "");
    DM_REQUIRE(ldx >= F, "dm_kmeans_sums: leading dimension of X %lld < F = %d", (long long)ldx, F);
    DM_REQUIRE(workspace_bytes >= (int64_t)p.total, "dm_kmeans_sums: workspace of %lld bytes, need %lld",
               (long long)workspace_bytes, (long long)p.total);
    DM_REQUIRE(((uintptr_t)workspace & 255) == 0, "dm_kmeans_sums: workspace is not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (vec4_ok(X, ldx, F))
        km_sums_launch<true>(p, X, (int)N, F, ldx, labels, K, sums, (long long *)counts, (char *)workspace, s);
    else
        km_sums_launch<false>(p, X, (int)N, F, ldx, labels, K, sums, (long long *)counts, (char *)workspace, s);
    return dm_launch_status("dm_kmeans_sums");
}

extern "C" int dm_kmeans_row_d2(const float *X, int64_t N, int F, int64_t ldx, const float *C, int K, const int32_t *labels,
                                double *d2, void *stream)
{
    DM_REQUIRE(X && C && d2, "dm_kmeans_row_d2: X / C / d2 is NULL");
    KmPlan p;
    const char *why = km_plan(N, F, K, &p);
    DM_REQUIRE(!why, "dm_kmeans_row_d2: N = %lld, F = %d, K = %d: %s", (long long)N, F, K, why ? why : "");
    DM_REQUIRE(ldx >= F, "dm_kmeans_row_d2: leading dimension of X %lld < F = %d", (long long)ldx, F);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((N + 3) / 4));
    if (vec4_ok(X, ldx, F) && vec4_ok(C, F, F))
        hipLaunchKernelGGL(km_row_d2_kernel<true>, grid, dim3(256), 0, s, X, (int)N, F, ldx, C, K, labels, d2);
    else
        hipLaunchKernelGGL(km_row_d2_kernel<false>, grid, dim3(256), 0, s, X, (int)N, F, ldx, C, K, labels, d2);
    return dm_launch_status("dm_kmeans_row_d2");
}
