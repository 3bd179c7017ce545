// eig.hip -- Y = A Q in float64 for the partial eigensolver behind the latent PCA (dynamorph_amd/eig.py).
//
// A is n x n float64 (row-major, leading dimension lda), Q and Y are n x b float64 (ldq, ldy), b a multiple of 16 in 16 .. 256.
// Nothing here assumes A symmetric.
//   eig_apply_kernel<NT>   a workgroup (4 waves) owns EG_TM = 64 rows of A, all b = 16 NT columns and one range of the inner
//            dimension; wave w owns rows 16 w .. 16 w + 15 as NT accumulators of v_mfma_f64_16x16x4_f64.  Every element of A is
//            loaded once, by the one lane that multiplies it, straight into registers; the stage of Q (KS rows x b) is shared
//            through LDS.  The loads of stage st + 1 are issued before the matrix steps of stage st (knn_gram_kernel's order).
//            Within a stage a lane holds the inner indices k0 + 8 i + 2 g + e (g = lane >> 4, i < KS / 8, e < 2): a lane's pair
//            is one 16-byte load, and the four lane groups of a row read 64 consecutive bytes per instruction.
//   eig_reduce_kernel      more than one range: the partial products lie in the workspace and are added in range order.
// No atomics: the order of every sum is fixed by (n, b), so repeated launches are equal in every bit, whatever the leading
// dimensions.  The ranges are chosen from (n, b) for a part of 256 compute units, never from the device.
#include "dm_common.h"

namespace {

constexpr int EG_TM = 64;               // rows of A per workgroup (16 per wave)
constexpr int EG_TARGET = 512;          // workgroups wanted: two per compute unit of a 256-CU part
constexpr int EG_MIN_RANGE = 256;       // a range of the inner dimension is at least this long

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

template <int NT>
struct EgShape {
    static constexpr int B = 16 * NT;                       // columns
    static constexpr int KS = NT <= 4 ? 32 : 16;            // inner indices per LDS stage
    static constexpr int LW = B + 8;                        // LDS row stride: lane groups g and g + 1 (2 rows apart) land 16 banks apart
    static constexpr int QR = KS * B / 256;                 // doubles of the Q stage a thread carries
    static constexpr int AP = KS / 8;                       // pairs of A a lane carries per stage
    static constexpr size_t LDS = (size_t)2 * KS * LW * sizeof(double);
};

constexpr int eg_stage(int64_t b) { return b <= 64 ? 32 : 16; }

template <int NT>
__global__ __launch_bounds__(256) void eig_apply_kernel(const double *__restrict__ A, long long n, long long lda,
                                                        const double *__restrict__ Q, long long ldq,
                                                        double *__restrict__ out, long long ldo, long long split_stride,
                                                        long long range, int vec)
{
    using S = EgShape<NT>;
    constexpr int KS = S::KS, LW = S::LW, QR = S::QR, AP = S::AP, B = S::B;
    extern __shared__ __attribute__((aligned(16))) double eg_lds[];     // [2][KS][LW]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, g = lane >> 4;
    const long long I = (long long)blockIdx.x * EG_TM;
    const long long kbeg = (long long)blockIdx.y * range;
    const long long kend = kbeg + range < n ? kbeg + range : n;
    long long row = I + 16 * w + r;
    if (row >= n) row = n - 1;                              // (rows past n repeat the last row: nothing of theirs is stored)
    const double *__restrict__ arow = A + row * lda;
    const int nstages = (int)((kend - kbeg + KS - 1) / KS);

    double a[2][2 * AP], q[QR];
    // Stage `st` of A into register slot `slot`, and of Q into q.  A whole stage inside the range: plain loads; the last one
    // (and anything past the end) index by index, zeros past kend.
    auto fetch = [&](int st, int slot) {
        const long long k0 = kbeg + (long long)st * KS;
        if (k0 + KS <= kend) {
#pragma unroll
            for (int i = 0; i < AP; ++i) {
                const long long k = k0 + 8 * i + 2 * g;
                if (vec) {
                    const f64x2 v = *reinterpret_cast<const f64x2 *>(arow + k);
                    a[slot][2 * i] = v.x;
                    a[slot][2 * i + 1] = v.y;
                } else {
                    a[slot][2 * i] = arow[k];
                    a[slot][2 * i + 1] = arow[k + 1];
                }
            }
#pragma unroll
            for (int i = 0; i < QR; ++i) {
                const int e = tid + 256 * i;
                q[i] = Q[(k0 + e / B) * ldq + e % B];
            }
        } else {
#pragma unroll
            for (int i = 0; i < AP; ++i) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const long long k = k0 + 8 * i + 2 * g + e;
                    a[slot][2 * i + e] = k < kend ? arow[k] : 0.0;
                }
            }
#pragma unroll
            for (int i = 0; i < QR; ++i) {
                const int e = tid + 256 * i;
                const long long k = k0 + e / B;
                q[i] = k < kend ? Q[k * ldq + e % B] : 0.0;
            }
        }
    };
    auto stash = [&](int buf) {
        double *dst = eg_lds + buf * KS * LW;
#pragma unroll
        for (int i = 0; i < QR; ++i) {
            const int e = tid + 256 * i;
            dst[(e / B) * LW + e % B] = q[i];
        }
    };

    f64x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = (f64x4){0.0, 0.0, 0.0, 0.0};

    fetch(0, 0);
    stash(0);
    __syncthreads();
    for (int st0 = 0; st0 < nstages; st0 += 2) {            // (an odd count: the last pair's second stage multiplies zeros)
#pragma unroll
        for (int u = 0; u < 2; ++u) {                       // stage st lives in register slot u and LDS buffer u
            const int st = st0 + u;
            fetch(st + 1, u ^ 1);                           // (past the end: zeros, no loads)
            __builtin_amdgcn_sched_barrier(0);              // the loads are issued here, not after the products
            const double *Bq = eg_lds + u * KS * LW + 2 * g * LW + r;
#pragma unroll
            for (int i = 0; i < AP; ++i) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const double av = a[u][2 * i + e];
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bq[(8 * i + e) * LW + 16 * j], acc[j], 0, 0, 0);
                }
            }
            stash(u ^ 1);
            __syncthreads();
        }
    }

    // C/D map of the f64 instruction: column lane & 15, row (lane >> 4) + 4 reg
    double *__restrict__ o = out + (long long)blockIdx.y * split_stride;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long long orow = I + 16 * w + g + 4 * e;
        if (orow < n) {
#pragma unroll
            for (int j = 0; j < NT; ++j) o[orow * ldo + 16 * j + r] = acc[j][e];
        }
    }
}

// Y[row][col] = part[0][row][col] + part[1][row][col] + ... in range order; part: splits x n x b, contiguous.
__global__ __launch_bounds__(256) void eig_reduce_kernel(const double *__restrict__ part, long long n, int b, int splits,
                                                         double *__restrict__ Y, long long ldy)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = n * b;
    if (idx >= total) return;
    double s = part[idx];
    for (int k = 1; k < splits; ++k) s += part[(long long)k * total + idx];
    Y[(idx / b) * ldy + idx % b] = s;
}

size_t eg_align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct EgPlan {
    int row_tiles, splits, stage;
    long long range;
    size_t ws;
};

// 0, or the reason the shape is refused.  A function of (n, b) alone.
const char *eg_plan(int64_t n, int64_t b, EgPlan *p)
{
    if (n < 1 || n > 0x7fffffffLL - EG_TM) return "n outside 1 .. 2^31 - 65";
    if (b < 16 || b > DM_EIG_MAX_BLOCK || b % 16) return "b is not a multiple of 16 in 16 .. DM_EIG_MAX_BLOCK";
    const long long tiles = (n + EG_TM - 1) / EG_TM;
    long long s = (EG_TARGET + tiles - 1) / tiles;
    const long long most = (n + EG_MIN_RANGE - 1) / EG_MIN_RANGE;
    if (s > most) s = most;
    if (s < 1) s = 1;
    const long long range = ((n + s - 1) / s + 31) / 32 * 32;      // whole stages of either length
    s = (n + range - 1) / range;
    p->row_tiles = (int)tiles;
    p->splits = (int)s;
    p->stage = eg_stage(b);
    p->range = range;
    p->ws = s > 1 ? eg_align256((size_t)s * (size_t)n * (size_t)b * sizeof(double)) : 256;
    return nullptr;
}

template <int NT>
void eg_launch(const EgPlan &p, const double *A, long long n, long long lda, const double *Q, long long ldq, double *out,
               long long ldo, long long split_stride, int vec, hipStream_t s)
{
    hipLaunchKernelGGL(eig_apply_kernel<NT>, dim3(p.row_tiles, p.splits), dim3(256), EgShape<NT>::LDS, s, A, n, lda, Q, ldq, out,
                       ldo, split_stride, p.range, vec);
}

DmPerDeviceOnce g_eg_once;

}  // namespace

extern "C" int64_t dm_eig_apply_workspace_bytes(int64_t n, int64_t b)
{
    EgPlan p;
    if (eg_plan(n, b, &p)) return -1;
    return (int64_t)p.ws;
}

extern "C" int dm_eig_apply_plan(int64_t n, int64_t b, int *row_tiles, int *splits, int *tile_rows, int *stage)
{
    EgPlan p;
    const char *why = eg_plan(n, b, &p);
    DM_REQUIRE(!why, "dm_eig_apply_plan: n = %lld, b = %lld: %s", (long long)n, (long long)b, why ? why : "");
    if (row_tiles) *row_tiles = p.row_tiles;
    if (splits) *splits = p.splits;
    if (tile_rows) *tile_rows = EG_TM;
    if (stage) *stage = p.stage;
    return 0;
}

extern "C" int dm_eig_apply(const double *A, int64_t n, int64_t lda, const double *Q, int64_t b, int64_t ldq, double *Y,
                            int64_t ldy, void *ws, size_t ws_bytes, void *stream)
{
    DM_REQUIRE(A && Q && Y, "dm_eig_apply: A / Q / Y is NULL");
    DM_REQUIRE(ws, "dm_eig_apply: workspace is NULL");
    EgPlan p;
    const char *why = eg_plan(n, b, &p);
    DM_REQUIRE(!why, "dm_eig_apply: n = %lld, b = %lld: %s", (long long)n, (long long)b, why ? why : "");
    DM_REQUIRE(lda >= n, "dm_eig_apply: leading dimension of A %lld < n = %lld", (long long)lda, (long long)n);
    DM_REQUIRE(ldq >= b, "dm_eig_apply: leading dimension of Q %lld < b = %lld", (long long)ldq, (long long)b);
    DM_REQUIRE(ldy >= b, "dm_eig_apply: leading dimension of Y %lld < b = %lld", (long long)ldy, (long long)b);
    DM_REQUIRE(ws_bytes >= p.ws, "dm_eig_apply: workspace of %llu bytes, need %llu", (unsigned long long)ws_bytes,
               (unsigned long long)p.ws);
    DM_REQUIRE(((uintptr_t)ws & 255) == 0, "dm_eig_apply: workspace is not 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
#define EG_NEED(NT) {(const void *)eig_apply_kernel<NT>, EgShape<NT>::LDS}
    if (const int rc = dm_reserve_lds(g_eg_once, {EG_NEED(1), EG_NEED(2), EG_NEED(3), EG_NEED(4), EG_NEED(5), EG_NEED(6),
                                                  EG_NEED(7), EG_NEED(8), EG_NEED(9), EG_NEED(10), EG_NEED(11), EG_NEED(12),
                                                  EG_NEED(13), EG_NEED(14), EG_NEED(15), EG_NEED(16)}, "dm_eig_apply"))
        return rc;
#undef EG_NEED
    const int vec = ((uintptr_t)A & 15) == 0 && (lda & 1) == 0;
    const bool split = p.splits > 1;
    double *out = split ? (double *)ws : Y;
    const long long ldo = split ? b : ldy, stride = split ? (long long)n * b : 0;
    switch ((int)(b / 16)) {
#define EG_CASE(NT) case NT: eg_launch<NT>(p, A, n, lda, Q, ldq, out, ldo, stride, vec, s); break;
        EG_CASE(1) EG_CASE(2) EG_CASE(3) EG_CASE(4) EG_CASE(5) EG_CASE(6) EG_CASE(7) EG_CASE(8)
        EG_CASE(9) EG_CASE(10) EG_CASE(11) EG_CASE(12) EG_CASE(13) EG_CASE(14) EG_CASE(15) EG_CASE(16)
#undef EG_CASE
    }
    if (split) {
        const long long total = (long long)n * b;
        hipLaunchKernelGGL(eig_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const double *)ws,
                           (long long)n, (int)b, p.splits, Y, (long long)ldy);
    }
    return dm_launch_status("dm_eig_apply");
}
