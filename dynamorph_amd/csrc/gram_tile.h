// gram_tile.h -- what the four 128-wide f32 Gram-tile kernels on v_mfma_f32_32x32x2_f32 share: gram_kernel and rowgram_kernel
// (pca.hip), knn_gram_kernel (knn.hip), km_filter_kernel (kmeans.hip).  The certificates of the k-NN graph and of k-means
// (DESIGN.md sections 3.5b, 3.5f, 3.5g) are proofs about these kernels' loop: operands fl(x - s), fp32 sums within a slab of
// GT_SLAB features, float64 across the slabs in feature order.  Here, once: the tile, the stage, the LDS stride and the slab
// (exact_form_filter_bound(GT_SLAB) is the bound of every one of them); the row loads the operands come through; the C/D map
// of the matrix instruction; the norms |x - s|^2 of the filter and their maximum; the host side around the launches.
// The loop itself -- accumulator clear, fetch / stash, the 2 x 2 products, the slab fold -- is still written out in each
// kernel: behind a function (accumulators by reference, or the whole loop with its accumulators inside) hipcc allocates other
// registers for the same source text (HISTORY.md, "One header for the four f32 Gram-tile kernels", has the forms tried).
// Nothing in this file multiplies and then adds in fp32: it compiles to the same operations with and without
// -ffp-contract=off (pca.o is built without, knn.o and kmeans.o with).
#pragma once
#include "dm_common.h"

namespace {

constexpr int GT = 128;                 // tile edge: a workgroup computes a 128-wide block
constexpr int GT_CH = 16;               // depth of one LDS stage (8 k-steps of the 32x32x2 instruction)
constexpr int GT_LW = GT + 32;          // LDS row stride: the two lane halves of a read (depths k, k + 1) land 32 banks apart
constexpr int GT_SLAB = 256;            // features accumulated in fp32 before the partial sum is added in float64
static_assert(GT_SLAB == DM_PCA_ROWGRAM_SLAB_FEATURES, "the certificates' slab is the row Gram's");
static_assert(GT_SLAB % GT_CH == 0, "a slab is a whole number of LDS stages");
constexpr int GT_SLOTS = 256;           // workgroups resident at once on a 256-CU part (one per CU: 316 registers per lane)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ----------------------------------------------------------------------------------------------------- row loads
// The 16-byte form of every kernel: rows start on 16 bytes and are a whole number of float4s.
bool vec4_ok(const float *p, long long ld, int F) { return ld % 4 == 0 && F % 4 == 0 && ((uintptr_t)p & 15) == 0; }
// ... of the kernels that take the features past a multiple of four one by one: rows start on 16 bytes.
bool vec4_ok(const float *p, long long ld) { return ld % 4 == 0 && ((uintptr_t)p & 15) == 0; }

// Four consecutive features f .. f + 3 of a row, f < F, zero past F (V4: F % 4 == 0, nothing lies past it).
template <bool V4>
__device__ __forceinline__ f32x4 row_load4(const float *__restrict__ row, int f, int F)
{
    if (V4) return *(const f32x4 *)(row + f);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (f + e < F) v[e] = row[f + e];
    return v;
}

__device__ __forceinline__ f32x4 shift_load4(const float *__restrict__ shift, int f, int F)
{
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (shift) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (f + e < F) s[e] = shift[f + e];
    }
    return s;
}

// The same four features without a branch, for loads that must not be waited for where they are issued: addresses past F
// are clamped into the row and the caller discards those elements.  V4: the 16-byte form, F % 4 == 0 and F >= 4.
template <bool V4>
__device__ __forceinline__ f32x4 row_load4_clamped(const float *__restrict__ row, int f, int F)
{
    if (V4) return *(const f32x4 *)(row + (f < F ? f : F - 4));
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[f + e < F ? f + e : F - 1];
    return v;
}

// ------------------------------------------------------------------------------------------------- the C/D map
// C/D map of the 32x32 instructions: element e of a lane is row (e & 3) + 8 (e >> 2) + 4 (lane >> 5), column lane & 31, of the
// 32 x 32 block whose first row / column is `base`.  (base comes first in the sum: the kernels' address arithmetic was
// written that way, and `gt_row(e, lane)` added to a base afterwards compiles to other instructions.)
__device__ __forceinline__ int gt_row(int base, int e, int lane) { return base + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ int gt_col(int base, int lane) { return base + (lane & 31); }

// ------------------------------------------------------------------------------------------ norms and their maximum
// One wave per row: sum_f fl(x_f - s_f)^2, the squares and the sum in float64 (the squares of fp32 numbers are exact there),
// lanes added in a butterfly.
template <bool V4>
__global__ __launch_bounds__(256) void row_norms_kernel(const float *__restrict__ X, long long rows, int F, long long ld,
                                                        const float *__restrict__ shift, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float *__restrict__ row = X + r * ld;
    double acc = 0.0;
    for (int f = 4 * lane; f < F; f += 256) {
        const f32x4 v = row_load4<V4>(row, f, F) - shift_load4(shift, f, F);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += (double)v[e] * (double)v[e];
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) out[r] = acc;
}

// The largest of n norms (one workgroup of NT = 256); thread 0 also clears the call's counter (fallback rows, rechecked rows).
// (A template, so that a file that includes this header and does not launch it -- pca.hip -- gets no kernel from it.)
template <int NT>
__global__ __launch_bounds__(NT) void norms_max_kernel(const double *__restrict__ v, long long n, double *__restrict__ out,
                                                       int *__restrict__ counter)
{
    static_assert(NT == 256, "the tree below starts at 128");
    __shared__ double s[256];
    double m = 0.0;
    for (long long i = threadIdx.x; i < n; i += 256) m = fmax(m, v[i]);
    s[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) { *out = s[0]; *counter = 0; }
}

// ------------------------------------------------------------------------------------------------------- host
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// The filter's loads are unconditional: no shift = a vector of F zeros, cleared here at `zeros` (in the call's workspace).
// *filter_shift is what the filter kernel reads.  0, or the HIP error with the message set under the entry point's name.
int shift_or_zeros(const char *who, const float *shift, void *zeros, int F, hipStream_t s, const float **filter_shift)
{
    *filter_shift = shift ? shift : (const float *)zeros;
    if (shift) return 0;
    const hipError_t e = hipMemsetAsync(zeros, 0, (size_t)F * sizeof(float), s);
    if (e != hipSuccess) dm_set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    return (int)e;
}

// Upper-triangular tile pairs (ti <= tj) of T tiles, row by row: the pair of an index, the index of a pair.
__device__ __forceinline__ void pair_of(int p, int T, int &ti, int &tj)
{
    ti = 0;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    tj = ti + p;
}
__device__ __forceinline__ long long pair_index(int ta, int tb, int T)
{
    return (long long)ta * T - (long long)ta * (ta - 1) / 2 + (tb - ta);
}

// `pairs` tile pairs whose inner dimension has `nslabs` slabs: the inner dimension is cut into S ranges of slabs_per slabs,
// one workgroup per (pair, range).  S is the split whose last wave of workgroups is fullest (ties: the smaller S), capped by
// the slabs there are and by a 2 GiB workspace; direct_pairs > 0: from that many pairs on the pairs fill the part, S = 1.
// The split depends on the shape only, never on the device, so the summation order -- and the result -- is a function of
// the data alone.
struct SplitPlan { int S; long long slabs_per; };

SplitPlan split_plan(long long pairs, long long nslabs, long long direct_pairs)
{
    const long long tile_bytes = (long long)GT * GT * 8;
    int best = 1;
    double best_eff = 0.0;
    for (int s = 1; (!direct_pairs || pairs < direct_pairs) && s <= 64 && s <= nslabs; ++s) {
        if (s > 1 && (long long)s * pairs * tile_bytes > (2LL << 30)) break;
        const long long blocks = (long long)s * pairs;
        const double eff = (double)blocks / (double)(((blocks + GT_SLOTS - 1) / GT_SLOTS) * GT_SLOTS);
        if (eff > best_eff + 1e-9) { best_eff = eff; best = s; }
    }
    SplitPlan p;
    p.slabs_per = (nslabs + best - 1) / best;
    p.S = (int)((nslabs + p.slabs_per - 1) / p.slabs_per);
    return p;
}

}  // namespace
