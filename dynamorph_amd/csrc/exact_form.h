// exact_form.h -- the exact-form distance of a pair of fp32 rows, on the row loads of gram_tile.h: ONE definition for every
// kernel that evaluates it (knn.hip, kmeans.hip).  The files that include it are compiled with
// -ffp-contract=off: the vector and the scalar load forms, and every kernel that calls knn_exact_d2, produce the same bits.
#pragma once
#include "gram_tile.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------ the exact form
// d^2 of one pair by one wave: lane l takes features 4 l + 256 t .. + 3; differences and squares in fp32, the four squares of
// a step added in fp32 as (x^2 + y^2) + (z^2 + w^2), the steps in float64 in order, the lanes in a butterfly (every lane gets
// the sum).  No contraction: the vector and the scalar load forms, and every kernel that calls this, produce the same bits.
template <bool V4>
__device__ __forceinline__ double knn_exact_d2(const float *__restrict__ a, const float *__restrict__ b, int F, int lane)
{
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int f = 4 * lane; f < F; f += 256) {
        const f32x4 df = row_load4<V4>(a, f, F) - row_load4<V4>(b, f, F);
        const float x2 = df.x * df.x, y2 = df.y * df.y, z2 = df.z * df.z, w2 = df.w * df.w;
        acc += (double)((x2 + y2) + (z2 + w2));
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    return acc;
}

// The exact-form distance: the float64 sum's root, rounded to fp32 once.  It is the sort key AND the reported number.
__device__ __forceinline__ float knn_dist_of(double d2) { return (float)sqrt(d2); }

// The filter's error bound per unit of |q - s|^2 + |x - s|^2 for slabs of `slab` features summed in
// fp32 on the f32 matrix instruction: a slab of products and their sums, each operation with relative error <= 2^-23
// (round-to-nearest or truncation inside the matrix instruction), is off by at most gamma = n u / (1 - n u), n = slab + 2,
// times sum |a b| <= (|a|^2 + |b|^2) / 2, and g takes -2 of it; the slab sums, the norms and g itself are float64 (< 2^-36
// together); the rounding of g to fp32 (<= 2^-23 (1 + ...)) and of the shifted operands (<= (4 u + ...) = 2^-22 (1 + ...))
// fit into 2^-21.
inline double exact_form_filter_bound(int slab)
{
    const double n = slab + 2, u = 0x1p-23;
    return n * u / (1.0 - n * u) + 0x1p-21;
}

}  // namespace
