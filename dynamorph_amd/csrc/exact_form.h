// exact_form.h -- the exact-form distance of a pair of fp32 rows and the row loads it is built from: ONE definition for every
// kernel that evaluates it (knn.hip, kmeans.hip).  The files that include it are compiled with
// -ffp-contract=off: the vector and the scalar load forms, and every kernel that calls knn_exact_d2, produce the same bits.
#pragma once
#include "dm_common.h"
#include <math.h>

namespace {

// The 16-byte form of every kernel: rows start on 16 bytes and are a whole number of float4s.
bool vec4_ok(const float *p, long long ld, int F) { return ld % 4 == 0 && F % 4 == 0 && ((uintptr_t)p & 15) == 0; }

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
// are clamped into the row and the caller discards those elements.
template <bool V4>
__device__ __forceinline__ f32x4 row_load4_clamped(const float *__restrict__ row, int f, int F)
{
    if (V4) return *(const f32x4 *)(row + (f < F ? f : F - 4));
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = row[f + e < F ? f + e : F - 1];
    return v;
}

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
