// conv3x3_bwd.hip -- backward of a 3x3 convolution on a 16 x 16 latent grid that feeds a train-mode BatchNorm: data AND
// weight gradient in one pass.
//
// Reference: enc.10 = Conv2d(num_hiddens, num_hiddens, 3, padding=1) and the first convolution of every ResidualBlock layer,
// Conv2d(num_hiddens, num_residual_hiddens, 3, padding=1) (HiddenStateExtractor/vq_vae.py:287, 205), as autograd
// differentiates them for total_loss.backward() (run_training.py:406): aten::convolution_backward (input and weight) with
// BatchNorm's backward folded into the output gradient's load, the ReLU mask (and residual join) of the layer below and the
// reductions its BatchNorm backward needs in the epilogue.
//
// As two kernels (conv3x3_kernel + wgrad_kernel) each layer staged its output gradient -- two tensors of CD channels -- and its
// input twice.  A 16 x 16 latent with its zero padding fits LDS whole, so here a workgroup keeps ONE patch at a time,
//     da  [CD][18][24]   = c0*dy + c1*y + c2 inside the image, 0 in the padding      (BatchNorm backward; dm_operand AFFINE2)
//     T   [16][18][24]   = relu(c0x*x + c2x) (or relu(x)) inside, 0 in the padding   (what the forward multiplied)
// and runs both products on v_mfma_f32_16x16x4_f32:
//     data gradient    dx[ci][y][x] = [T > 0] * sum_{co,ky,kx} da[co][y+1-ky][x+1-kx] * W[co][ci][ky][kx]  (+ resid)
//                      M = the 16 positions of a row, N = ci, K = (tap, co): 9 * CD / 4 steps
//     weight gradient  dW[co][ci][ky][kx] = sum_{y,x} da[co][y][x] * T[ci][y+ky-1][x+kx-1]
//                      M = co (CD / 16 tiles), N = (ci, ky, kx) = 9 tiles, K = positions, four consecutive x per step
// plus the (sum dx, sum dx*q) slabs of the BatchNorm below.  CD = 16: 256 threads, two workgroups per CU; CD = 32: 512 threads
// (the transposed weights and the weight-gradient accumulators are 72 registers each), one workgroup per CU.
#include "dm_common.h"
#include "tile.h"

namespace {

constexpr int C3_HW = 16, C3_RS = 24, C3_ROWS = 18;
constexpr int C3_PS = C3_ROWS * C3_RS + 20;          // 452 == 4 (mod 32) dwords

// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4; LDS address = the first active lane's + 16 * lane)
__device__ __forceinline__ void c3_glds16(const float *g, float *l)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g, (__attribute__((address_space(3))) void *)l, 16, 0, 0);
}
// BAND (round 5): 32-column latent grids (32 x 32: 256-pixel patches, default-width VQ_VAE_z32) as tiles of 8 rows x 32 columns --
// 256 positions like the whole 16 x 16 patch, the same 16 M tiles (two per row), the zero padding left and right still the
// image border.  Only the rows above and below are REAL halo: two full rows per plane = 16 aligned 16-byte pieces, which go
// global -> LDS directly (global_load_lds, no registers: the kernel is at its register limit) into a side buffer of raw values;
// the wave that requested them transforms them into the padded image at the commit (zeros outside the image).
// (A first form with 16 x 16 tiles fetched 36 + 32 single halo elements per plane, the columns one cache line each: slower than
// the two kernels it replaced.)
constexpr int C3B_ROWS = 8, C3B_W = 32, C3B_H = 32, C3B_RS = 40;
constexpr int C3B_PS = (C3B_ROWS + 2) * C3B_RS + 28;            // 428: the weight gradient's B reads (ci, ky, kx, kq) fall on 32 distinct banks
constexpr int C3B_HALO = 2 * C3B_W;                             // floats per plane in the side buffer

// ---- what the kernels below share: the geometry, and every step that does not depend on how a kernel's loads leave or where
// ---- its commit sits.  The parts take the registers they work on as arguments (the kernels sit at 221 - 255 of 256 VGPRs: how state
// ---- is handed over decides whether they spill, HISTORY.md).
template <int CD_, int NTH_, bool BAND>
struct C3Geom {
    static constexpr int CD = CD_, NTH = NTH_, CX = 16, NW = NTH / 64, MT = CD / 16, KS = 9 * CD / 4, NTT = 9;
    static constexpr int ED = CD / NW, ET = CX / NW, RPW = C3_HW / NW;       // staged planes and M-tile rows per wave
    static constexpr int PS = BAND ? C3B_PS : C3_PS, RS = BAND ? C3B_RS : C3_RS, W = BAND ? C3B_W : C3_HW;
    static constexpr int H = BAND ? C3B_H : C3_HW, HW = H * W, bands = BAND ? H / C3B_ROWS : 1;     // tiles per patch
    static_assert(CD % 16 == 0 && CD % NW == 0 && CX % NW == 0, "whole planes per wave");
    // WLDS (CD = 32): the transposed weights wait in LDS in operand order ([K step][lane]: one conflict-free read per step, shared
    // by the two rows in flight) -- as 72 more registers beside the 72 accumulators they spilled 47
    static constexpr bool WLDS = CD > 16;
    static constexpr int NWREG = WLDS ? 1 : KS;
    static constexpr int LDS_FLOATS = (CD + CX) * PS + (WLDS ? KS * 64 : 0);          // the two tile images and the weights
    static_assert(NW * NTT * 256 <= (CD + CX) * PS, "the slab combine reuses the tile images");

    // M-tile row `y` (0..15) of the tile: image row / first column inside the tile (BAND: two M tiles per image row)
    static __device__ __forceinline__ int ry(int y) { return BAND ? y >> 1 : y; }
    static __device__ __forceinline__ int cx(int y) { return BAND ? 16 * (y & 1) : 0; }
    // tile k of this workgroup: patches blockIdx.x, blockIdx.x + gridDim.x, ...; BAND: the four bands of a patch one after the
    // other in ONE workgroup (a band's halo rows are its neighbours' interior rows: they are then re-read from this XCD's L2,
    // not by another one from HBM)
    static __device__ __forceinline__ int patch(int k) { return blockIdx.x + (k / bands) * gridDim.x; }
    static __device__ __forceinline__ void origin(int k, int &b, int &y0)
    {
        b = patch(k);
        y0 = (k % bands) * C3B_ROWS;
    }
    static __device__ __forceinline__ bool live(int k, int npatches) { return (int)blockIdx.x + (k / bands) * (int)gridDim.x < npatches; }
    // data gradient: K step s = (tap, channel group): the offset of its A operand from the row's first one
    static __device__ __forceinline__ constexpr int koff(int s)
    {
        const int tap = s / (CD / 4), cg = s - tap * (CD / 4), ky = tap / 3, kx = tap - 3 * ky;
        return 4 * cg * PS - ky * RS - kx;
    }
};

// The two load transforms for the planes e * NW + wave this wave stages: BatchNorm backward of the output gradient (the operand
// transform of tile.h: two fused multiply-adds), BatchNorm (+ ReLU) of the layer input (no xcoef: ReLU alone)
template <class G>
struct C3Coef {
    DyCoef dc[G::ED];
    float tc0[G::ET], tc2[G::ET];
    __device__ __forceinline__ f32x4 td(int e, f32x4 v, f32x4 u, bool two) const { return dy_commit(dc[e], v, u, two); }
    __device__ __forceinline__ f32x4 tx(int e, f32x4 r, bool affine) const
    {
        f32x4 v = tc0[e] * r + tc2[e];
        if (!affine) v = r;
        return dm_relu4(v);
    }
};

// ---- prologue.  (The clear of the weight-gradient accumulators stays in the kernels: behind a reference it becomes one wide
// ---- store and the kernels spill, HISTORY.md.)
template <class G>
__device__ __forceinline__ void c3_fill(float *lds3, const float *w, float *sW, int lane, int m, int kq, int wave, float (&wreg)[G::NWREG])
{
    constexpr int CD = G::CD, CX = G::CX;
    // the padding never changes: zero both tile images once (the commits write the interior only)
    for (int i = threadIdx.x; i < (CD + CX) * G::PS / 4; i += G::NTH) reinterpret_cast<f32x4 *>(lds3)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // data gradient: K step s = (tap, channel group), B[k = kq][n = ci = m] = W[co = 4 cg + kq][ci][ky][kx]
#pragma unroll
    for (int s = 0; s < G::KS; ++s) {
        const int tap = s / (CD / 4), cg = s - tap * (CD / 4);
        const float wv = w[((4 * cg + kq) * CX + m) * 9 + tap];
        if constexpr (G::WLDS) { if (wave == 0) sW[s * 64 + lane] = wv; } else wreg[s] = wv;
    }
}
template <class G>
__device__ __forceinline__ void c3_coefs(const float *dcoef, bool two, const float *xcoef, int wave, C3Coef<G> &co)
{
#pragma unroll
    for (int e = 0; e < G::ET; ++e) {
        const int c = e * G::NW + wave;
        co.tc0[e] = xcoef ? xcoef[c * 4] : 1.f;
        co.tc2[e] = xcoef ? xcoef[c * 4 + 2] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < G::ED; ++e) co.dc[e] = dy_coef(dcoef, two, e * G::NW + wave);
}
// weight gradient: B column n = 16 t + m = (ci, ky, kx): T[ci][y + ky - 1][x + kx - 1] <-> sT[ci*PS + (y + ky)*RS + x + kx + 3]
template <class G>
__device__ __forceinline__ void c3_boff(int m, int kq, int (&boff)[G::NTT])
{
#pragma unroll
    for (int t = 0; t < G::NTT; ++t) {
        const int n = 16 * t + m, ci = n / 9, k2 = n - ci * 9, ky = k2 / 3, kx = k2 - ky * 3;
        boff[t] = ci * G::PS + ky * G::RS + kx + 3 + kq;
    }
}
// staging: float4 (lane) of plane e * NW + wave: row lane >> 2, columns 4 (lane & 3) ..
// (BAND: row lane >> 3, columns 4 (lane & 7) .. of the 8 x 32 tile: 1 KB contiguous per plane)
template <class G>
__device__ __forceinline__ int c3_sq(int lane) { return G::bands > 1 ? 4 * lane : (lane >> 2) * C3_HW + 4 * (lane & 3); }     // offset inside the tile's plane
template <class G>
__device__ __forceinline__ int c3_sl(int lane)                                                                                  // ... inside its padded LDS image
{
    return G::bands > 1 ? ((lane >> 3) + 1) * G::RS + 4 + 4 * (lane & 7) : ((lane >> 2) + 1) * G::RS + 4 + 4 * (lane & 3);
}

// the staged tile out of the registers into the interior of the LDS images
template <class G>
__device__ __forceinline__ void c3_commit(float *sD, float *sT, int wave, int sl, const C3Coef<G> &co, bool two, bool affine,
                                          const f32x4 (&rv)[G::ED], const f32x4 (&ru)[G::ED], const f32x4 (&rx)[G::ET])
{
#pragma unroll
    for (int e = 0; e < G::ED; ++e) *reinterpret_cast<f32x4 *>(sD + (e * G::NW + wave) * G::PS + sl) = co.td(e, rv[e], ru[e], two);
#pragma unroll
    for (int e = 0; e < G::ET; ++e) *reinterpret_cast<f32x4 *>(sT + (e * G::NW + wave) * G::PS + sl) = co.tx(e, rx[e], affine);
}

// ---- weight gradient: this wave's rows, four positions per step
template <class G>
__device__ __forceinline__ void c3_wgrad_rows(const float *sD, const float *sT, const int (&boff)[G::NTT], int m, int kq, int wave,
                                              f32x4 (&wacc)[G::MT][G::NTT])
{
    constexpr int MT = G::MT, PS = G::PS, RS = G::RS;
#pragma unroll
    for (int rr = 0; rr < G::RPW; ++rr) {
        const int y = wave + G::NW * rr;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float a[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = sD[(16 * i + m) * PS + (G::ry(y) + 1) * RS + G::cx(y) + 4 * s + kq + 4];
#pragma unroll
            for (int t = 0; t < G::NTT; ++t) {
                const float bv = sT[boff[t] + G::ry(y) * RS + G::cx(y) + 4 * s];
#pragma unroll
                for (int i = 0; i < MT; ++i) wacc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bv, wacc[i][t], 0, 0, 0);
            }
        }
    }
}

// ---- data gradient: one M tile per row.  Lane (m, kq) holds positions x = 4 kq .. 4 kq + 3 of M-tile row y, channel ci = m:
// its A operand's first address, its element offset inside the patch's dx, and ReLU's mask of the layer below on its accumulator.
// (The K-step loop itself stays in the kernels: as a function of the row pair the 32-channel kernels spill, HISTORY.md.)
template <class G>
__device__ __forceinline__ const float *c3_arow(const float *sD, int m, int kq, int y)
{
    return sD + kq * G::PS + (G::ry(y) + 2) * G::RS + G::cx(y) + m + 5;
}
template <class G>
__device__ __forceinline__ int c3_out_off(int m, int kq, int y) { return m * G::HW + G::ry(y) * G::W + G::cx(y) + 4 * kq; }
template <class G>
__device__ __forceinline__ f32x4 c3_gated(const float *sT, int m, int kq, int y, f32x4 acc)
{
    return relu_gate4(*reinterpret_cast<const f32x4 *>(sT + m * G::PS + (G::ry(y) + 1) * G::RS + G::cx(y) + 4 + 4 * kq), acc);
}

// ---- the workgroup's slabs.  s_stat: [NW][CX][2] doubles
template <class G>
__device__ __forceinline__ void c3_finish(float *lds3, double *s_stat, int wave, int lane, double s1, double s2,
                                          const f32x4 (&wacc)[G::MT][G::NTT], double *stats, float *wslabs)
{
    constexpr int NW = G::NW, NTT = G::NTT, CX = G::CX;
    // statistics: the four kq groups of a channel, then the waves in wave order
    __syncthreads();
    if (stats) stat_fold<CX, true>(s_stat, wave, lane, s1, s2);
    __syncthreads();
    // weight gradient: every wave's accumulators through LDS, summed in wave order, one M tile of 16 output-gradient
    // channels at a time (the tile images are free now; all of CD = 32 at once would not fit them)
    float *red = lds3;                                           // [wave][NTT][64 lanes][4]
    if (stats) stat_slab<NW, CX, true>(s_stat, stats + (long long)blockIdx.x * CX * 2);
#pragma unroll
    for (int i = 0; i < G::MT; ++i) {
        if (i) __syncthreads();
#pragma unroll
        for (int t = 0; t < NTT; ++t) *reinterpret_cast<f32x4 *>(red + ((wave * NTT + t) * 64 + lane) * 4) = wacc[i][t];
        __syncthreads();
        // element e = dW[co = 16 i + c][n], n = (ci, ky, kx) = ci*9 + k2: accumulator row c = 4 kq + r, column n & 15 of N tile n >> 4
        for (int e = threadIdx.x; e < 16 * 144; e += G::NTH) {
            const int c = e / 144, n = e - c * 144;
            const int t = n >> 4, ln = (c >> 2) * 16 + (n & 15), r = c & 3;
            float sum = 0.f;
#pragma unroll
            for (int wv = 0; wv < NW; ++wv) sum += red[((wv * NTT + t) * 64 + ln) * 4 + r];
            wslabs[(long long)blockIdx.x * G::CD * 144 + (16 * i + c) * 144 + n] = sum;
        }
    }
}

template <int CD, int NTH, bool BAND = false>
__global__ __launch_bounds__(NTH, NTH == 512 ? 1 : 2)
void conv3x3_bwd_kernel(Operand dy, const float *__restrict__ x, const float *__restrict__ xcoef, const float *__restrict__ w,
                        const float *__restrict__ resid, const float *__restrict__ q, float *__restrict__ dx,
                        double *__restrict__ stats, float *__restrict__ wslabs, int ntiles)
{
    using G = C3Geom<CD, NTH, BAND>;
    constexpr int CX = G::CX, NW = G::NW, KS = G::KS, ED = G::ED, ET = G::ET, RPW = G::RPW;
    constexpr int PS = G::PS, RS = G::RS, W = G::W, H = G::H, HW = G::HW;
    extern __shared__ __attribute__((aligned(16))) float lds3[];
    __shared__ double s_stat[G::NW][G::CX][2];
    float *sD = lds3, *sT = lds3 + G::CD * G::PS, *sW = lds3 + (G::CD + G::CX) * G::PS;
    const int lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool two = dy.p1 != nullptr;
    float wreg[G::NWREG];
    c3_fill<G>(lds3, w, sW, lane, m, kq, wave, wreg);
    C3Coef<G> co;
    c3_coefs<G>(dy.coef, two, xcoef, wave, co);
    int boff[G::NTT];
    c3_boff<G>(m, kq, boff);
    f32x4 wacc[G::MT][G::NTT], rv[G::ED], ru[G::ED], rx[G::ET];          // the weight gradient; the staged tile
#pragma unroll
    for (int i = 0; i < G::MT; ++i)
#pragma unroll
        for (int t = 0; t < G::NTT; ++t) wacc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    double s1 = 0.0, s2 = 0.0;
    const int sq = c3_sq<G>(lane), sl = c3_sl<G>(lane);
    // BAND: raw halo rows of the planes this wave stages: [dy planes | y planes | x planes][2 rows][32]
    float *sHalo = lds3 + G::LDS_FLOATS;

    auto issue = [&](int t) {
        int b, y0;
        G::origin(t, b, y0);
        if constexpr (BAND) {
            // (addresses as a uniform 64-bit base + a 32-bit lane offset: the 64-bit per-lane pointers of the whole-patch form
            //  would not fit beside the accumulators here -- their spills' reloads wait for vmcnt(0) while LDS-DMA is in flight
            //  and with it for the stores of dx just issued: 249 us per layer instead of 204)
            const float *__restrict__ b0 = dy.p0 + (long long)b * CD * HW, *__restrict__ b1 = dy.p1 + (long long)b * CD * HW;
            const float *__restrict__ bx = x + (long long)b * CX * HW;
            const unsigned lo = (unsigned)(y0 * W + sq);
#pragma unroll
            for (int e = 0; e < ED; ++e) {
                const unsigned off = (unsigned)((e * NW + wave) * HW) + lo;
                rv[e] = *reinterpret_cast<const f32x4 *>(b0 + off);
                if (two) ru[e] = *reinterpret_cast<const f32x4 *>(b1 + off);
            }
#pragma unroll
            for (int e = 0; e < ET; ++e) rx[e] = *reinterpret_cast<const f32x4 *>(bx + ((unsigned)((e * NW + wave) * HW) + lo));
            // lanes 0..7 the row above, 8..15 the row below (a row outside the image: the nearest one inside, replaced by 0 at the commit)
            if (lane < 16) {
                const int yy = lane < 8 ? y0 - 1 : y0 + C3B_ROWS, yc = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
                const unsigned ho = (unsigned)(yc * W + 4 * (lane & 7));
#pragma unroll
                for (int e = 0; e < ED; ++e) {
                    const unsigned pl = (unsigned)((e * NW + wave) * HW) + ho;
                    c3_glds16(b0 + pl, sHalo + (e * NW + wave) * C3B_HALO + 4 * lane);
                    if (two) c3_glds16(b1 + pl, sHalo + (CD + e * NW + wave) * C3B_HALO + 4 * lane);
                }
#pragma unroll
                for (int e = 0; e < ET; ++e)
                    c3_glds16(bx + ((unsigned)((e * NW + wave) * HW) + ho), sHalo + (2 * CD + e * NW + wave) * C3B_HALO + 4 * lane);
            }
        } else {
            const long long db = (long long)b * CD * HW, xb = (long long)b * CX * HW;
#pragma unroll
            for (int e = 0; e < ED; ++e) {
                const long long off = db + (long long)(e * NW + wave) * HW + sq;
                rv[e] = *reinterpret_cast<const f32x4 *>(dy.p0 + off);
                if (two) ru[e] = *reinterpret_cast<const f32x4 *>(dy.p1 + off);
            }
#pragma unroll
            for (int e = 0; e < ET; ++e) rx[e] = *reinterpret_cast<const f32x4 *>(x + xb + (long long)(e * NW + wave) * HW + sq);
        }
    };
    int tile = 0;
    if (G::live(tile, ntiles)) issue(tile);
    __syncthreads();                                             // the zero fill is complete

    // BAND: the two barriers of the tile loop as raw s_barrier behind a wait for the LDS counter only.  With LDS-DMA requests
    // in flight hipcc's __syncthreads() waits for vmcnt(0): every tile would drain the stores of dx it has just issued
    // (measured: 249 us per layer with __syncthreads(), 204 us without any halo work).
    auto tile_barrier = [&]() {
        if constexpr (BAND) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        } else __syncthreads();
    };
    while (G::live(tile, ntiles)) {
        if (tile != 0) tile_barrier();                           // the previous tile has been consumed
        c3_commit<G>(sD, sT, wave, sl, co, two, xcoef != nullptr, rv, ru, rx);
        int b, ty0;
        G::origin(tile, b, ty0);
        if constexpr (BAND) {
            // the halo rows of this wave's planes: raw values from the side buffer (its own requests),
            // the same transforms, zeros outside the image.  LDS rows 0 and 9, columns 4 + 4 (lane & 7) ..
            // (counted: the only vector-memory operations issued after the requests and possibly still pending are the previous
            //  tile's RPW stores of dx -- vmcnt retires in issue order on gfx9 -- and a wait for 0 would drain them every tile)
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(RPW) : "memory");
            if (lane < 16) {
                const int yy = lane < 8 ? ty0 - 1 : ty0 + C3B_ROWS;
                const bool in = (unsigned)yy < (unsigned)H;
                const int lo = (lane < 8 ? 0 : C3B_ROWS + 1) * RS + 4 + 4 * (lane & 7);
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                // (plane by plane: reading every raw value first costs registers the kernel does not have -- 72 bytes of scratch, 309 us)
#pragma unroll
                for (int e = 0; e < ED; ++e) {
                    const f32x4 hv = *reinterpret_cast<const f32x4 *>(sHalo + (e * NW + wave) * C3B_HALO + 4 * lane);
                    const f32x4 hu = two ? *reinterpret_cast<const f32x4 *>(sHalo + (CD + e * NW + wave) * C3B_HALO + 4 * lane) : zero;
                    *reinterpret_cast<f32x4 *>(sD + (e * NW + wave) * PS + lo) = in ? co.td(e, hv, hu, two) : zero;
                }
#pragma unroll
                for (int e = 0; e < ET; ++e) {
                    const f32x4 r = *reinterpret_cast<const f32x4 *>(sHalo + (2 * CD + e * NW + wave) * C3B_HALO + 4 * lane);
                    // (its own copy of C3Coef::tx: through the function this form spills a float4, HISTORY.md)
                    f32x4 v = co.tc0[e] * r + co.tc2[e];
                    if (!xcoef) v = r;
                    *reinterpret_cast<f32x4 *>(sT + (e * NW + wave) * PS + lo) = in ? dm_relu4(v) : zero;
                }
            }
        }
        tile_barrier();
        ++tile;
        if (G::live(tile, ntiles)) issue(tile);                  // in flight during the products below

        c3_wgrad_rows<G>(sD, sT, boff, m, kq, wave, wacc);
        // ---- data gradient: two rows in flight
        const long long ob = (long long)b * CX * HW + ty0 * W;
#pragma unroll
        for (int rr = 0; rr < RPW; rr += 2) {
            f32x4 acc[2], rres[2], rq[2];
            const float *pa[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                const int yj = wave + NW * (rr + j);
                pa[j] = c3_arow<G>(sD, m, kq, yj);
                // the epilogue's side inputs are requested now: their latency passes under the products
                const long long o = ob + c3_out_off<G>(m, kq, yj);
                if (resid) rres[j] = *reinterpret_cast<const f32x4 *>(resid + o);
                if (stats && q) rq[j] = *reinterpret_cast<const f32x4 *>(q + o);
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const float wv = G::WLDS ? sW[s * 64 + lane] : wreg[G::WLDS ? 0 : s];
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[j][G::koff(s)], wv, acc[j], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int y = wave + NW * (rr + j);
                f32x4 v = c3_gated<G>(sT, m, kq, y, acc[j]);
                if (resid) v += rres[j];
                *reinterpret_cast<f32x4 *>(dx + ob + c3_out_off<G>(m, kq, y)) = v;
                if (stats) {
                    s1 += (double)pair_sum4(v);
                    s2 += (double)pair_dot4_rounded(v, q ? rq[j] : v);
                }
            }
        }
    }
    c3_finish<G>(lds3, &s_stat[0][0][0], wave, lane, s1, s2, wacc, stats, wslabs);
}

// COUNTED form (round 7) of the whole-patch kernel for CD = 32, the residual layers of the default model: the same staging,
// products and sums, bit for bit, with every load and store of the tile loop unconditional -- the next tile's loads leave through
// the descriptors of its patch, empty when there is no next tile, the epilogue's side inputs through descriptors that are empty
// when the tensor is not there (tile.h) -- so every wait inside the loop is counted and the stores of dx stay in flight behind
// the next commit (101.5 -> 96.7 us per layer at B = 2048).  conv3x3_bwd_kernel above waits for vmcnt(0) at its commit and in
// front of its stores and stays for the other two shapes: keeping the side inputs in flight across the products takes
// registers they do not have (the 16-channel form, whose transposed weights are registers, spills 56 bytes, the band form 64),
// and without that the rest gained them nothing (the 16-channel form: 54.8 -> 55.2 us).
template <int CD, int NTH>
__global__ __launch_bounds__(NTH, NTH == 512 ? 1 : 2)
void conv3x3_bwd_counted_kernel(Operand dy, const float *__restrict__ x, const float *__restrict__ xcoef, const float *__restrict__ w,
                        const float *__restrict__ resid, const float *__restrict__ q, float *__restrict__ dx,
                        double *__restrict__ stats, float *__restrict__ wslabs, int ntiles)
{
    using G = C3Geom<CD, NTH, false>;                            // (the whole patch is the tile)
    constexpr int CX = G::CX, NW = G::NW, KS = G::KS, ED = G::ED, ET = G::ET, RPW = G::RPW, HW = G::HW;
    extern __shared__ __attribute__((aligned(16))) float lds3[];
    __shared__ double s_stat[G::NW][G::CX][2];
    float *sD = lds3, *sT = lds3 + G::CD * G::PS, *sW = lds3 + (G::CD + G::CX) * G::PS;
    const int lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool two = dy.p1 != nullptr;
    float wreg[G::NWREG];
    c3_fill<G>(lds3, w, sW, lane, m, kq, wave, wreg);
    C3Coef<G> co;
    c3_coefs<G>(dy.coef, two, xcoef, wave, co);
    int boff[G::NTT];
    c3_boff<G>(m, kq, boff);
    f32x4 wacc[G::MT][G::NTT], rv[G::ED], ru[G::ED], rx[G::ET];          // the weight gradient; the staged tile
#pragma unroll
    for (int i = 0; i < G::MT; ++i)
#pragma unroll
        for (int t = 0; t < G::NTT; ++t) wacc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    double s1 = 0.0, s2 = 0.0;
    const int sq = c3_sq<G>(lane), sl = c3_sl<G>(lane);
    // Every load of the tile loop is unconditional: the next tile's leave through the descriptors of its patch, which are empty
    // when there is no next tile (tile.h; the second gradient tensor's also when there is no such tensor), so the commit's waits
    // are counted and the stores of dx just issued stay in flight behind them.
    auto issue = [&](int t, bool live) {
        const int b = G::patch(t);
        const __amdgpu_buffer_rsrc_t r0 = tile_rsrc(dy.p0, (long long)b * CD * HW, CD * HW, live);
        const __amdgpu_buffer_rsrc_t r1 = tile_rsrc(dy.p1, (long long)b * CD * HW, CD * HW, live && two);
        const __amdgpu_buffer_rsrc_t rX = tile_rsrc(x, (long long)b * CX * HW, CX * HW, live);
        const int lo = sq * 4;
#pragma unroll
        for (int e = 0; e < ED; ++e) {
            rv[e] = tile_load4(r0, (e * NW + wave) * HW * 4 + lo);
            ru[e] = tile_load4(r1, (e * NW + wave) * HW * 4 + lo);
        }
#pragma unroll
        for (int e = 0; e < ET; ++e) rx[e] = tile_load4(rX, (e * NW + wave) * HW * 4 + lo);
        __builtin_amdgcn_sched_barrier(0);                       // (the requests leave here, in this order, on every path)
    };
    // The commit of tile i + 1 closes the loop body of tile i (the first one: ahead of the loop): the only way to it leads
    // through tile i's requests and stores, so its waits are counted.  (At the head of the loop it is also reached from the
    // prologue, where no store follows the requests, and hipcc waits for the smaller count of the two paths: vmcnt(0).)
    int tile = 0;
    const bool any = G::live(tile, ntiles);
    issue(tile, any);
    __syncthreads();                                             // the zero fill is complete
    if (any) c3_commit<G>(sD, sT, wave, sl, co, two, xcoef != nullptr, rv, ru, rx);
    while (any) {
        __syncthreads();                                         // the tile images are complete
        const int b = G::patch(tile);
        ++tile;
        const bool more = G::live(tile, ntiles);
        issue(tile, more);                                       // in flight during the products below

        c3_wgrad_rows<G>(sD, sT, boff, m, kq, wave, wacc);
        // ---- data gradient: two rows in flight
        const long long ob = (long long)b * CX * HW;
        const __amdgpu_buffer_rsrc_t rR = tile_rsrc(resid, ob, CX * HW, resid != nullptr);
        const __amdgpu_buffer_rsrc_t rQ = tile_rsrc(q, ob, CX * HW, stats && q);
#pragma unroll
        for (int rr = 0; rr < RPW; rr += 2) {
            f32x4 acc[2], rres[2], rq[2];
            const float *pa[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                const int yj = wave + NW * (rr + j);
                pa[j] = c3_arow<G>(sD, m, kq, yj);
                // the epilogue's side inputs are requested now: their latency passes under the products
                // (unconditionally: a tensor that is not there has an empty descriptor)
                rres[j] = tile_load4(rR, c3_out_off<G>(m, kq, yj) * 4);
                rq[j] = tile_load4(rQ, c3_out_off<G>(m, kq, yj) * 4);
            }
            __builtin_amdgcn_sched_barrier(0);                   // (the requests AHEAD of the products: left to hipcc they sink below them)
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const float wv = G::WLDS ? sW[s * 64 + lane] : wreg[G::WLDS ? 0 : s];
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[j][G::koff(s)], wv, acc[j], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);                   // (and their first use BEHIND the products)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int y = wave + NW * (rr + j);
                f32x4 v = c3_gated<G>(sT, m, kq, y, acc[j]);
                // (a select, not a branch: hipcc sinks the load into a branch that holds its only use.  v + (-0) is v, bit for bit)
                v += resid ? rres[j] : (f32x4){-0.f, -0.f, -0.f, -0.f};
                *reinterpret_cast<f32x4 *>(dx + ob + c3_out_off<G>(m, kq, y)) = v;
                // (summed whether or not there is a statistics destination: a use inside a branch takes its load along)
                s1 += (double)pair_sum4(v);
                s2 += (double)pair_dot4_rounded(v, q ? rq[j] : v);
            }
        }
        if (!more) break;
        __syncthreads();                                         // this tile has been consumed
        c3_commit<G>(sD, sT, wave, sl, co, two, xcoef != nullptr, rv, ru, rx);
    }
#pragma unroll
    for (int e = 0; e < ED; ++e) { tile_keep(rv[e]); tile_keep(ru[e]); }
#pragma unroll
    for (int e = 0; e < ET; ++e) tile_keep(rx[e]);
    c3_finish<G>(lds3, &s_stat[0][0][0], wave, lane, s1, s2, wacc, stats, wslabs);
}

bool conv3x3_bwd_shape(int CD, int CX, int H, int W)
{
    if (!((CD == 16 || CD == 32) && CX == 16)) return false;
    if (H == C3_HW && W == C3_HW) return true;
    // 32 x 32: bands of 8 rows x 32 columns -- for the residual layers' 32 output-gradient channels (238 us per layer against the
    // two kernels' 267 at C5's shape); with 16 (enc.10) the two kernels are as fast (120 against 125 us) and stay
    return CD == 32 && W == C3B_W && H == C3B_H;
}
constexpr size_t conv3x3_bwd_lds(int CD, bool band = false)
{
    return ((size_t)(CD + 16) * (band ? C3B_PS : C3_PS) + (CD > 16 ? 9 * CD / 4 * 64 : 0) + (band ? (2 * CD + 16) * C3B_HALO : 0)) * sizeof(float);
}

}  // namespace

extern "C" int dm_conv3x3_bwd_fused_supported(int CD, int CX, int H, int W) { return conv3x3_bwd_shape(CD, CX, H, W) ? 1 : 0; }

extern "C" int dm_conv3x3_bwd_fused_num_blocks(int B, int CD, int CX, int H, int W)
{
    if (B <= 0 || !conv3x3_bwd_shape(CD, CX, H, W)) return -1;
    const int cap = CD == 32 ? 256 : 512;                        // resident workgroups: one / two per CU
    return B < cap ? B : cap;
}

extern "C" int dm_conv3x3_bwd_fused(const dm_operand *dy, const float *x, const float *xcoef, const float *w, const float *resid,
                                    const float *q, float *dx, double *stats, float *wslabs, int B, int CD, int CX, int H, int W,
                                    void *stream)
{
    DM_REQUIRE(dy && dy->p0 && x && w && dx && wslabs, "dm_conv3x3_bwd_fused: NULL pointer");
    DM_REQUIRE(B > 0 && conv3x3_bwd_shape(CD, CX, H, W), "dm_conv3x3_bwd_fused: shape %d -> %d channels on %dx%d not built", CX, CD, H, W);
    Operand d;
    if (dm_bwd_dy_operand(dy, "dm_conv3x3_bwd_fused", &d)) return -1;
    DM_REQUIRE(!q || stats, "dm_conv3x3_bwd_fused: q without a statistics destination");
    // (the band form reads the halo rows of a neighbouring band: dx written over an input would corrupt them)
    DM_REQUIRE(dx != dy->p0 && dx != dy->p1 && dx != x, "dm_conv3x3_bwd_fused: dx must not alias dy or x");
    const int grid = dm_conv3x3_bwd_fused_num_blocks(B, CD, CX, H, W);
    hipStream_t st = (hipStream_t)stream;
    static DmPerDeviceOnce attr_done;
    if (const int rc = dm_reserve_lds(attr_done, {{(const void *)conv3x3_bwd_counted_kernel<32, 512>, conv3x3_bwd_lds(32)},
                                                  {(const void *)conv3x3_bwd_kernel<16, 256>, conv3x3_bwd_lds(16)},
                                                  {(const void *)conv3x3_bwd_kernel<32, 512, true>, conv3x3_bwd_lds(32, true)}},
                                      "dm_conv3x3_bwd_fused"))
        return rc;
    const bool band = W != C3_HW;
    const int ntiles = B;                                        // (patches; BAND: four tiles each, taken by one workgroup)
    DM_REQUIRE((long long)B * (CD > CX ? CD : CX) * H * W < (1LL << 31), "dm_conv3x3_bwd_fused: tensor too large for 32-bit offsets");
    if (CD == 32 && band)
        hipLaunchKernelGGL((conv3x3_bwd_kernel<32, 512, true>), dim3(grid), dim3(512), conv3x3_bwd_lds(32, true), st, d, x, xcoef, w, resid,
                           q, dx, stats, wslabs, ntiles);
    else if (CD == 32)
        hipLaunchKernelGGL((conv3x3_bwd_counted_kernel<32, 512>), dim3(grid), dim3(512), conv3x3_bwd_lds(32), st, d, x, xcoef, w, resid, q, dx,
                           stats, wslabs, ntiles);
    else
        hipLaunchKernelGGL((conv3x3_bwd_kernel<16, 256>), dim3(grid), dim3(256), conv3x3_bwd_lds(16), st, d, x, xcoef, w, resid, q, dx,
                           stats, wslabs, ntiles);
    return dm_launch_status("dm_conv3x3_bwd_fused");
}
