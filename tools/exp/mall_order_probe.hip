// mall_order_probe.hip -- does the ORDER in which a consumer walks its tiles, relative to the producer before it, decide how much
// of the shared tensor it finds in the 256 MiB Infinity Cache?
//
//   hipcc -O3 --offload-arch=gfx950 -o mall_order_probe mall_order_probe.hip && ./mall_order_probe
//
// A producer streams `in` -> T over a grid-stride tile walk (768 workgroups, ascending).  A consumer launched straight after it
// reads T and NSEC further buffers of T's size over the same walk, once ascending and once descending (tile id ntiles - 1 - k-th).
// The accesses are the conv staging's: a tile is a [16 planes][8 rows][32 floats] patch of a [16][128][128] sample, a lane loads
// 16 bytes, 8 lanes cover one 128-byte row segment, a workgroup covers the tile in four passes of four planes.
// Same-order streaming puts (1-f)*P + f*C bytes between the two uses of the line at fraction f of T (P, C: producer's and
// consumer's traffic), reversed streaming u*(P + C) for the line a fraction u from the end: the model says everything with
// u < 256 MiB / (P + C) hits when the consumer walks down, nothing when it walks up.
//
// Cases: T = 256 MiB, P = 512 (256 in), C = 512 (T + one buffer)      -- the conv pairs of the training step
//        T = 128 MiB, P = 192 (64 in),  C = 512 (T + three buffers)   -- dec.2 forward -> decoder tail
// The consumer is timed with stream events, REPS repetitions per order, alternating, the producer re-run before every one.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int BLOCK = 256, GRID = 768, REPS = 12;
constexpr int SW = 128, SH = 128, SC = 16;                 // sample: [16][128][128] floats = 1 MiB
constexpr int TH = 8, TW = 32;                             // tile: 16 planes x 8 rows x 128 bytes = 16 KiB
constexpr int TILES_X = SW / TW, TILES_Y = SH / TH, TILES_PER_SAMPLE = TILES_X * TILES_Y;
constexpr long long SAMPLE = (long long)SC * SH * SW;      // floats

// float offset of this thread's element of pass p of tile t (pass p: planes 4p .. 4p+3)
__device__ __forceinline__ long long elem_of(int t, int p)
{
    const int x0 = (t % TILES_X) * TW, y0 = ((t / TILES_X) % TILES_Y) * TH, b = t / TILES_PER_SAMPLE;
    const int j4 = threadIdx.x & 7, r = (threadIdx.x >> 3) & 7, c = 4 * p + (threadIdx.x >> 6);
    return b * SAMPLE + ((long long)(c * SH + y0 + r) * SW + x0 + 4 * j4);
}

// in_passes of the tile's four passes are read (the others written from registers): P = (in_passes / 4 + 1) * |T|
__global__ __launch_bounds__(BLOCK, 3)
void producer(const float *__restrict__ in, float *__restrict__ T, int ntiles, int in_passes)
{
    for (int k = blockIdx.x; k < ntiles; k += gridDim.x) {
        f32x4 v[4];
#pragma unroll
        for (int p = 0; p < 4; ++p)
            v[p] = p < in_passes ? *reinterpret_cast<const f32x4 *>(in + elem_of(k, p)) : (f32x4){1.f, 2.f, 3.f, 4.f};
#pragma unroll
        for (int p = 0; p < 4; ++p) *reinterpret_cast<f32x4 *>(T + elem_of(k, p)) = v[p] + 1.f;
    }
}

template <int NSEC, bool DESC>
__global__ __launch_bounds__(BLOCK, 3)
void consumer(const float *__restrict__ T, const float *__restrict__ sec, long long sec_stride, float *__restrict__ out, int ntiles)
{
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = blockIdx.x; k < ntiles; k += gridDim.x) {
        const int t = DESC ? ntiles - 1 - k : k;
        f32x4 v[4], u[NSEC][4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const long long e = elem_of(t, p);
            v[p] = *reinterpret_cast<const f32x4 *>(T + e);
#pragma unroll
            for (int s = 0; s < NSEC; ++s) u[s][p] = *reinterpret_cast<const f32x4 *>(sec + s * sec_stride + e);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            acc += v[p];
#pragma unroll
            for (int s = 0; s < NSEC; ++s) acc += u[s][p];
        }
    }
    *reinterpret_cast<f32x4 *>(out + ((long long)blockIdx.x * BLOCK + threadIdx.x) * 4) = acc;
}

template <int NSEC>
static void run_case(const char *name, int t_mib, int in_passes, float *in, float *T, float *sec, float *out)
{
    const int ntiles = t_mib * TILES_PER_SAMPLE;           // 1 MiB per sample
    const long long stride = (long long)t_mib * SAMPLE;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<float> us[2];
    for (int rep = -2; rep < 2 * REPS; ++rep) {            // two warm-up rounds
        const int desc = rep & 1;
        producer<<<GRID, BLOCK>>>(in, T, ntiles, in_passes);
        CHECK(hipEventRecord(e0));
        if (desc) consumer<NSEC, true><<<GRID, BLOCK>>>(T, sec, stride, out, ntiles);
        else consumer<NSEC, false><<<GRID, BLOCK>>>(T, sec, stride, out, ntiles);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (rep >= 0) us[desc].push_back(ms * 1e3f);
    }
    const double c_mib = (double)t_mib * (1 + NSEC), p_mib = t_mib * (1.0 + in_passes / 4.0);
    printf("case %s: T = %d MiB, P = %.0f MiB, C = %.0f MiB, P + C = %.0f MiB, %d tiles of 16 KiB, %d workgroups\n", name, t_mib, p_mib,
           c_mib, p_mib + c_mib, ntiles, GRID);
    double med[2], spread[2];
    for (int d = 0; d < 2; ++d) {
        printf("  %-10s us:", d ? "descending" : "ascending");
        for (float v : us[d]) printf(" %.1f", v);
        std::vector<float> s = us[d];
        std::sort(s.begin(), s.end());
        med[d] = 0.5 * (s[s.size() / 2] + s[(s.size() - 1) / 2]);
        spread[d] = s.back() - s.front();
        printf("\n  %-10s min %.1f  median %.1f  max %.1f  spread %.1f us   %.2f TB/s at the median\n", "", s.front(), med[d], s.back(),
               spread[d], c_mib * 1048576.0 / (med[d] * 1e-6) / 1e12);
    }
    const double gain = med[0] - med[1], sp = std::max(spread[0], spread[1]);
    const double model_hit = std::min(1.0, 256.0 / (p_mib + c_mib)) * t_mib;
    printf("  descending is %.1f us (%.1f %%) %s than ascending; larger spread of one order %.1f us; model: %.0f MiB of T hit -> %s\n",
           gain < 0 ? -gain : gain, 100.0 * (gain < 0 ? -gain : gain) / med[0], gain < 0 ? "SLOWER" : "faster", sp, model_hit,
           gain > sp ? "ORDER MATTERS" : "no effect beyond the spread");
    CHECK(hipEventDestroy(e0));
    CHECK(hipEventDestroy(e1));
}

int main()
{
    const size_t MiB = 1048576;
    float *in, *T, *sec, *out;
    CHECK(hipMalloc(&in, 256 * MiB));
    CHECK(hipMalloc(&T, 256 * MiB));
    CHECK(hipMalloc(&sec, 384 * MiB));
    CHECK(hipMalloc(&out, (size_t)GRID * BLOCK * 16));
    CHECK(hipMemset(in, 0, 256 * MiB));
    CHECK(hipMemset(sec, 0, 384 * MiB));
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    printf("mall_order_probe on %s (%s), %d CUs, %d repetitions per order, alternating\n", prop.name, prop.gcnArchName,
           prop.multiProcessorCount, REPS);
    run_case<1>("conv pair", 256, 4, in, T, sec, out);
    run_case<3>("dec.2 -> tail", 128, 2, in, T, sec, out);
    CHECK(hipDeviceSynchronize());
    CHECK(hipFree(in)); CHECK(hipFree(T)); CHECK(hipFree(sec)); CHECK(hipFree(out));
    return 0;
}
