// wide_host.h -- host-side checks and grid arithmetic shared by the dispatchers of conv_wide.hip and wide_stream.hip.
#pragma once
#include "dm_common.h"
#include <initializer_list>

// one coefficient row set per sample (per-sample BatchNorm): the streaming and one-pass kernels stage a single shared set
static inline bool per_sample_coef(const Operand &op) { return op.mode >= DM_LOAD_AFFINE && op.coef_bstride; }

// what no streaming convolution takes: per-tile statistics, a ones channel, the border-bias table, per-sample coefficients
static inline bool stream_operand_ok(const Operand &in, const Epilogue &ep, int Cphys, int CIN, int per_tile)
{
    return !(per_tile || Cphys != CIN || in.ones || ep.bias_border || per_sample_coef(in));
}

// the gate of a streaming convolution: no mask, or the mask tensor read as it is or through one shared affine row set
static inline bool stream_mask_ok(const Epilogue &ep)
{
    return !(ep.mask.p0 && (ep.mask.mode == DM_LOAD_RELU || ep.mask.mode > DM_LOAD_AFFINE || ep.mask.coef_bstride || ep.mask.ones));
}

// Persistent grid: one workgroup per `per_wg` units up to `cap`; where every workgroup writes a slab of its own (`slabbed`),
// no more workgroups than the caller's `nslabs`; at least one.
static inline int persistent_grid(long long units, int per_wg, int cap, bool slabbed, int nslabs)
{
    int grid = (int)(units / per_wg < cap ? (units + per_wg - 1) / per_wg : cap);
    if (slabbed && grid > nslabs) grid = nslabs;
    return grid < 1 ? 1 : grid;
}

// What a dispatcher decided for a persistent kernel (dm_launch_plan, include/dynamorph_hip.h): filled by the *_plan function of
// a launcher, which is where "does it take the call, and with what grid" lives; the launcher launches p.workgroups and the
// host-only queries (dm_conv4x4s2_plan ...) hand the same struct out.
static inline dm_launch_plan persistent_plan(int kernel, int workgroups, int waves, int walkers, int dealing, long long units, int ring = 0)
{
    dm_launch_plan p{};
    p.kernel = kernel; p.workgroups = workgroups; p.waves = waves; p.walkers = walkers; p.dealing = dealing; p.ring = ring;
    p.units = units;
    return p;
}
// a kernel family that is not a persistent stream: only the kernel value is set
static inline dm_launch_plan family_plan(int kernel) { return persistent_plan(kernel, 0, 0, 0, DM_DEAL_NONE, 0); }

// Dynamic LDS beyond 64 KB has to be granted per kernel (per launch: the attribute belongs to the current device's copy of it).
static inline bool reserve_dynamic_lds(std::initializer_list<const void *> kernels, int bytes)
{
    for (const void *k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    return true;
}
