/*
 * rt_paths_body.h -- what rt_paths.hip (include/rt_paths.h) and rt_paths_compact.hip (include/rt_paths_compact.h) share, one copy
 * of each: THE DEFINITION's arithmetic of a step -- the light's mask and the accumulation (rt_paths_accumulate), the throughput's
 * multiplication and the decision whether a path goes on (rt_paths_decide), the next ray with its hash (rt_paths_next_ray) -- the
 * resolve (rt_paths_resolve), and the argument checks.  What differs between the two units is WHERE a lane reads and writes,
 * never what it computes: rt_paths.hip in place, path = slot on every bounce; rt_paths_compact.hip a dense list of the paths still
 * alive whose survivors go to the next list.  The functions are inlined into each unit's own kernels.  rt_paths.hip takes the
 * resolve, the checks and the chunk rule from here, and its resolve kernel kept its machine code; ITS STEP KERNEL KEEPS ITS OWN
 * TEXT of the step's arithmetic, because calling these functions from it changed the instructions of two of its four
 * instantiations (DESIGN.md section 35 has the tables, as section 31 has for the glass step) -- a change to the arithmetic below
 * is a change to rt_paths_step_kernel as well, and tests/test_paths_compact_gpu.py compares the two units word for word.  Both
 * units compile this file under `#pragma clang fp contract(off)` and the library's arithmetic flags.  (As rt_mirror_body.h is
 * for rt_mirror.hip and rt_mirror_compact.hip.)
 */
#ifndef RT_PATHS_BODY_H_
#define RT_PATHS_BODY_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/rt_paths.h"
#include "rt_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPathsBlock = 256;                       /* step: paths a workgroup; resolve: lanes a workgroup */
constexpr int kPathsResolveSamples = 1024;             /* resolve: paths a workgroup -- 1024 / S records */
constexpr int kPathsMaxSamples = RT_INDIRECT_MAX_SAMPLES;   /* n */
constexpr int kPathsMaxBounces = RT_PATHS_MAX_BOUNCES;      /* B */
constexpr long long kPathsMaxBatchRays = 0x7fffffffLL - 64; /* rt_trace_rays' grid limit for a flat list (include/rt_capi_rays.h) */
constexpr int kPathsMaxRecords = 533333333;            /* rt_render_gbuffer's record limit */
constexpr int kPathsHitWords = 12, kPathsHitFlagsWord = 11; /* an rt_hit in 4-byte words; its flags (byte 44) */
constexpr uint32_t kPathsGolden = 0x9e3779b9u;
/* alive[b] is kept as kPathsCountSlots partial counts, one 128-byte line each: a wavefront adds to the slot of its number.  One
 * counter a bounce serialised a million same-address atomics a step at 4096 x 4096, n = 2 -- 12.8 ms a step against 0.5 ms for a
 * copy of the step's bytes (profiles/paths_experiments.txt) */
constexpr uint32_t kPathsCountSlots = 128, kPathsCountStride = 16;   /* slots a bounce; 64-bit words from slot to slot */

/* resolve: a record's 3 S floats in LDS, padded to an odd stride so that the sums' reads spread over the banks */
constexpr int rt_paths_lds_stride(int S) { return (3 * S) | 1; }
constexpr int rt_paths_lds_floats() {
    int most = 0;
    for (int n = 1; n <= kPathsMaxSamples; ++n)
        most = std::max(most, (kPathsResolveSamples / (n * n)) * rt_paths_lds_stride(n * n));
    return most;
}
static_assert(rt_paths_lds_floats() * 4 <= 16384, "resolve: LDS");

} // namespace

/* the 32-bit integer hash "lowbias32" (include/rt_capi_soft.h) */
__device__ __forceinline__ uint32_t rt_paths_hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

/* Whether the record of a path (in place: a slot's; compact: an entry's) is live at bounce 0: hits is the chunk's first record,
 * p the path's record of the chunk */
__device__ __forceinline__ bool rt_paths_record_live(const int32_t *__restrict__ hits, uint32_t p) {
    const int32_t *h = hits + (size_t)p * kPathsHitWords;
    return h[0] >= 0 && (h[kPathsHitFlagsWord] & RT_HIT_LIGHT) == 0;
}

/* the header's mask and accumulation at one bounce: (cx, cy, cz) the colour the ray brought, flags its record's (0 where none was
 * asked for: the last bounce with emitters == 1), T the path's throughput T_b, a its sum.  FIRST: acc = colour_0. */
template <bool FIRST>
__device__ __forceinline__ void rt_paths_accumulate(float cx, float cy, float cz, int32_t flags, int emitters, float Tx, float Ty,
                                                    float Tz, float *a) {
    const bool light = (flags & RT_HIT_LIGHT) != 0;
    if (!emitters && light) cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (FIRST) {
        a[0] = cx, a[1] = cy, a[2] = cz;
    } else {
        a[0] = a[0] + Tx * cx, a[1] = a[1] + Ty * cy, a[2] = a[2] + Tz * cz;
    }
}

/* DOES THIS PATH GO ON after bounce b, as ONE function of its record's object, flags and colour (gx, gy, gz), its object's kd and
 * its throughput: T is T_b and the decision's T is T_{b+1}, w.c = (g.color.c * kd) * gain and T_{b+1}.c = T_b.c * w.c, operation
 * for operation; the path ends on a miss (object < 0), on a light, or where all three channels of T_{b+1} compare equal to 0.
 * It reads kd[object] where the object is one of the scene's and nothing else.  rt_paths_compact.hip's count kernel and its step
 * both decide by this function of the same words, so the ranks the step derives are those the count counted. */
struct RtPathsDecision {
    bool goes_on;
    float Tx, Ty, Tz;                                  /* T_{b+1} */
};

__device__ __forceinline__ RtPathsDecision rt_paths_decide(int32_t object, int32_t flags, float gx, float gy, float gz,
                                                           const float *__restrict__ kd, int n_objects, float gain, float Tx,
                                                           float Ty, float Tz) {
    const bool light = (flags & RT_HIT_LIGHT) != 0;
    const float k = object >= 0 && object < n_objects ? kd[object] : 0.0f;
    Tx = Tx * ((gx * k) * gain), Ty = Ty * ((gy * k) * gain), Tz = Tz * ((gz * k) * gain);
    if (object < 0 || light || (Tx == 0.0f && Ty == 0.0f && Tz == 0.0f)) return {false, Tx, Ty, Tz};
    return {true, Tx, Ty, Tz};
}

/* ray_{b+1} of the path whose bounce-b record is q0, q1 and flags (rt_hit's first eight words and its last) to o[0..5]:
 * rt_indirect_rays' single ray of that record with the hash H(H(seed ^ golden) ^ (key + r)), seed the NEXT bounce's, key the chunk's
 * first path's key and r the path's SLOT in the chunk (never its place in a list): key + r is the path's key kq.  The record's frame is rt_indirect_raygen_kernel's arithmetic (ao_tile()'s, rt_kernel.hip), operation for
 * operation; the one sample of n = 1: s = 0, i = j = 0, step = 2 / 1. */
__device__ __forceinline__ void rt_paths_next_ray(float4 q0, float4 q1, int32_t flags, uint32_t seed, uint32_t key, uint32_t r, float *o) {
    const float Px = q0.z, Py = q0.w, Pz = q1.x;
    const bool flip = (flags & RT_HIT_INSIDE) != 0;
    const float Nx = flip ? -q1.y : q1.y, Ny = flip ? -q1.z : q1.z, Nz = flip ? -q1.w : q1.w;
    const bool ax = fabsf(Nx) < 0.5f;
    const float Ax = ax ? 1.0f : 0.0f, Ay = ax ? 0.0f : 1.0f, Az = 0.0f;
    const float ux = Ay * Nz - Az * Ny, uy = Az * Nx - Ax * Nz, uz = Ax * Ny - Ay * Nx;
    const float len = sqrtf(ux * ux + uy * uy + uz * uz);
    const float Ux = ux / len, Uy = uy / len, Uz = uz / len;
    const float Vx = Ny * Uz - Nz * Uy, Vy = Nz * Ux - Nx * Uz, Vz = Nx * Uy - Ny * Ux;
    const uint32_t hs = rt_paths_hash(rt_paths_hash(rt_paths_hash(seed ^ kPathsGolden) ^ (key + r)) ^ 0u);
    const float xi1 = (float)(hs >> 8) * 0x1p-24f;
    const float xi2 = (float)(rt_paths_hash(hs ^ kPathsGolden) >> 8) * 0x1p-24f;
    const float step = 2.0f / 1.0f;
    const float pa = (0.0f + xi1) * step - 1.0f, pb = (0.0f + xi2) * step - 1.0f;
    const float dx = pa * sqrtf(1.0f - (pb * pb) * 0.5f), dy = pb * sqrtf(1.0f - (pa * pa) * 0.5f);
    const float w = (1.0f - dx * dx) - dy * dy;
    const float dz = w > 0.0f ? sqrtf(w) : 0.0f;
    const float Dx = (Ux * dx + Vx * dy) + Nx * dz, Dy = (Uy * dx + Vy * dy) + Ny * dz, Dz = (Uz * dx + Vz * dy) + Nz * dz;
    o[0] = Px, o[1] = Py, o[2] = Pz;
    o[3] = Px + Dx, o[4] = Py + Dy, o[5] = Pz + Dz;
}

/* out[3 p + c] = base[3 p + c] + term.c of the header for the m records of a chunk: path s of record p has its sum at
 * acc[3 (p S + s) ..].  rt_indirect_resolve_kernel's text without the gather records (the steps have masked already): a workgroup
 * of kPathsBlock lanes takes kPathsResolveSamples / S records, reads their paths' floats as the consecutive words they are into
 * lds (rt_paths_lds_floats() floats, rt_paths_lds_stride(S) a record), then one lane per record and channel sums its S values in
 * order, divides, multiplies by the weight, adds the base and stores.  A word of the output is read (base) and stored by the same
 * lane, once: out == base is allowed.  Each unit has a kernel of its own around this body. */
__device__ __forceinline__ void rt_paths_resolve(float *lds, uint32_t m, int S, float gain, const float *__restrict__ acc,
                                                 const int32_t *__restrict__ hits, const float *__restrict__ kd, int n_objects,
                                                 const float *base, float *out) {
    const uint32_t group = (uint32_t)kPathsResolveSamples / (uint32_t)S;
    const uint32_t g0 = blockIdx.x * group;
    const uint32_t records = min(group, m - g0);                         /* (g0 < m: the grid is ceil(m / group)) */
    const uint32_t per = 3u * (uint32_t)S, stride = (uint32_t)rt_paths_lds_stride(S), words = records * per;
    const float *src = acc + (size_t)per * (size_t)g0;
    for (uint32_t i = threadIdx.x; i < words; i += (uint32_t)kPathsBlock) {
        const uint32_t px = i / per;
        lds[px * stride + (i - px * per)] = src[i];
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < 3u * records; t += (uint32_t)kPathsBlock) {
        const uint32_t px = t / 3u, c = t - 3u * px;
        const float *v = lds + px * stride + c;
        float sum = v[0];
        for (int s = 1; s < S; ++s) sum = sum + v[3 * s];
        const float mean = sum / (float)S;
        const int32_t *h = hits + (size_t)(g0 + px) * kPathsHitWords;
        const int32_t object = h[0];
        float term = 0.0f;
        if (object >= 0 && (h[kPathsHitFlagsWord] & RT_HIT_LIGHT) == 0) {
            const float k = object < n_objects ? kd[object] : 0.0f;
            term = ((__int_as_float(h[8 + c]) * k) * gain) * mean;
        }
        const size_t at = 3 * (size_t)(g0 + px) + c;
        out[at] = base ? base[at] + term : term;
    }
}

/* ---- THE HOST SIDE: the argument checks of both units (fail() is rt_host.h's) ---- */

namespace {

/* rt_paths.h's checks (1) .. (12) in its order (device: the device variant's alignments as well), which rt_paths_compact.h takes
 * over word for word */
inline int rt_paths_check_args(const rt_scene *s, const rt_paths_params *pr, int n, const void *hits, const void *base,
                               const void *out, bool device) {
    if (!s) return fail(RT_ERR_INVALID, "scene is NULL");
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->samples < 1 || pr->samples > kPathsMaxSamples)
        return fail(RT_ERR_INVALID, "samples must be 1.." + std::to_string(kPathsMaxSamples) + " (got " + std::to_string(pr->samples) + ")");
    if (pr->bounces < 1 || pr->bounces > kPathsMaxBounces)
        return fail(RT_ERR_INVALID, "bounces must be 1.." + std::to_string(kPathsMaxBounces) + " (got " + std::to_string(pr->bounces) + ")");
    if (pr->gather_depth < 0) return fail(RT_ERR_INVALID, "gather_depth must not be negative");
    if (pr->chunk_records < 0) return fail(RT_ERR_INVALID, "chunk_records must not be negative");
    if (pr->emitters != 0 && pr->emitters != 1)
        return fail(RT_ERR_INVALID, "emitters must be 0 or 1 (got " + std::to_string(pr->emitters) + ")");
    if (!std::isfinite(pr->gain)) return fail(RT_ERR_INVALID, "gain must be finite");
    if (n < 0) return fail(RT_ERR_INVALID, "n < 0");
    if (n > 0 && !hits) return fail(RT_ERR_INVALID, "hits pointer is NULL");
    if (n > 0 && !out) return fail(RT_ERR_INVALID, "output pointer is NULL");
    if (n > kPathsMaxRecords) return fail(RT_ERR_INVALID, "more than " + std::to_string(kPathsMaxRecords) + " records");
    if (device && ((uintptr_t)hits & 15u) != 0) return fail(RT_ERR_INVALID, "d_hits must be 16-byte aligned");
    if (device && ((uintptr_t)out & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_rgb must be 4-byte aligned");
    if (device && base && ((uintptr_t)base & 3u) != 0) return fail(RT_ERR_INVALID, "d_base_rgb must be 4-byte aligned");
    if (rt_internal_scene_soft(s))
        return fail(RT_ERR_INVALID, "the indirect paths refuse a scene with area lights: a ray batch keys their shadow samples by "
                                    "the ray index (include/rt_capi_soft.h), so the result would change with chunk_records");
    return RT_OK;
}

/* the records a launch gathers for: the caller's chunk_records, or the default -- as many as keep a chunk's scratch of path_bytes
 * a path within chunk_bytes, at least one -- never more than kPathsMaxBatchRays rays' worth, nor than the batch has */
inline int rt_paths_chunk_records(const rt_paths_params &pr, int n, size_t path_bytes, size_t chunk_bytes) {
    const long long S = (long long)pr.samples * pr.samples;                          /* paths a record; <= 64 */
    long long c = pr.chunk_records > 0 ? pr.chunk_records : std::max<long long>(1, (long long)(chunk_bytes / (path_bytes * (size_t)S)));
    c = std::min(c, kPathsMaxBatchRays / S);
    return (int)std::min<long long>(c, n);
}

} // namespace

#endif /* RT_PATHS_BODY_H_ */
