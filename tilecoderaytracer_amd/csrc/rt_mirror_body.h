/*
 * rt_mirror_body.h -- what rt_mirror.hip (include/rt_mirror.h) and rt_mirror_compact.hip (include/rt_mirror_compact.h) share, one
 * copy of each: the step of a mirror chain -- THE DEFINITION's arithmetic -- as a kernel template both units instantiate, the
 * rule that decides `mirror`, and the argument checks.  What differs between the two units is WHERE a lane
 * reads and writes, never what it computes: in place, entry = ray = place; compact, a dense list of the rays still alive whose
 * survivors go to the next list.  Both units compile this file under `#pragma clang fp contract(off)` and the library's
 * arithmetic flags.  (As rt_accumulate_body.h is for rt_temporal.hip and rt_motion.hip.)
 * rt_glass.hip (include/rt_glass.h) shares the argument checks and, through rt_glass_body.h, the __device__ helpers; its step is a
 * kernel of its own there, and the kernel below is as it was before that unit existed (DESIGN.md section 29 says why).
 */
#ifndef RT_MIRROR_BODY_H_
#define RT_MIRROR_BODY_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/rt_glass.h"
#include "../../include/rt_mirror.h"
#include "rt_host.h"
#include "rt_scan.h"

#pragma clang fp contract(off)

/* the 32-bit integer hash "lowbias32" (include/rt_capi_ao.h) */
__device__ __forceinline__ uint32_t rt_mirror_hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float rt_mirror_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

/* normalize(T - E) of the ray at r[0..5], createEyeRay's arithmetic */
__device__ __forceinline__ void rt_mirror_direction(const float *r, float *dx, float *dy, float *dz) {
    const float x = r[3] - r[0], y = r[4] - r[1], z = r[5] - r[2];
    const float len = sqrtf((x * x + y * y) + z * z);
    *dx = x / len, *dy = y / len, *dz = z / len;
}

/* the header's `mirror` of a record with this object and these flags, and *refl = rf[object] (0 where there is none) */
__device__ __forceinline__ bool rt_mirror_followed(int32_t object, int32_t flags, const float *__restrict__ rf, int n_objects,
                                                   float min_reflective, float *refl) {
    *refl = (object >= 0 && object < n_objects) ? rf[object] : 0.0f;
    return object >= 0 && object < n_objects && (flags & RT_HIT_LIGHT) == 0 && *refl >= min_reflective;
}

constexpr int kMirrorBlock = 256;                      /* entries a workgroup (kRankBlock: the workgroup ranks its flags) */
static_assert(kMirrorBlock == kRankBlock, "rt_scan_rank's workgroup");
constexpr int kMirrorLdsStride = 13;                   /* STAGE: a record's 12 words in LDS, odd stride */
constexpr uint32_t kMirrorDone = 1u << 9;              /* in place: the state word is out_path's (k | cut << 8 | tag << 12) and this */

/* Bounce s of the m entries of a chunk's list, one lane an entry (i < m < 2^31).
 * IN PLACE (COMPACT false, rt_mirror.hip): the list is the chunk, entry i is ray i on every bounce.  records[3 i ..] is the
 * record of ray_s, rays_k[6 i ..] is ray_s itself (FIRST: the caller's rays; later the chunk's scratch, which rays_next then is
 * as well: a lane reads its own ray before it writes it), rays0 the caller's rays, state the chunk's planes of `stride` words
 * (14 of them with GUIDE -- the word, w, L, A -- else 4).  A ray whose chain ends before the last bounce is retired where it
 * stands: six +0.0f as its next ray and kMirrorDone as its word.  The five last arguments are not read.
 * COMPACT (rt_mirror_compact.hip): the list holds the rays still alive, in ray order.  Entry i's ray of the chunk is idx_k[i]
 * (FIRST: i), its state is read from state_k and never from `state`; a chain that ends writes its outputs and nothing else; one
 * that goes on writes its next ray, state and index to place p of rays_next, state and idx_next -- the OTHER list, never the one
 * being read -- where p = group_base[b / kScanBlock] + offsets[b] + the lane's rank among workgroup b's chains that go on
 * (rt_scan.h; the counts scanned are rt_mirror_compact_count_kernel's, which decides by the same function of the same two words).  With
 * `last` nothing goes on and neither array is read.  p < the scan's total <= m <= stride.
 * FIRST: s == 0, the starting state is the header's and no state is read.  last: s == max_bounces, every chain still alive ends
 * here.  GUIDE: out_guide is given, so L and A are carried.  STAGE: the workgroup's records are read as the consecutive words
 * they are through LDS (in place only).  Every address is the entry's, its ray's or its place's own (STAGE: or one of the
 * workgroup's records, below records[3 m]): nothing is read or written past them.
 * COMPACT false compiles to what rt_mirror.hip's kernel was before it moved here: the COMPACT branches are resolved at compile
 * time, and the registers are the same (profiles/mirror_compact_experiments.txt). */
template <bool FIRST, bool GUIDE, bool STAGE, bool COMPACT>
__global__ __launch_bounds__(kMirrorBlock) void rt_mirror_step_kernel(uint32_t m, uint32_t stride, int last, float min_reflective,
                                                                      const float *__restrict__ rf, int n_objects,
                                                                      const float4 *__restrict__ records, const float *rays_k,
                                                                      const float *__restrict__ rays0, float *rays_next, uint32_t *state,
                                                                      float4 *__restrict__ out_hits, float4 *__restrict__ out_guide,
                                                                      float *__restrict__ out_weight, uint32_t *__restrict__ out_path,
                                                                      const uint32_t *state_k, const uint32_t *idx_k, uint32_t *idx_next,
                                                                      const uint32_t *offsets, const uint32_t *group_base) {
    const uint32_t i = blockIdx.x * (uint32_t)kMirrorBlock + threadIdx.x;
    __shared__ float lds[STAGE ? kMirrorBlock * kMirrorLdsStride : 1];
    __shared__ uint32_t wave_count[COMPACT ? kMirrorBlock / 64 : 1];
    static_assert(!(STAGE && COMPACT), "the compact list reads its records with three 16-byte loads");
    if (STAGE) {
        const uint32_t base = blockIdx.x * (uint32_t)kMirrorBlock;           /* (base < m: the grid is ceil(m / kMirrorBlock)) */
        const uint32_t words = min((uint32_t)kMirrorBlock, m - base) * 12u;
        const float *src = reinterpret_cast<const float *>(records) + (size_t)base * 12;
        for (uint32_t t = threadIdx.x; t < words; t += (uint32_t)kMirrorBlock) {
            const uint32_t rec = t / 12u;
            lds[rec * kMirrorLdsStride + (t - rec * 12u)] = src[t];
        }
        __syncthreads();
    }
    uint32_t place = i;
    if (COMPACT && !last) {                                                   /* (uniform; every lane of the workgroup ranks) */
        bool live = false;
        if (i < m) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(records) + 12 * (size_t)i;
            float unused;
            live = rt_mirror_followed((int32_t)w[0], (int32_t)w[11], rf, n_objects, min_reflective, &unused);
        }
        uint32_t count;
        place = rt_scan_rank(live, wave_count, &count);
        place += group_base[blockIdx.x / (uint32_t)kScanBlock] + offsets[blockIdx.x];
    }
    if (i >= m) return;
    const uint32_t *state_in = COMPACT ? state_k : state;
    const uint32_t word = FIRST ? 0u : state_in[i];
    if (word & kMirrorDone) return;
    const uint32_t p = COMPACT ? place : i;                                   /* the entry written */
    const uint32_t ray = (COMPACT && !FIRST) ? idx_k[i] : i;                  /* the entry's ray of the chunk */
    float4 q0, q1, q2;
    if (STAGE) {
        const float *q = lds + threadIdx.x * kMirrorLdsStride;
        q0 = make_float4(q[0], q[1], q[2], q[3]), q1 = make_float4(q[4], q[5], q[6], q[7]), q2 = make_float4(q[8], q[9], q[10], q[11]);
    } else {
        q0 = records[3 * (size_t)i], q1 = records[3 * (size_t)i + 1], q2 = records[3 * (size_t)i + 2];
    }
    const int32_t object = __float_as_int(q0.x), flags = __float_as_int(q2.w);
    const uint32_t k = word & 0xffu, tag = word >> 12;
    float wx = 1.0f, wy = 1.0f, wz = 1.0f, L = 0.0f;
    float A[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (!FIRST) {
        wx = __uint_as_float(state_in[(size_t)stride + i]);
        wy = __uint_as_float(state_in[2 * (size_t)stride + i]);
        wz = __uint_as_float(state_in[3 * (size_t)stride + i]);
        if (GUIDE) {
            L = __uint_as_float(state_in[4 * (size_t)stride + i]);
#pragma unroll
            for (int c = 0; c < 9; ++c) A[c] = __uint_as_float(state_in[(size_t)(5 + c) * stride + i]);
        }
    }
    if (GUIDE && object >= 0) L = L + q0.y;
    const float refl = (object >= 0 && object < n_objects) ? rf[object] : 0.0f;
    const bool mirror = object >= 0 && object < n_objects && (flags & RT_HIT_LIGHT) == 0 && refl >= min_reflective;
    const float Px = q0.z, Py = q0.w, Pz = q1.x, nx = q1.y, ny = q1.z, nz = q1.w;

    if (!mirror || last) {                                                    /* the terminal record */
        out_hits[3 * (size_t)ray] = q0, out_hits[3 * (size_t)ray + 1] = q1, out_hits[3 * (size_t)ray + 2] = q2;
        if (out_weight) {
            float *o = out_weight + 3 * (size_t)ray;
            o[0] = wx, o[1] = wy, o[2] = wz;
        }
        if (out_path) out_path[ray] = k | (mirror ? 1u << 8 : 0u) | tag << 12;
        if (GUIDE) {
            float4 g0 = q0, g1 = q1;
            if (!FIRST && object >= 0 && k != 0u) {
                const float *e = rays0 + 6 * (size_t)ray;
                float dx, dy, dz;
                rt_mirror_direction(e, &dx, &dy, &dz);
                g0.x = __int_as_float((int32_t)(tag << 12 | (uint32_t)object));
                g0.y = L;
                g0.z = e[0] + dx * L, g0.w = e[1] + dy * L, g1.x = e[2] + dz * L;
                g1.y = rt_mirror_dot(A[0], A[1], A[2], nx, ny, nz);
                g1.z = rt_mirror_dot(A[3], A[4], A[5], nx, ny, nz);
                g1.w = rt_mirror_dot(A[6], A[7], A[8], nx, ny, nz);
            }
            out_guide[3 * (size_t)ray] = g0, out_guide[3 * (size_t)ray + 1] = g1, out_guide[3 * (size_t)ray + 2] = q2;
        }
        if (!COMPACT && !last) {                                              /* retired: a degenerate ray from here on */
            float *o = rays_next + 6 * (size_t)p;
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = 0.0f;
            state[p] = kMirrorDone;
        }
        return;
    }

    float dx, dy, dz;
    rt_mirror_direction(rays_k + 6 * (size_t)i, &dx, &dy, &dz);
    const float c = rt_mirror_dot(nx, ny, nz, dx, dy, dz);
    const float rx = ((-2.0f * nx) * c) + dx, ry = ((-2.0f * ny) * c) + dy, rz = ((-2.0f * nz) * c) + dz;
    float *o = rays_next + 6 * (size_t)p;
    o[0] = Px, o[1] = Py, o[2] = Pz;
    o[3] = Px + rx, o[4] = Py + ry, o[5] = Pz + rz;
    state[p] = (k + 1u) | (1u + rt_mirror_hash(tag << 12 | (uint32_t)object) % 0x7fffeu) << 12;
    state[(size_t)stride + p] = __float_as_uint(wx * (refl * q2.x));
    state[2 * (size_t)stride + p] = __float_as_uint(wy * (refl * q2.y));
    state[3 * (size_t)stride + p] = __float_as_uint(wz * (refl * q2.z));
    if (GUIDE) {
        state[4 * (size_t)stride + p] = __float_as_uint(L);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float an = rt_mirror_dot(A[3 * r], A[3 * r + 1], A[3 * r + 2], nx, ny, nz);
            const float two = 2.0f * an;
            state[(size_t)(5 + 3 * r) * stride + p] = __float_as_uint(A[3 * r] - two * nx);
            state[(size_t)(6 + 3 * r) * stride + p] = __float_as_uint(A[3 * r + 1] - two * ny);
            state[(size_t)(7 + 3 * r) * stride + p] = __float_as_uint(A[3 * r + 2] - two * nz);
        }
    }
    if (COMPACT) idx_next[p] = ray;
}

/* ---- THE HOST SIDE: the argument checks of both units (fail() is rt_host.h's, which a unit includes before this file) ---- */

namespace {

constexpr double kMaxRayFloats = 2.0e9 * 4.0;          /* rt_render's limit for one output, in floats */
constexpr long long kMaxCells = 0x7fffffffLL - 64;     /* rt_trace_rays' grid limit (include/rt_capi_rays.h) */

inline bool rt_mirror_transmissive_nan(const rt_mirror_params &) { return false; }
inline bool rt_mirror_transmissive_nan(const rt_glass_params &pr) { return std::isnan(pr.min_transmissive); }

/* rt_mirror.h's checks (1) .. (10), which rt_mirror_compact.h takes over word for word and rt_glass.h (Params = rt_glass_params)
 * with one check more */
template <class Params>
inline int rt_mirror_check_args(const rt_scene *s, const Params *pr, int n, int rows, const void *rays, const void *out_hits,
               const void *out_guide, const void *out_weight, const void *out_path, bool device) {
    if (!s) return fail(RT_ERR_INVALID, "scene is NULL");
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->max_bounces < 0 || pr->max_bounces > RT_MIRROR_MAX_BOUNCES)
        return fail(RT_ERR_INVALID, "max_bounces must be 0.." + std::to_string(RT_MIRROR_MAX_BOUNCES) + " (got " +
                                        std::to_string(pr->max_bounces) + ")");
    if (pr->chunk_rays < 0) return fail(RT_ERR_INVALID, "chunk_rays must not be negative");
    if (std::isnan(pr->min_reflective)) return fail(RT_ERR_INVALID, "min_reflective must not be NaN");
    if (rt_mirror_transmissive_nan(*pr)) return fail(RT_ERR_INVALID, "min_transmissive must not be NaN");
    if (n < 0) return fail(RT_ERR_INVALID, "n < 0");
    if (rows < 1) return fail(RT_ERR_INVALID, "rows must be positive");
    if (n > 0 && !rays) return fail(RT_ERR_INVALID, "rays pointer is NULL");
    if (n > 0 && !out_hits) return fail(RT_ERR_INVALID, "out_hits pointer is NULL");
    /* rt_trace_rays' limit (rays_args() of rt_capi.hip): the batch's floats, and the cells of its grid of rows */
    const int r = std::min(rows, std::max(n, 1));
    if ((double)n * 3.0 > kMaxRayFloats || (((long long)n + r - 1) / r) * r > kMaxCells)
        return fail(RT_ERR_INVALID, "ray batch too large for its rows");
    if (!device) return RT_OK;
    if (((uintptr_t)rays & 3u) != 0) return fail(RT_ERR_INVALID, "d_rays must be 4-byte aligned");
    if (((uintptr_t)out_hits & 15u) != 0) return fail(RT_ERR_INVALID, "d_out_hits must be 16-byte aligned");
    if (((uintptr_t)out_guide & 15u) != 0) return fail(RT_ERR_INVALID, "d_out_guide must be 16-byte aligned");
    if (((uintptr_t)out_weight & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_weight must be 4-byte aligned");
    if (((uintptr_t)out_path & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_path must be 4-byte aligned");
    return RT_OK;
}

} // namespace

#endif /* RT_MIRROR_BODY_H_ */
