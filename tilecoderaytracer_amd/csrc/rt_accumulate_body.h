/*
 * rt_accumulate_body.h -- the one copy of the per-pixel definition of include/rt_temporal.h and include/rt_motion.h, and of the
 * host code the two units share: the argument checks in the headers' order, the kernel's arguments computed from the cameras, the
 * device variant's alignment and overlap rules.  rt_temporal.hip instantiates the kernel without a motion table (kNoTable) and
 * compiles to the instructions it compiled to when the kernel stood in that file (profiles/motion_experiments.txt, RESOURCES);
 * rt_motion.hip instantiates it with the table read from global memory (kTableGlobal) or staged in LDS (kTableLds).  The table is
 * a parameter pack behind Args and not an argument of a body function called by two kernels: a kernel that hands its Args to a
 * function, by reference or by value, addresses them through a second base register pair and needs 106 scalar registers where
 * this one needs 104.  Everything here has internal linkage but rt_temporal_args, which the kernels' names carry, and the kernel.
 */
#ifndef RT_ACCUMULATE_BODY_H_
#define RT_ACCUMULATE_BODY_H_

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rt_temporal.h"
#include "rt_host.h"

static_assert(sizeof(rt_hit) == 48, "rt_hit layout");
static_assert(sizeof(rt_temporal_params) == 28, "rt_temporal_params layout");
static_assert(sizeof(rt_camera_desc) == 64, "rt_camera_desc layout");

namespace {

constexpr int kTileZ = 64, kTileX = 4;                 /* a workgroup: 4 wavefronts, each 64 consecutive z of one column */
constexpr uint64_t kMaxGroups = 1ull << 20;            /* workgroups of a launch; they stride over the tiles */
constexpr double kMaxPixels = 2.0e9 * 4.0 * 4.0 / 60.0; /* rt_render_gbuffer's limit: 3.2e10 bytes of colours and records */

/* how a lane gets its object's motion (include/rt_motion.h): not at all, three 16-byte loads from global memory, or from a copy
 * of the table each workgroup stages in LDS before its loop over the tiles */
constexpr int kNoTable = 0, kTableGlobal = 1, kTableLds = 2;
/* the largest table staged in LDS: 170 * 48 = 8160 bytes beside the 12 KiB of record staging is 20 448 bytes a workgroup, so
 * that the 160 KiB of a CU still hold 8 workgroups -- one wavefront of each per SIMD, the most the registers ever allow */
constexpr int kLdsMotions = 170;

struct V3 {
    float x, y, z;
};

} // namespace

struct rt_temporal_args {    /* the kernel's arguments beside its buffers */
    int W, H, x0, Wn;
    int match_color, plane, identity;
    float normal_cos, eps2, alpha, alpha_moments, max_history;
    float eye[3], nh[3], na[3], nb[3], q;              /* the previous camera's, header step 3 */
    float halfwidth, width, halfheight, height, fW, fH;
    uint32_t tiles_z;
    uint64_t tiles;
};
using Args = rt_temporal_args;

/* a record's three 16-byte words: {object, distance, point.xy}, {point.z, normal.xyz}, {color.rgb, flags} */
struct Rec {
    uint4 a, b, c;
};

__device__ __forceinline__ Rec load_rec(const uint4 *__restrict__ hits, int64_t index) {
    const uint4 *r = hits + 3 * index;                  /* (64-bit: 48 index passes 2^32 in a large frame) */
    return Rec{r[0], r[1], r[2]};
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

/* what a kernel with a table has behind its Args: the table and its length; a kernel without one has nothing there */
__device__ __forceinline__ const uint4 *table_of() { return nullptr; }
__device__ __forceinline__ const uint4 *table_of(const uint4 *motions, int) { return motions; }
__device__ __forceinline__ int entries_of() { return 0; }
__device__ __forceinline__ int entries_of(const uint4 *, int n_motions) { return n_motions; }

/* the headers' definition, one lane a pixel.  kC: channels; kFirst: no previous frame (its pointers are NULL); kStage: the
 * wavefront's current records come through LDS (a lane without a pixel stays for the barriers); kTable: where the motion of a
 * record's object comes from, and Table: nothing for kNoTable, else (const uint4 *motions, int n_motions), n_motions entries of
 * three 16-byte words, the rows of the 3 x 4 matrix.  prev_* and motions are never written and never alias an output. */
template <int kC, bool kFirst, bool kStage, int kTable, class... Table>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_temporal_kernel(
    const float *cur, const uint4 *__restrict__ cur_hits, const uint4 *__restrict__ prev_hits,
    const float *__restrict__ prev_value, const float *__restrict__ prev_moments, const float *__restrict__ prev_len,
    float *out_value, float *__restrict__ out_moments, float *__restrict__ out_len, float *__restrict__ out_variance,
    uint8_t *__restrict__ out_flags, Args A, Table... the_table) {
    static_assert(sizeof...(Table) == (kTable == kNoTable ? 0 : 2), "a kernel with a table takes (motions, n_motions)");
    const uint4 *const motions = table_of(the_table...);
    const int n_motions = entries_of(the_table...);
    (void)motions, (void)n_motions;
    __shared__ uint4 stage[kStage ? kTileX : 1][kStage ? 3 * kTileZ : 1];
    __shared__ uint4 table[kTable == kTableLds ? 3 * kLdsMotions : 1];
    if constexpr (kTable == kTableLds) {                    /* (n_motions <= kLdsMotions: the host chose this kernel) */
        for (int k = (int)(threadIdx.y * kTileZ + threadIdx.x); k < 3 * n_motions; k += kTileZ * kTileX) table[k] = motions[k];
        __syncthreads();
    }
    for (uint64_t tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const uint64_t tz = tile % A.tiles_z, tx = tile / A.tiles_z;
        const int64_t xl = (int64_t)tx * kTileX + threadIdx.y, z64 = (int64_t)tz * kTileZ + threadIdx.x;
        const bool mine = xl < A.Wn && z64 < A.H;
        Rec h;
        if (kStage) {
            /* rows [z0, z0 + n) of column xl: 3 n consecutive 16-byte words */
            const int64_t z0 = (int64_t)tz * kTileZ;
            const int n = xl < A.Wn ? (int)(A.H - z0 < kTileZ ? A.H - z0 : kTileZ) : 0;
            const uint4 *src = cur_hits + 3 * (xl * A.H + z0);
            for (int k = (int)threadIdx.x; k < 3 * n; k += kTileZ) stage[threadIdx.y][k] = src[k];
            __syncthreads();
            if (mine) h = Rec{stage[threadIdx.y][3 * threadIdx.x], stage[threadIdx.y][3 * threadIdx.x + 1], stage[threadIdx.y][3 * threadIdx.x + 2]};
            __syncthreads();
        }
        if (!mine) continue;
        const int x = A.x0 + (int)xl, z = (int)z64;
        const int64_t p = xl * A.H + z;                     /* the strip's pixel */
        if (!kStage) h = load_rec(cur_hits, p);
        float c[kC];
#pragma unroll
        for (int k = 0; k < kC; ++k) c[k] = cur[p * kC + k];
        float l;
        if constexpr (kC == 3) l = (0.25f * c[0] + 0.5f * c[1]) + 0.25f * c[2];
        else l = c[0];
        const float ll = l * l;
        float acc[kC + 3], wsum = 0.0f;                     /* the channels, m1, m2, len */
#pragma unroll
        for (int k = 0; k < kC + 3; ++k) acc[k] = 0.0f;
        if constexpr (!kFirst) {
            const bool dead = (int32_t)h.a.x < 0 || (h.c.w & (uint32_t)RT_HIT_LIGHT) != 0u;
            /* where the point and its normal were in the previous frame: the record's own words unless its object moved */
            float ppx = __uint_as_float(h.a.z), ppy = __uint_as_float(h.a.w), ppz = __uint_as_float(h.b.x);
            float npx = __uint_as_float(h.b.y), npy = __uint_as_float(h.b.z), npz = __uint_as_float(h.b.w);
            bool identity = A.identity;
            if constexpr (kTable != kNoTable) {
                if (!dead && h.a.x < (uint32_t)n_motions) {
                    const uint4 *m = (kTable == kTableLds ? table : motions) + 3 * (size_t)h.a.x;
                    const uint4 r0 = m[0], r1 = m[1], r2 = m[2];
                    constexpr uint32_t one = 0x3F800000u;
                    const uint32_t differs = (r0.x ^ one) | r0.y | r0.z | r0.w | r1.x | (r1.y ^ one) | r1.z | r1.w | r2.x | r2.y |
                                             (r2.z ^ one) | r2.w;
                    if (differs) {                          /* moving: always reprojected, also under equal cameras */
                        const float Px = ppx, Py = ppy, Pz = ppz, Nx = npx, Ny = npy, Nz = npz;
                        ppx = dot3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), Px, Py, Pz) + __uint_as_float(r0.w);
                        ppy = dot3(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z), Px, Py, Pz) + __uint_as_float(r1.w);
                        ppz = dot3(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z), Px, Py, Pz) + __uint_as_float(r2.w);
                        npx = dot3(__uint_as_float(r0.x), __uint_as_float(r0.y), __uint_as_float(r0.z), Nx, Ny, Nz);
                        npy = dot3(__uint_as_float(r1.x), __uint_as_float(r1.y), __uint_as_float(r1.z), Nx, Ny, Nz);
                        npz = dot3(__uint_as_float(r2.x), __uint_as_float(r2.y), __uint_as_float(r2.z), Nx, Ny, Nz);
                        identity = false;
                    }
                }
            }
            int i0 = x, j0 = z;
            float fx = 0.0f, fz = 0.0f;
            bool seen = !dead;
            if (!identity) {
                const float Dx = ppx - A.eye[0], Dy = ppy - A.eye[1], Dz = ppz - A.eye[2];
                const float s = dot3(Dx, Dy, Dz, A.nh[0], A.nh[1], A.nh[2]);
                const float a = dot3(Dx, Dy, Dz, A.na[0], A.na[1], A.na[2]) / s;
                const float b = dot3(Dx, Dy, Dz, A.nb[0], A.nb[1], A.nb[2]) / s;
                const float px = ((a + A.halfwidth) / A.width) * A.fW;
                const float pz = ((b + A.halfheight) / A.height) * A.fH;
                seen = seen && s * A.q > 0.0f && px > -1.0f && px < A.fW && pz > -1.0f && pz < A.fH;
                if (seen) {                                 /* (px, pz in (-1, 533 333 333]: they fit an int) */
                    const float flx = floorf(px), flz = floorf(pz);
                    i0 = (int)flx, j0 = (int)flz;
                    fx = px - flx, fz = pz - flz;
                }
            }
            if (seen) {
#pragma unroll
                for (int a = 0; a < 2; ++a) {
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        const int64_t i = (int64_t)i0 + a, j = (int64_t)j0 + b;
                        float bw = 1.0f;
                        if (identity) {
                            if (a || b) continue;
                        } else {
                            bw = (a ? fx : 1.0f - fx) * (b ? fz : 1.0f - fz);
                        }
                        if (i < 0 || i >= A.W || j < 0 || j >= A.H || !(bw > 0.0f)) continue;
                        const int64_t cell = i * A.H + j;
                        const Rec g = load_rec(prev_hits, cell);
                        bool take = g.a.x == h.a.x && ((g.c.w ^ h.c.w) & 3u) == 0u;
                        if (A.match_color) take = take && g.c.x == h.c.x && g.c.y == h.c.y && g.c.z == h.c.z;
                        const float t = dot3(npx, npy, npz, __uint_as_float(g.b.y), __uint_as_float(g.b.z), __uint_as_float(g.b.w));
                        take = take && t >= A.normal_cos;
                        if (A.plane) {
                            const float ex = __uint_as_float(g.a.z) - ppx, ey = __uint_as_float(g.a.w) - ppy, ez = __uint_as_float(g.b.x) - ppz;
                            const float d = dot3(ex, ey, ez, npx, npy, npz);
                            take = take && d * d <= A.eps2;
                        }
                        if (take) {
#pragma unroll
                            for (int k = 0; k < kC; ++k) acc[k] = acc[k] + bw * prev_value[cell * kC + k];
                            acc[kC] = acc[kC] + bw * prev_moments[cell * 2];
                            acc[kC + 1] = acc[kC + 1] + bw * prev_moments[cell * 2 + 1];
                            acc[kC + 2] = acc[kC + 2] + bw * prev_len[cell];
                            wsum = wsum + bw;
                        }
                    }
                }
            }
        }
        float v[kC], m1 = l, m2 = ll, len = 1.0f, var = 0.0f;
#pragma unroll
        for (int k = 0; k < kC; ++k) v[k] = c[k];
        const bool history = wsum > 0.0f;
        if (history) {
            float N = acc[kC + 2] / wsum + 1.0f;
            if (!(N <= A.max_history)) N = A.max_history;
            float ac = 1.0f / N, am = ac;
            if (!(ac >= A.alpha)) ac = A.alpha;
            if (!(am >= A.alpha_moments)) am = A.alpha_moments;
#pragma unroll
            for (int k = 0; k < kC; ++k) {
                const float hc = acc[k] / wsum;
                v[k] = hc + ac * (c[k] - hc);
            }
            const float hm1 = acc[kC] / wsum, hm2 = acc[kC + 1] / wsum;
            m1 = hm1 + am * (l - hm1);
            m2 = hm2 + am * (ll - hm2);
            len = N;
            const float d = m2 - m1 * m1;
            var = d > 0.0f ? d : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < kC; ++k) out_value[p * kC + k] = v[k];
        out_moments[p * 2] = m1;
        out_moments[p * 2 + 1] = m2;
        out_len[p] = len;
        if (out_variance) out_variance[p] = var;
        if (out_flags) out_flags[p] = history ? 0 : 1;
    }
}

namespace {

inline V3 cross(const V3 &a, const V3 &b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

inline int check_params(const rt_temporal_params *pr, int W, int H, int x0, int x1) {
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->channels != 1 && pr->channels != 3) return fail(RT_ERR_INVALID, "channels must be 1 or 3");
    if ((pr->match_color | 1) != 1) return fail(RT_ERR_INVALID, "match_color must be 0 or 1");
    if (pr->max_history < 1 || pr->max_history > 65535) return fail(RT_ERR_INVALID, "max_history must be 1..65535");
    if (!(pr->normal_cos >= -1.0f && pr->normal_cos <= 1.0f)) return fail(RT_ERR_INVALID, "normal_cos must be -1..1");
    if (!(pr->plane_eps >= 0.0f) || std::isinf(pr->plane_eps)) return fail(RT_ERR_INVALID, "plane_eps must be finite and >= 0");
    if (!(pr->alpha >= 0.0f && pr->alpha <= 1.0f)) return fail(RT_ERR_INVALID, "alpha must be 0..1");
    if (!(pr->alpha_moments >= 0.0f && pr->alpha_moments <= 1.0f)) return fail(RT_ERR_INVALID, "alpha_moments must be 0..1");
    if (W <= 0 || H <= 0) return fail(RT_ERR_INVALID, "need W, H > 0");
    if (x0 < 0 || x1 > W || x0 >= x1) return fail(RT_ERR_INVALID, "need 0 <= x0 < x1 <= W");
    if ((double)W * (double)H > kMaxPixels) return fail(RT_ERR_INVALID, "frame too large for its colours and records");
    return RT_OK;
}

/* the NULL rules, the same for host and device memory */
inline int check_buffers(const rt_camera_desc *cam_prev, const rt_camera_desc *cam, const void *cur, const void *cur_hits,
                         const void *prev_hits, const void *prev_value, const void *prev_moments, const void *prev_len,
                         const void *out_value, const void *out_moments, const void *out_len) {
    if (!cam || !cur || !cur_hits || !out_value || !out_moments || !out_len)
        return fail(RT_ERR_INVALID, "cam / cur / cur_hits / out_value / out_moments / out_len is NULL");
    const int given = (prev_hits != nullptr) + (prev_value != nullptr) + (prev_moments != nullptr) + (prev_len != nullptr) +
                      (cam_prev != nullptr);
    if (given != (prev_hits ? 5 : 0))
        return fail(RT_ERR_INVALID, "first frame: prev_hits, prev_value, prev_moments, prev_len and cam_prev are NULL together or not at all");
    return RT_OK;
}

struct Buffers {             /* the call's buffers, in host or in device memory */
    const void *cur, *cur_hits, *prev_hits, *prev_value, *prev_moments, *prev_len;
    void *out_value, *out_moments, *out_len, *out_variance, *out_flags;
};

/* the device variants' rules for buffers that passed check_buffers: the records (and the motion table, if the call has one: table,
 * table_bytes) 16-byte aligned, the floats 4-byte aligned, no output overlapping a prev_* buffer or the table */
inline int check_device_buffers(const rt_temporal_params *pr, int W, int H, int x0, int x1, const Buffers &b, const void *table,
                                size_t table_bytes, bool has_table) {
    if ((((uintptr_t)b.cur_hits | (uintptr_t)b.prev_hits | (uintptr_t)table) & 15u) != 0)
        return fail(RT_ERR_INVALID, has_table ? "d_cur_hits, d_prev_hits and d_motions must be 16-byte aligned"
                                              : "d_cur_hits and d_prev_hits must be 16-byte aligned");
    if ((((uintptr_t)b.cur | (uintptr_t)b.prev_value | (uintptr_t)b.prev_moments | (uintptr_t)b.prev_len | (uintptr_t)b.out_value |
          (uintptr_t)b.out_moments | (uintptr_t)b.out_len | (uintptr_t)b.out_variance) & 3u) != 0)
        return fail(RT_ERR_INVALID, "the float buffers must be 4-byte aligned");
    const size_t strip = (size_t)(x1 - x0) * (size_t)H, frame = (size_t)W * (size_t)H, cb = (size_t)pr->channels * sizeof(float);
    const void *outs[5] = {b.out_value, b.out_moments, b.out_len, b.out_variance, b.out_flags};
    const size_t out_bytes[5] = {strip * cb, strip * 8, strip * 4, strip * 4, strip};
    const void *prevs[4] = {b.prev_hits, b.prev_value, b.prev_moments, b.prev_len};
    const size_t prev_bytes[4] = {frame * sizeof(rt_hit), frame * cb, frame * 8, frame * 4};
    for (int o = 0; o < 5; ++o) {
        for (int q = 0; q < 4; ++q)
            if (overlap(outs[o], out_bytes[o], prevs[q], prev_bytes[q])) return fail(RT_ERR_INVALID, "an output overlaps a prev_* buffer");
        if (table_bytes && overlap(outs[o], out_bytes[o], table, table_bytes))
            return fail(RT_ERR_INVALID, "an output overlaps the motion table");
    }
    return RT_OK;
}

/* the kernel's arguments: what depends on the parameters, the frame and the previous camera alone, in the header's fp32
 * operations; cam_prev == NULL on a first frame */
inline Args make_args(const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam, int W, int H, int x0,
                      int x1) {
    Args A{};
    A.W = W, A.H = H, A.x0 = x0, A.Wn = x1 - x0;
    A.match_color = pr->match_color, A.plane = pr->plane_eps > 0.0f, A.eps2 = pr->plane_eps * pr->plane_eps;
    A.normal_cos = pr->normal_cos, A.alpha = pr->alpha, A.alpha_moments = pr->alpha_moments, A.max_history = (float)pr->max_history;
    A.fW = (float)W, A.fH = (float)H;
    if (cam_prev) {
        A.identity = std::memcmp(cam_prev, cam, sizeof(rt_camera_desc)) == 0;
        const float *e = cam_prev->eye_origin, *so = cam_prev->screen_origin;
        const V3 hv{cam_prev->vector_horizontal[0], cam_prev->vector_horizontal[1], cam_prev->vector_horizontal[2]};
        const V3 vv{cam_prev->vector_vertical[0], cam_prev->vector_vertical[1], cam_prev->vector_vertical[2]};
        const V3 O{so[0] - e[0], so[1] - e[1], so[2] - e[2]};
        const V3 nh = cross(hv, vv), na = cross(vv, O), nb = cross(O, hv);
        A.eye[0] = e[0], A.eye[1] = e[1], A.eye[2] = e[2];
        A.nh[0] = nh.x, A.nh[1] = nh.y, A.nh[2] = nh.z;
        A.na[0] = na.x, A.na[1] = na.y, A.na[2] = na.z;
        A.nb[0] = nb.x, A.nb[1] = nb.y, A.nb[2] = nb.z;
        A.q = (O.x * nh.x + O.y * nh.y) + O.z * nh.z;
        A.halfwidth = cam_prev->screen_halfwidth, A.width = cam_prev->screen_width;
        A.halfheight = cam_prev->screen_halfheight, A.height = cam_prev->screen_height;
    }
    A.tiles_z = (uint32_t)(((uint64_t)H + kTileZ - 1) / kTileZ);
    A.tiles = (uint64_t)A.tiles_z * (((uint64_t)A.Wn + kTileX - 1) / kTileX);
    return A;
}

inline dim3 grid_of(const Args &A) { return dim3((unsigned)(A.tiles < kMaxGroups ? A.tiles : kMaxGroups)); }

} // namespace

#endif /* RT_ACCUMULATE_BODY_H_ */
