/*
 * rt_glass_compact_body.h -- the device code of rt_glass_compact.hip (include/rt_glass_compact.h): whether a glass chain goes on,
 * as ONE function of an entry's record, its ray and its object's table rows, and the two kernels that call it -- the pass that
 * counts the chains that go on, and the step over a dense list.  The arithmetic is rt_glass.h's steps 3 to 8 in that header's
 * order of operations; the child is rt_glass_body.h's rt_glass_child, the one copy.  The in-place rt_glass_step_kernel of that
 * file keeps its own text (DESIGN.md section 31 has the comparison).  Compiled under `#pragma clang fp contract(off)` and the
 * library's arithmetic flags.
 */
#ifndef RT_GLASS_COMPACT_BODY_H_
#define RT_GLASS_COMPACT_BODY_H_

#include "rt_glass_body.h"
#include "rt_scan.h"

#pragma clang fp contract(off)

/* what rt_glass.h's steps 3 to 8 decide about one hit; O, D, chord are the child's where `candidate` (chord: a sphere's) */
struct RtGlassDecision {
    bool eligible, candidate, through, mirror, follow, sphere;
    float refl, tf, chord, O[3], D[3];
};

/* rt_glass.h's steps 3 to 8 of the hit with this object and these flags: tp[0..3] its record's distance and point (words 1 .. 4),
 * e_k[0..5] the ray that made it, rf and glass the tables of rt_internal_object_reflective and rt_internal_object_glass.  It reads
 * rf[object] where the object is one of the scene's, the object's tf when the hit is eligible, and tp, e_k and the object's 48
 * table bytes only when it is a candidate -- nothing else, and nothing at all of a miss.  The count kernel and the step kernel
 * below both decide by this function of the same words, so the ranks the step derives are those the count counted. */
__device__ __forceinline__ RtGlassDecision rt_glass_decide(int32_t object, int32_t flags, const float *tp, const float *e_k,
                                                           float min_reflective, float min_transmissive,
                                                           const float *__restrict__ rf, const float4 *__restrict__ glass,
                                                           int n_objects) {
    RtGlassDecision d;
    const bool known = object >= 0 && object < n_objects;
    d.eligible = known && (flags & RT_HIT_LIGHT) == 0;                        /* step 3 */
    d.refl = known ? rf[object] : 0.0f;
    d.tf = d.eligible ? reinterpret_cast<const float *>(glass)[12 * (size_t)object] : 0.0f;
    d.candidate = d.eligible && d.tf > 0.0f && d.tf >= min_transmissive;      /* step 4 */
    d.through = false, d.sphere = false, d.chord = 0.0f;
    d.O[0] = d.O[1] = d.O[2] = 0.0f, d.D[0] = d.D[1] = d.D[2] = 0.0f;
    if (d.candidate) {                                                        /* steps 5 and 6: its rows, and the ray's d */
        const float4 g0 = glass[3 * (size_t)object], g1 = glass[3 * (size_t)object + 1], g2 = glass[3 * (size_t)object + 2];
        float dx, dy, dz;
        rt_mirror_direction(e_k, &dx, &dy, &dz);
        d.sphere = g0.z == 0.0f;
        d.through = rt_glass_child(g0, g1, g2, tp[0], tp[1], tp[2], tp[3], e_k, dx, dy, dz, d.O, d.D, &d.chord);
    }
    d.mirror = d.eligible && d.refl >= min_reflective;                        /* step 7 */
    d.follow = d.through || d.mirror;                                         /* step 8 */
    return d;
}

/* Of a list's m entries, the chains that go on, per workgroup of the step kernel.  Entry i's record is records[12 i ..] and its
 * ray rays_k[6 i ..]; what is read of them is what rt_glass_decide reads.  Lanes past the end count as ended and read nothing. */
__global__ __launch_bounds__(kMirrorBlock) void rt_glass_compact_count_kernel(uint32_t m, float min_reflective, float min_transmissive,
                                                                              const float *__restrict__ rf,
                                                                              const float4 *__restrict__ glass, int n_objects,
                                                                              const float *__restrict__ records,
                                                                              const float *__restrict__ rays_k,
                                                                              uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_count[kMirrorBlock / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kMirrorBlock + threadIdx.x;
    bool live = false;
    if (i < m) {
        const float *w = records + 12 * (size_t)i;
        live = rt_glass_decide(__float_as_int(w[0]), __float_as_int(w[11]), w + 1, rays_k + 6 * (size_t)i, min_reflective,
                               min_transmissive, rf, glass, n_objects).follow;
    }
    uint32_t count;
    (void)rt_scan_rank(live, wave_count, &count);
    if (threadIdx.x == 0u) counts[blockIdx.x] = count;
}

/* Bounce s of the m entries of a chunk's dense list, one lane an entry (i < m < 2^31): rt_glass_step_kernel's step (rt_glass_body.h)
 * with rt_mirror_step_kernel's COMPACT places (rt_mirror_body.h).  The list holds the rays still alive, in ray order: entry i's
 * record is records[3 i ..], its ray rays_k[6 i ..] (FIRST: the caller's rays), its ray of the chunk idx_k[i] (FIRST: i), its
 * state state_k's planes of `stride` words (14 with GUIDE -- the word, w, L, A -- else 4; FIRST: the header's start, nothing read).
 * The state word is out_path's (k | g << 10 | tag << 12).  A chain that ends writes out_*[ray] and nothing else; one that goes on
 * writes its next ray, state and index to place p of rays_next, state_next and idx_next -- the OTHER list, never the one being
 * read -- where p = group_base[b / kScanBlock] + offsets[b] + the lane's rank among workgroup b's chains that go on; the counts
 * scanned are rt_glass_compact_count_kernel's, which decides by the same function of the same words.  With `last` nothing goes
 * on and neither array is read.  p < the scan's total <= m <= stride.  Every address is the entry's, its ray's, its object's rows
 * (object < n_objects is checked first) or its place's own: nothing is read or written past them.  Every offset is 64-bit. */
template <bool FIRST, bool GUIDE>
__global__ __launch_bounds__(kMirrorBlock) void rt_glass_compact_step_kernel(
    uint32_t m, uint32_t stride, int last, float min_reflective, float min_transmissive, const float *__restrict__ rf,
    const float4 *__restrict__ glass, int n_objects, const float4 *__restrict__ records, const float *__restrict__ rays_k,
    const float *__restrict__ rays0, const uint32_t *__restrict__ state_k, const uint32_t *__restrict__ idx_k,
    float *__restrict__ rays_next, uint32_t *__restrict__ state_next, uint32_t *__restrict__ idx_next,
    const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ group_base, float4 *__restrict__ out_hits,
    float4 *__restrict__ out_guide, float *__restrict__ out_weight, uint32_t *__restrict__ out_path) {
    __shared__ uint32_t wave_count[kMirrorBlock / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kMirrorBlock + threadIdx.x;
    const bool in = i < m;
    float4 q0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), q1 = q0, q2 = q0;
    const float *e_k = rays_k + 6 * (size_t)(in ? i : 0u);
    RtGlassDecision dec{};
    if (in) {
        q0 = records[3 * (size_t)i], q1 = records[3 * (size_t)i + 1], q2 = records[3 * (size_t)i + 2];
        const float tp[4] = {q0.y, q0.z, q0.w, q1.x};
        dec = rt_glass_decide(__float_as_int(q0.x), __float_as_int(q2.w), tp, e_k, min_reflective, min_transmissive, rf, glass,
                              n_objects);
    }
    uint32_t p = 0;
    if (!last) {                                                              /* (uniform; every lane of the workgroup ranks) */
        uint32_t count;
        p = rt_scan_rank(in && dec.follow, wave_count, &count);
        p += group_base[blockIdx.x / (uint32_t)kScanBlock] + offsets[blockIdx.x];
    }
    if (!in) return;
    const uint32_t word = FIRST ? 0u : state_k[i];
    const uint32_t ray = FIRST ? i : idx_k[i];                                /* the entry's ray of the chunk */
    const int32_t object = __float_as_int(q0.x);
    const uint32_t k = word & 0xffu, tag = word >> 12, seen = word & kGlassSeen;
    float wx = 1.0f, wy = 1.0f, wz = 1.0f, L = 0.0f;
    float A[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (!FIRST) {
        wx = __uint_as_float(state_k[(size_t)stride + i]);
        wy = __uint_as_float(state_k[2 * (size_t)stride + i]);
        wz = __uint_as_float(state_k[3 * (size_t)stride + i]);
        if (GUIDE) {
            L = __uint_as_float(state_k[4 * (size_t)stride + i]);
#pragma unroll
            for (int c = 0; c < 9; ++c) A[c] = __uint_as_float(state_k[(size_t)(5 + c) * stride + i]);
        }
    }
    if (GUIDE && object >= 0) L = L + q0.y;
    const float Px = q0.z, Py = q0.w, Pz = q1.x, nx = q1.y, ny = q1.z, nz = q1.w;

    if (!dec.follow || last) {                                                /* the terminal record */
        out_hits[3 * (size_t)ray] = q0, out_hits[3 * (size_t)ray + 1] = q1, out_hits[3 * (size_t)ray + 2] = q2;
        if (out_weight) {
            float *o = out_weight + 3 * (size_t)ray;
            o[0] = wx, o[1] = wy, o[2] = wz;
        }
        if (out_path) out_path[ray] = k | (dec.follow ? 1u << 8 : 0u) | seen | tag << 12;
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
        return;
    }

    float *o = rays_next + 6 * (size_t)p;
    idx_next[p] = ray;
    if (dec.through) {                                                        /* the header's step 10: A is carried unchanged */
        o[0] = dec.O[0], o[1] = dec.O[1], o[2] = dec.O[2];
        o[3] = dec.O[0] + dec.D[0], o[4] = dec.O[1] + dec.D[1], o[5] = dec.O[2] + dec.D[2];
        state_next[p] = (k + 1u) | kGlassSeen | (1u + rt_mirror_hash(tag << 12 | (uint32_t)object | 0x80000000u) % 0x7fffeu) << 12;
        state_next[(size_t)stride + p] = __float_as_uint(wx * (dec.tf * q2.x));
        state_next[2 * (size_t)stride + p] = __float_as_uint(wy * (dec.tf * q2.y));
        state_next[3 * (size_t)stride + p] = __float_as_uint(wz * (dec.tf * q2.z));
        if (GUIDE) {
            state_next[4 * (size_t)stride + p] = __float_as_uint(dec.sphere ? L + dec.chord : L);
#pragma unroll
            for (int c = 0; c < 9; ++c) state_next[(size_t)(5 + c) * stride + p] = __float_as_uint(A[c]);
        }
        return;
    }

    float dx, dy, dz;                                                         /* step 11: rt_mirror.h's mirror step */
    rt_mirror_direction(e_k, &dx, &dy, &dz);
    const float c = rt_mirror_dot(nx, ny, nz, dx, dy, dz);
    const float rx = ((-2.0f * nx) * c) + dx, ry = ((-2.0f * ny) * c) + dy, rz = ((-2.0f * nz) * c) + dz;
    o[0] = Px, o[1] = Py, o[2] = Pz;
    o[3] = Px + rx, o[4] = Py + ry, o[5] = Pz + rz;
    state_next[p] = (k + 1u) | seen | (1u + rt_mirror_hash(tag << 12 | (uint32_t)object) % 0x7fffeu) << 12;
    state_next[(size_t)stride + p] = __float_as_uint(wx * (dec.refl * q2.x));
    state_next[2 * (size_t)stride + p] = __float_as_uint(wy * (dec.refl * q2.y));
    state_next[3 * (size_t)stride + p] = __float_as_uint(wz * (dec.refl * q2.z));
    if (GUIDE) {
        state_next[4 * (size_t)stride + p] = __float_as_uint(L);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float an = rt_mirror_dot(A[3 * r], A[3 * r + 1], A[3 * r + 2], nx, ny, nz);
            const float two = 2.0f * an;
            state_next[(size_t)(5 + 3 * r) * stride + p] = __float_as_uint(A[3 * r] - two * nx);
            state_next[(size_t)(6 + 3 * r) * stride + p] = __float_as_uint(A[3 * r + 1] - two * ny);
            state_next[(size_t)(7 + 3 * r) * stride + p] = __float_as_uint(A[3 * r + 2] - two * nz);
        }
    }
}

#endif /* RT_GLASS_COMPACT_BODY_H_ */
