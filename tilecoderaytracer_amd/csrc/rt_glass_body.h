/*
 * rt_glass_body.h -- the step of rt_glass.h's chain, a kernel template of its own which rt_glass.hip instantiates.  It is
 * rt_mirror_body.h's in-place step (records read with three 16-byte loads a lane, no LDS) with the header's one more way to go
 * on, and is built from that file's __device__ helpers: the hash, dot, the direction of a ray.  It is not a GLASS branch of
 * rt_mirror_step_kernel because neither way of making it one could be kept (DESIGN.md section 29,
 * profiles/glass_experiments.txt): as a template parameter of that kernel it adds four instantiations under a name the library
 * is held to have eight of, and as one __device__ function inlined into two kernels it moves the registers of two of the eight.
 * rt_mirror_body.h's kernel is therefore left as it is, and the mirror step of this file -- step 11 of the header -- restates it.
 * rt_glass_child below is the library's one copy of the child's arithmetic: rt_glass_compact_body.h's decision function, which
 * the compacting unit's count and step kernels call, is built on it (DESIGN.md section 31 says why the kernel here does not
 * call that function).
 * Compiled under `#pragma clang fp contract(off)` and the library's arithmetic flags.
 */
#ifndef RT_GLASS_BODY_H_
#define RT_GLASS_BODY_H_

#include "rt_mirror_body.h"

#pragma clang fp contract(off)

constexpr uint32_t kGlassSeen = 1u << 10;              /* rt_glass.h's g, in the state word where out_path has it */

/* rt_glass.h's transmitted child {O, D} of a candidate hit on the object whose table rows (rt_internal_object_glass) are
 * g0 = {tf, ior, kind, 0}, g1 = {centre | normal}, g2 = {- | reverse_normal}: t and P the record's distance and point, E and d
 * the origin and direction of the ray that made it.  rt_capi_refract.h's expressions in that header's order.  Returns `exists`;
 * *s is a sphere's chord, which the path's length takes as well (a pane: not written). */
__device__ __forceinline__ bool rt_glass_child(const float4 g0, const float4 g1, const float4 g2, float t, float Px, float Py, float Pz,
                                               const float *E, float dx, float dy, float dz, float *O, float *D, float *s) {
    if (g0.z == 0.0f) {                                                       /* RT_KIND_SPHERE */
        const float ior = g0.y;
        const float Qx = Px - g1.x, Qy = Py - g1.y, Qz = Pz - g1.z;
        const float ql = sqrtf((Qx * Qx + Qy * Qy) + Qz * Qz);
        const float Nx = Qx / ql, Ny = Qy / ql, Nz = Qz / ql;
        const float eta = 1.0f / ior;
        const float c1 = -rt_mirror_dot(Nx, Ny, Nz, dx, dy, dz);
        const float k1 = 1.0f - (eta * eta) * (1.0f - c1 * c1);
        const float f1 = eta * c1 - sqrtf(k1);
        const float ax = dx * eta + Nx * f1, ay = dy * eta + Ny * f1, az = dz * eta + Nz * f1;
        const float al = sqrtf((ax * ax + ay * ay) + az * az);
        const float T1x = ax / al, T1y = ay / al, T1z = az / al;
        const float chord = -2.0f * rt_mirror_dot(T1x, T1y, T1z, Qx, Qy, Qz);
        const float P2x = Px + T1x * chord, P2y = Py + T1y * chord, P2z = Pz + T1z * chord;
        const float Rx = P2x - g1.x, Ry = P2y - g1.y, Rz = P2z - g1.z;
        const float rl = sqrtf((Rx * Rx + Ry * Ry) + Rz * Rz);
        const float N2x = Rx / rl, N2y = Ry / rl, N2z = Rz / rl;
        const float c2 = rt_mirror_dot(N2x, N2y, N2z, T1x, T1y, T1z);
        const float k2 = 1.0f - (ior * ior) * (1.0f - c2 * c2);
        const float f2 = ior * c2 - sqrtf(k2);
        const float T2x = T1x * ior - N2x * f2, T2y = T1y * ior - N2y * f2, T2z = T1z * ior - N2z * f2;
        const float tl = sqrtf((T2x * T2x + T2y * T2y) + T2z * T2z);
        O[0] = P2x + N2x * 1e-3f, O[1] = P2y + N2y * 1e-3f, O[2] = P2z + N2z * 1e-3f;
        D[0] = T2x / tl, D[1] = T2y / tl, D[2] = T2z / tl;
        *s = chord;
        return t >= 0.0f && !(k1 < 0.0f) && chord > 0.0f && !(k2 < 0.0f);
    }
    const bool towards = rt_mirror_dot(g1.x, g1.y, g1.z, dx, dy, dz) < 0.0f;  /* the record chose `normal`: the child leaves by the other */
    const float Mx = towards ? g2.x : g1.x, My = towards ? g2.y : g1.y, Mz = towards ? g2.z : g1.z;
    const float ix = dx * t + E[0], iy = dy * t + E[1], iz = dz * t + E[2];
    O[0] = ix + Mx * 1e-3f, O[1] = iy + My * 1e-3f, O[2] = iz + Mz * 1e-3f;
    D[0] = dx, D[1] = dy, D[2] = dz;
    return true;
}

/* Bounce s of the m rays of a chunk, one lane a ray (i < m < 2^31), in place: rt_mirror_step_kernel's arguments as its in-place
 * form reads them (rt_mirror_body.h) -- records[3 i ..] the record of ray_s, rays_k[6 i ..] ray_s itself (FIRST: the caller's
 * rays; later the chunk's scratch, which rays_next then is as well: a lane reads its own ray before it writes it), rays0 the
 * caller's rays, state the chunk's planes of `stride` words (14 with GUIDE -- the word, w, L, A -- else 4) -- and glass, the
 * table of rt_internal_object_glass, three float4 an object.  A lane reads its object's tf (4 bytes) when its hit is eligible
 * and the object's 48 bytes only when it is a candidate.  The state word is out_path's (k | cut << 8 | g << 10 | tag << 12) and
 * kMirrorDone.  A ray whose chain ends before the last bounce is retired where it stands: six +0.0f as its next ray and
 * kMirrorDone as its word.  Every address is the ray's own or its object's rows (object < n_objects is checked first): nothing
 * is read or written past them.  Every offset is 64-bit. */
template <bool FIRST, bool GUIDE>
__global__ __launch_bounds__(kMirrorBlock) void rt_glass_step_kernel(uint32_t m, uint32_t stride, int last, float min_reflective,
                                                                     float min_transmissive, const float *__restrict__ rf,
                                                                     const float4 *__restrict__ glass, int n_objects,
                                                                     const float4 *__restrict__ records, const float *rays_k,
                                                                     const float *__restrict__ rays0, float *rays_next, uint32_t *state,
                                                                     float4 *__restrict__ out_hits, float4 *__restrict__ out_guide,
                                                                     float *__restrict__ out_weight, uint32_t *__restrict__ out_path) {
    const uint32_t i = blockIdx.x * (uint32_t)kMirrorBlock + threadIdx.x;
    if (i >= m) return;
    const uint32_t word = FIRST ? 0u : state[i];
    if (word & kMirrorDone) return;
    const float4 q0 = records[3 * (size_t)i], q1 = records[3 * (size_t)i + 1], q2 = records[3 * (size_t)i + 2];
    const int32_t object = __float_as_int(q0.x), flags = __float_as_int(q2.w);
    const uint32_t k = word & 0xffu, tag = word >> 12, seen = word & kGlassSeen;
    float wx = 1.0f, wy = 1.0f, wz = 1.0f, L = 0.0f;
    float A[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (!FIRST) {
        wx = __uint_as_float(state[(size_t)stride + i]);
        wy = __uint_as_float(state[2 * (size_t)stride + i]);
        wz = __uint_as_float(state[3 * (size_t)stride + i]);
        if (GUIDE) {
            L = __uint_as_float(state[4 * (size_t)stride + i]);
#pragma unroll
            for (int c = 0; c < 9; ++c) A[c] = __uint_as_float(state[(size_t)(5 + c) * stride + i]);
        }
    }
    if (GUIDE && object >= 0) L = L + q0.y;
    const bool eligible = object >= 0 && object < n_objects && (flags & RT_HIT_LIGHT) == 0;
    const float refl = (object >= 0 && object < n_objects) ? rf[object] : 0.0f;
    const bool mirror = eligible && refl >= min_reflective;
    const float Px = q0.z, Py = q0.w, Pz = q1.x, nx = q1.y, ny = q1.z, nz = q1.w;
    const float *e_k = rays_k + 6 * (size_t)i;

    bool through = false, sphere = false;
    float tf = 0.0f, chord = 0.0f, O[3], D[3];
    if (eligible) tf = reinterpret_cast<const float *>(glass)[12 * (size_t)object];
    if (eligible && tf > 0.0f && tf >= min_transmissive) {                    /* a candidate: its rows, and the ray's d */
        const float4 g0 = glass[3 * (size_t)object], g1 = glass[3 * (size_t)object + 1], g2 = glass[3 * (size_t)object + 2];
        float dx, dy, dz;
        rt_mirror_direction(e_k, &dx, &dy, &dz);
        sphere = g0.z == 0.0f;
        through = rt_glass_child(g0, g1, g2, q0.y, Px, Py, Pz, e_k, dx, dy, dz, O, D, &chord);
    }
    const bool follow = through || mirror;

    if (!follow || last) {                                                    /* the terminal record */
        out_hits[3 * (size_t)i] = q0, out_hits[3 * (size_t)i + 1] = q1, out_hits[3 * (size_t)i + 2] = q2;
        if (out_weight) {
            float *o = out_weight + 3 * (size_t)i;
            o[0] = wx, o[1] = wy, o[2] = wz;
        }
        if (out_path) out_path[i] = k | (follow ? 1u << 8 : 0u) | seen | tag << 12;
        if (GUIDE) {
            float4 g0 = q0, g1 = q1;
            if (!FIRST && object >= 0 && k != 0u) {
                const float *e = rays0 + 6 * (size_t)i;
                float dx, dy, dz;
                rt_mirror_direction(e, &dx, &dy, &dz);
                g0.x = __int_as_float((int32_t)(tag << 12 | (uint32_t)object));
                g0.y = L;
                g0.z = e[0] + dx * L, g0.w = e[1] + dy * L, g1.x = e[2] + dz * L;
                g1.y = rt_mirror_dot(A[0], A[1], A[2], nx, ny, nz);
                g1.z = rt_mirror_dot(A[3], A[4], A[5], nx, ny, nz);
                g1.w = rt_mirror_dot(A[6], A[7], A[8], nx, ny, nz);
            }
            out_guide[3 * (size_t)i] = g0, out_guide[3 * (size_t)i + 1] = g1, out_guide[3 * (size_t)i + 2] = q2;
        }
        if (!last) {                                                          /* retired: a degenerate ray from here on */
            float *o = rays_next + 6 * (size_t)i;
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = 0.0f;
            state[i] = kMirrorDone;
        }
        return;
    }

    float *o = rays_next + 6 * (size_t)i;
    if (through) {                                                            /* the header's step 10: A is unchanged */
        o[0] = O[0], o[1] = O[1], o[2] = O[2];
        o[3] = O[0] + D[0], o[4] = O[1] + D[1], o[5] = O[2] + D[2];
        state[i] = (k + 1u) | kGlassSeen | (1u + rt_mirror_hash(tag << 12 | (uint32_t)object | 0x80000000u) % 0x7fffeu) << 12;
        state[(size_t)stride + i] = __float_as_uint(wx * (tf * q2.x));
        state[2 * (size_t)stride + i] = __float_as_uint(wy * (tf * q2.y));
        state[3 * (size_t)stride + i] = __float_as_uint(wz * (tf * q2.z));
        if (GUIDE) {
            state[4 * (size_t)stride + i] = __float_as_uint(sphere ? L + chord : L);
            if (FIRST) {                                                      /* (later bounces: the planes hold A already) */
#pragma unroll
                for (int c = 0; c < 9; ++c) state[(size_t)(5 + c) * stride + i] = __float_as_uint(A[c]);
            }
        }
        return;
    }

    float dx, dy, dz;                                                         /* step 11: rt_mirror.h's mirror step */
    rt_mirror_direction(e_k, &dx, &dy, &dz);
    const float c = rt_mirror_dot(nx, ny, nz, dx, dy, dz);
    const float rx = ((-2.0f * nx) * c) + dx, ry = ((-2.0f * ny) * c) + dy, rz = ((-2.0f * nz) * c) + dz;
    o[0] = Px, o[1] = Py, o[2] = Pz;
    o[3] = Px + rx, o[4] = Py + ry, o[5] = Pz + rz;
    state[i] = (k + 1u) | seen | (1u + rt_mirror_hash(tag << 12 | (uint32_t)object) % 0x7fffeu) << 12;
    state[(size_t)stride + i] = __float_as_uint(wx * (refl * q2.x));
    state[2 * (size_t)stride + i] = __float_as_uint(wy * (refl * q2.y));
    state[3 * (size_t)stride + i] = __float_as_uint(wz * (refl * q2.z));
    if (GUIDE) {
        state[4 * (size_t)stride + i] = __float_as_uint(L);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float an = rt_mirror_dot(A[3 * r], A[3 * r + 1], A[3 * r + 2], nx, ny, nz);
            const float two = 2.0f * an;
            state[(size_t)(5 + 3 * r) * stride + i] = __float_as_uint(A[3 * r] - two * nx);
            state[(size_t)(6 + 3 * r) * stride + i] = __float_as_uint(A[3 * r + 1] - two * ny);
            state[(size_t)(7 + 3 * r) * stride + i] = __float_as_uint(A[3 * r + 2] - two * nz);
        }
    }
}

#endif /* RT_GLASS_BODY_H_ */
