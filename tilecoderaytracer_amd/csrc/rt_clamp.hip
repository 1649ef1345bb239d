/*
 * rt_clamp.hip -- implementation of include/rt_clamp.h: neighbourhood clipping of an accumulated history.  The header is the
 * definition; the kernel is bit-exact to it (the library's arithmetic flags: no contraction, correctly rounded divide and square
 * root, denormals kept).
 *
 * SHAPE.  One launch a call, one lane a pixel, a workgroup of four wavefronts: 64 consecutive z of four
 * columns, so that x and a window row's bounds are wave-uniform.  A lane reads its own record, value, moments and length; only a
 * lane that is alive with a history longer than one walks the (2r+1)^2 window, behind a branch a wavefront without such a lane
 * skips -- a first frame costs its own words.  The kernels are specialised on channels and radius (the window is straight-line
 * code); box and match_color are kernel arguments (a colour mask, one branch after the window).  Two forms of the window's reads:
 *   direct   each lane loads its taps' words from global memory: the object word and the two 16-byte thirds of the record that
 *            hold the normal and colour | flags, and the tap's cur words; a tap that does not exist reads the lane's own cell and
 *            is dropped by a select, so the loads of a row stay unconditional.
 *   LDS      the workgroup stages its tile and a halo of r cells -- key {object, colour bits (zeros without match_color)}, aux
 *            {normal, side | dead << 2} and the cur words, 44 bytes a cell with three channels and 36 with one: 6 x 66 to
 *            10 x 70 cells, 14 512 to 31 056 bytes -- and the lanes walk the window there; a cell outside the rectangle is
 *            staged dead, so the walk has no bounds.  A workgroup none of whose lanes walks stages nothing.
 * The library has the LDS form: at 4096 x 4096 it takes 0.36 ms against the direct form's 0.82 at r = 1 with three channels, a
 * device copy of the call's bytes taking 0.35, and it is ahead at every radius and with one channel too.  RT_CLAMP_LDS picks
 * the form the library has; -DRT_CLAMP_VARIANTS=1 (scripts/clamp_experiments.py) builds both and exports the switch between
 * them, rt_internal_clamp_variant().  profiles/clamp_experiments.txt has the numbers.
 *
 * IN PLACE.  out_value, out_moments and out_len may be value, moments and len: a lane reads those at its own pixel alone, before
 * it writes them, and cur and hits -- read at neighbours -- are never written.  Every output cell of the rectangle is written
 * exactly once, dead pixels too, with plain vector stores.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/rt_clamp.h"
#include "rt_host.h"

static_assert(sizeof(rt_hit) == 48, "rt_hit layout");
static_assert(sizeof(rt_clamp_params) == 32, "rt_clamp_params layout");

#ifndef RT_CLAMP_LDS
#define RT_CLAMP_LDS 1                 /* the window's reads in the library: 0 direct loads, 1 (kept) a tile staged in LDS */
#endif
#ifndef RT_CLAMP_VARIANTS
#define RT_CLAMP_VARIANTS 0            /* 1: both forms, and the entry point that names one */
#endif

namespace {

constexpr int kTileZ = 64, kTileX = 4;                 /* a workgroup: 4 wavefronts, each 64 consecutive z of one column */
constexpr double kMaxPixels = 2.0e9 * 4.0 * 4.0 / 60.0; /* rt_render_gbuffer's limit: 3.2e10 bytes of colours and records */
constexpr uint32_t kDead = 4u;                         /* aux.w: flags & 3, and this bit for a miss or a light */

/* the kernels' arguments.  The history's inputs and outputs carry no __restrict__: they may be the same buffers. */
struct ClampArgs {
    const float *cur;
    const uint4 *hits;
    const float *value, *moments, *len;
    float *out_value, *out_moments, *out_len, *out_variance;
    uint8_t *out_flags;
    int Wn, H;
    uint32_t tiles_z;
    uint32_t color_mask;                               /* ~0 with match_color, else 0 */
    int box;
    float min_taps, clip_history, normal_cos, gamma;
};

/* what the window gives a pixel */
template <int kC>
struct Window {
    float cnt, s1[kC], s2[kC], mn[kC], mx[kC];
    __device__ __forceinline__ void start(const float *c) {
        cnt = 0.0f;
#pragma unroll
        for (int k = 0; k < kC; ++k) s1[k] = s2[k] = 0.0f, mn[k] = mx[k] = c[k];
    }
    /* header step 2's lines for a tap, taken only if `counts` (selects: the caller's loads stay unconditional) */
    __device__ __forceinline__ void tap(bool counts, const float *c) {
        cnt = counts ? cnt + 1.0f : cnt;
#pragma unroll
        for (int k = 0; k < kC; ++k) {
            s1[k] = counts ? s1[k] + c[k] : s1[k];
            s2[k] = counts ? s2[k] + c[k] * c[k] : s2[k];
            mn[k] = (counts & (c[k] < mn[k])) ? c[k] : mn[k];          /* (no short circuit: selects, not branches) */
            mx[k] = (counts & (c[k] > mx[k])) ? c[k] : mx[k];
        }
    }
};

template <int kC>
__device__ __forceinline__ float clamp_lum(const float *c) {
    return kC == 3 ? (0.25f * c[0] + 0.5f * c[1]) + 0.25f * c[2] : c[0];
}

/* header steps 2's end to 5 and the stores of pixel p; walked: the pixel is alive with a history longer than one, and w is its
 * window */
template <int kC>
__device__ __forceinline__ void clamp_finish(const ClampArgs &a, int64_t p, bool walked, const Window<kC> &w, const float *v,
                                             float m1, float m2, float L) {
    float vo[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) vo[k] = v[k];
    bool clipped = false;
    uint8_t flag = 0;
    if (walked) {
        if (w.cnt < a.min_taps) {
            flag = 2;
        } else {
#pragma unroll
            for (int k = 0; k < kC; ++k) {
                float lo = w.mn[k], hi = w.mx[k];
                if (a.box) {
                    const float mean = w.s1[k] / w.cnt, e2 = w.s2[k] / w.cnt;
                    float var = e2 - mean * mean;
                    var = var > 0.0f ? var : 0.0f;
                    const float g = a.gamma * sqrtf(var);
                    lo = mean - g, hi = mean + g;
                }
                float t = v[k];
                const bool below = v[k] < lo;
                t = below ? lo : t;
                const bool above = t > hi;
                t = above ? hi : t;
                clipped = clipped | below | above;
                vo[k] = t;
            }
        }
    }
    float m1o = m1, m2o = m2, Lo = L;
    if (clipped) {
        flag = 1;
        if (!(L <= a.clip_history)) Lo = a.clip_history;
        m1o = m1 + (clamp_lum<kC>(vo) - clamp_lum<kC>(v));
        m2o = m2 + (m1o * m1o - m1 * m1);
    }
    const float t = m2o - m1o * m1o;
#pragma unroll
    for (int k = 0; k < kC; ++k) a.out_value[p * kC + k] = vo[k];
    a.out_moments[p * 2] = m1o, a.out_moments[p * 2 + 1] = m2o;
    a.out_len[p] = Lo;
    if (a.out_variance) a.out_variance[p] = t > 0.0f ? t : 0.0f;
    if (a.out_flags) a.out_flags[p] = flag;
}

} // namespace

#if !RT_CLAMP_LDS || RT_CLAMP_VARIANTS
/* the window read with direct loads */
template <int kC, int kR>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_clamp_direct_kernel(const ClampArgs a) {
    const uint32_t tz = blockIdx.x % a.tiles_z, tx = blockIdx.x / a.tiles_z;
    const int64_t x64 = (int64_t)tx * kTileX + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int64_t z64 = (int64_t)tz * kTileZ + threadIdx.x;
    if (x64 >= a.Wn || z64 >= a.H) return;              /* (no barrier below: a thread without a pixel leaves) */
    const int x = (int)x64, z = (int)z64;
    const int64_t p = x64 * (int64_t)a.H + z;
    const uint32_t op = a.hits[3 * p].x;
    const uint4 p2 = a.hits[3 * p + 2];
    const float m1 = a.moments[p * 2], m2 = a.moments[p * 2 + 1], L = a.len[p];
    float v[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) v[k] = a.value[p * kC + k];
    const bool dead = (int32_t)op < 0 || (p2.w & (uint32_t)RT_HIT_LIGHT) != 0u;
    const bool walked = !dead && L > 1.0f;
    Window<kC> w;
    w.start(v);                                         /* (overwritten below; a pixel that is not walked never reads it) */
    if (walked) {
        const uint4 p1 = a.hits[3 * p + 1];
        const float npx = __uint_as_float(p1.y), npy = __uint_as_float(p1.z), npz = __uint_as_float(p1.w);
        float c[kC];
#pragma unroll
        for (int k = 0; k < kC; ++k) c[k] = a.cur[p * kC + k];
        w.start(c);
#pragma unroll
        for (int da = -kR; da <= kR; ++da) {
            const int xq = x + da;
            if (xq < 0 || xq >= a.Wn) continue;         /* (wave-uniform) */
            const int64_t row = (int64_t)xq * (int64_t)a.H;
#pragma unroll
            for (int db = -kR; db <= kR; ++db) {
                if (da == 0 && db == 0) {
                    w.tap(true, c);
                    continue;
                }
                const int zq = z + db;
                const bool inside = zq >= 0 && zq < a.H;
                const int64_t q = row + (inside ? zq : z);          /* a tap that does not exist reads this row's own z */
                const uint32_t oq = a.hits[3 * q].x;
                const uint4 q1 = a.hits[3 * q + 1], q2 = a.hits[3 * q + 2];
                float cq[kC];
#pragma unroll
                for (int k = 0; k < kC; ++k) cq[k] = a.cur[q * kC + k];
                const bool dead_q = (int32_t)oq < 0 || (q2.w & (uint32_t)RT_HIT_LIGHT) != 0u;
                const uint32_t differ = (oq ^ op) | ((q2.w ^ p2.w) & 3u) |
                                        (((q2.x ^ p2.x) | (q2.y ^ p2.y) | (q2.z ^ p2.z)) & a.color_mask);
                const float t = (npx * __uint_as_float(q1.y) + npy * __uint_as_float(q1.z)) + npz * __uint_as_float(q1.w);
                w.tap(inside & !dead_q & (differ == 0u) & (t >= a.normal_cos), cq);
            }
        }
    }
    clamp_finish<kC>(a, p, walked, w, v, m1, m2, L);
}
#endif

#if RT_CLAMP_LDS || RT_CLAMP_VARIANTS
/* the window read from a tile staged in LDS: the same arithmetic in the same order */
template <int kC, int kR>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_clamp_lds_kernel(const ClampArgs a) {
    constexpr int kLx = kTileX + 2 * kR, kLz = kTileZ + 2 * kR;
    __shared__ uint4 s_key[kLx][kLz], s_aux[kLx][kLz];
    __shared__ float s_cur[kC][kLx][kLz];
    const uint32_t tz = blockIdx.x % a.tiles_z, tx = blockIdx.x / a.tiles_z;
    const int64_t x0 = (int64_t)tx * kTileX, z0 = (int64_t)tz * kTileZ;
    const int64_t x64 = x0 + threadIdx.y, z64 = z0 + threadIdx.x;
    const bool mine = x64 < a.Wn && z64 < a.H;          /* (a thread without a pixel stays for the barriers) */
    const int64_t p = mine ? x64 * (int64_t)a.H + z64 : 0;
    float m1 = 0.0f, m2 = 0.0f, L = 0.0f;
    float v[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) v[k] = 0.0f;
    bool walked = false;
    if (mine) {
        const uint32_t op = a.hits[3 * p].x, fp = a.hits[3 * p + 2].w;
        m1 = a.moments[p * 2], m2 = a.moments[p * 2 + 1], L = a.len[p];
#pragma unroll
        for (int k = 0; k < kC; ++k) v[k] = a.value[p * kC + k];
        walked = !((int32_t)op < 0 || (fp & (uint32_t)RT_HIT_LIGHT) != 0u) && L > 1.0f;
    }
    Window<kC> w;
    w.start(v);
    if (__syncthreads_or(walked)) {
        for (int cell = (int)(threadIdx.y * kTileZ + threadIdx.x); cell < kLx * kLz; cell += kTileX * kTileZ) {
            const int i = cell / kLz, j = cell % kLz;
            const int64_t xq = x0 - kR + i, zq = z0 - kR + j;
            uint4 key = make_uint4(0u, 0u, 0u, 0u), aux = make_uint4(0u, 0u, 0u, kDead);     /* outside the rectangle: dead */
            float cq[kC];
#pragma unroll
            for (int k = 0; k < kC; ++k) cq[k] = 0.0f;
            if (xq >= 0 && xq < a.Wn && zq >= 0 && zq < a.H) {
                const int64_t q = xq * (int64_t)a.H + zq;
                const uint32_t oq = a.hits[3 * q].x;
                const uint4 q1 = a.hits[3 * q + 1], q2 = a.hits[3 * q + 2];
                const bool dead_q = (int32_t)oq < 0 || (q2.w & (uint32_t)RT_HIT_LIGHT) != 0u;
                key = make_uint4(oq, q2.x & a.color_mask, q2.y & a.color_mask, q2.z & a.color_mask);
                aux = make_uint4(q1.y, q1.z, q1.w, (q2.w & 3u) | (dead_q ? kDead : 0u));
#pragma unroll
                for (int k = 0; k < kC; ++k) cq[k] = a.cur[q * kC + k];
            }
            s_key[i][j] = key, s_aux[i][j] = aux;
#pragma unroll
            for (int k = 0; k < kC; ++k) s_cur[k][i][j] = cq[k];
        }
        __syncthreads();
        if (walked) {
            const int ci = (int)threadIdx.y + kR, cj = (int)threadIdx.x + kR;
            const uint4 kp = s_key[ci][cj], ap = s_aux[ci][cj];
            const float npx = __uint_as_float(ap.x), npy = __uint_as_float(ap.y), npz = __uint_as_float(ap.z);
            float c[kC];
#pragma unroll
            for (int k = 0; k < kC; ++k) c[k] = s_cur[k][ci][cj];
            w.start(c);
#pragma unroll
            for (int da = -kR; da <= kR; ++da) {
#pragma unroll
                for (int db = -kR; db <= kR; ++db) {
                    if (da == 0 && db == 0) {
                        w.tap(true, c);
                        continue;
                    }
                    const uint4 kq = s_key[ci + da][cj + db], aq = s_aux[ci + da][cj + db];
                    float cq[kC];
#pragma unroll
                    for (int k = 0; k < kC; ++k) cq[k] = s_cur[k][ci + da][cj + db];
                    const uint32_t differ = (kq.x ^ kp.x) | (kq.y ^ kp.y) | (kq.z ^ kp.z) | (kq.w ^ kp.w) | ((aq.w ^ ap.w) & 3u);
                    const float t = (npx * __uint_as_float(aq.x) + npy * __uint_as_float(aq.y)) + npz * __uint_as_float(aq.z);
                    w.tap(((aq.w & kDead) == 0u) & (differ == 0u) & (t >= a.normal_cos), cq);
                }
            }
        }
    }
    if (!mine) return;
    clamp_finish<kC>(a, p, walked, w, v, m1, m2, L);
}
#endif

namespace {

/* the header's checks up to the buffers, in its order */
int check_shape(const rt_clamp_params *pr, int Wn, int H) {
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->channels != 1 && pr->channels != 3) return fail(RT_ERR_INVALID, "channels must be 1 or 3");
    if ((pr->box | 1) != 1) return fail(RT_ERR_INVALID, "box must be 0 or 1");
    if (pr->radius < 1 || pr->radius > 3) return fail(RT_ERR_INVALID, "radius must be 1..3");
    if ((pr->match_color | 1) != 1) return fail(RT_ERR_INVALID, "match_color must be 0 or 1");
    if (pr->min_taps < 1 || pr->min_taps > 49) return fail(RT_ERR_INVALID, "min_taps must be 1..49");
    if (pr->clip_history < 1 || pr->clip_history > 65535) return fail(RT_ERR_INVALID, "clip_history must be 1..65535");
    if (!(pr->normal_cos >= -1.0f && pr->normal_cos <= 1.0f)) return fail(RT_ERR_INVALID, "normal_cos must be in -1..1");
    if (!(pr->gamma >= 0.0f) || std::isinf(pr->gamma)) return fail(RT_ERR_INVALID, "gamma must be finite and >= 0");
    if (Wn <= 0 || H <= 0) return fail(RT_ERR_INVALID, "need Wn, H > 0");
    if ((double)Wn * (double)H > kMaxPixels) return fail(RT_ERR_INVALID, "rectangle too large for its values and records");
    return RT_OK;
}

struct Buffers {             /* the call's buffers, in device memory */
    const void *cur, *hits, *value, *moments, *len;
    void *out_value, *out_moments, *out_len, *out_variance, *out_flags;
};

using Launch = void (*)(dim3, hipStream_t, const ClampArgs &);

#if !RT_CLAMP_LDS || RT_CLAMP_VARIANTS
template <int kC, int kR>
void launch_direct(dim3 grid, hipStream_t stream, const ClampArgs &a) {
    hipLaunchKernelGGL((rt_clamp_direct_kernel<kC, kR>), grid, dim3(kTileZ, kTileX), 0, stream, a);
}
const Launch kDirect[2][3] = {{launch_direct<1, 1>, launch_direct<1, 2>, launch_direct<1, 3>},
                              {launch_direct<3, 1>, launch_direct<3, 2>, launch_direct<3, 3>}};
#endif
#if RT_CLAMP_LDS || RT_CLAMP_VARIANTS
template <int kC, int kR>
void launch_lds(dim3 grid, hipStream_t stream, const ClampArgs &a) {
    hipLaunchKernelGGL((rt_clamp_lds_kernel<kC, kR>), grid, dim3(kTileZ, kTileX), 0, stream, a);
}
const Launch kLds[2][3] = {{launch_lds<1, 1>, launch_lds<1, 2>, launch_lds<1, 3>},
                           {launch_lds<3, 1>, launch_lds<3, 2>, launch_lds<3, 3>}};
#endif

#if RT_CLAMP_VARIANTS
bool g_lds = RT_CLAMP_LDS != 0;
#endif

/* the one launch, enqueued on stream; every argument already checked, the device current */
int enqueue(const rt_clamp_params *pr, int Wn, int H, const Buffers &b, hipStream_t stream) {
    const uint32_t tiles_z = (uint32_t)((H + kTileZ - 1) / kTileZ);
    const dim3 grid(tiles_z * (uint32_t)(((int64_t)Wn + kTileX - 1) / kTileX));
    const ClampArgs a{static_cast<const float *>(b.cur),    static_cast<const uint4 *>(b.hits),  static_cast<const float *>(b.value),
                      static_cast<const float *>(b.moments), static_cast<const float *>(b.len),   static_cast<float *>(b.out_value),
                      static_cast<float *>(b.out_moments),   static_cast<float *>(b.out_len),     static_cast<float *>(b.out_variance),
                      static_cast<uint8_t *>(b.out_flags),   Wn, H, tiles_z, pr->match_color ? ~0u : 0u, pr->box,
                      (float)pr->min_taps, (float)pr->clip_history, pr->normal_cos, pr->gamma};
    const int c = pr->channels == 3, r = pr->radius - 1;
#if RT_CLAMP_VARIANTS
    (g_lds ? kLds : kDirect)[c][r](grid, stream, a);
#elif RT_CLAMP_LDS
    kLds[c][r](grid, stream, a);
#else
    kDirect[c][r](grid, stream, a);
#endif
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

} // namespace

extern "C" {

int rt_capi_clamp_version(void) { return RT_CAPI_CLAMP_VERSION; }

#if RT_CLAMP_VARIANTS
/* 0: direct loads; 1: through LDS; returns what was set before */
int rt_internal_clamp_variant(int lds) {
    const int before = g_lds;
    g_lds = lds != 0;
    return before;
}
#endif

int rt_history_clamp(int device, const rt_clamp_params *pr, int Wn, int H, const float *cur, const rt_hit *hits, const float *value,
                     const float *moments, const float *len, float *out_value, float *out_moments, float *out_len,
                     float *out_variance, uint8_t *out_flags, double *kernel_ms) {
    int rc = check_shape(pr, Wn, H);
    if (rc) return rc;
    if (!cur || !hits || !value || !moments || !len || !out_value || !out_moments || !out_len)
        return fail(RT_ERR_INVALID, "cur / hits / value / moments / len / out_value / out_moments / out_len is NULL");
    if ((rc = rt_internal_check_device(device))) return rc;
    const size_t pixels = (size_t)Wn * (size_t)H, cb = (size_t)pr->channels * sizeof(float);
    const HostIn in[5] = {{cur, pixels * cb}, {hits, pixels * sizeof(rt_hit)}, {value, pixels * cb}, {moments, pixels * 8},
                          {len, pixels * 4}};
    const HostOut out[5] = {{out_value, pixels * cb}, {out_moments, pixels * 8}, {out_len, pixels * 4}, {out_variance, pixels * 4},
                            {out_flags, pixels}};
    return staged_call(device, in, 5, out, 5, 0, kernel_ms, [&](void *const *d_in, void *const *d_out, void *) {
        const Buffers b{d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], d_out[0], d_out[1], d_out[2], d_out[3], d_out[4]};
        return enqueue(pr, Wn, H, b, nullptr);
    });
}

int rt_history_clamp_device(int device, const rt_clamp_params *pr, int Wn, int H, const void *d_cur, const void *d_hits,
                            const void *d_value, const void *d_moments, const void *d_len, void *d_out_value, void *d_out_moments,
                            void *d_out_len, void *d_out_variance, void *d_out_flags, void *hip_stream) {
    int rc = check_shape(pr, Wn, H);
    if (rc) return rc;
    if (!d_cur || !d_hits || !d_value || !d_moments || !d_len || !d_out_value || !d_out_moments || !d_out_len)
        return fail(RT_ERR_INVALID, "d_cur / d_hits / d_value / d_moments / d_len / d_out_value / d_out_moments / d_out_len is NULL");
    if (((uintptr_t)d_hits & 15u) != 0) return fail(RT_ERR_INVALID, "d_hits must be 16-byte aligned");
    if ((((uintptr_t)d_cur | (uintptr_t)d_value | (uintptr_t)d_moments | (uintptr_t)d_len | (uintptr_t)d_out_value |
          (uintptr_t)d_out_moments | (uintptr_t)d_out_len | (uintptr_t)d_out_variance) & 3u) != 0)
        return fail(RT_ERR_INVALID, "the float buffers must be 4-byte aligned");
    const size_t pixels = (size_t)Wn * (size_t)H, cb = (size_t)pr->channels * sizeof(float);
    /* the outputs, then the inputs: outputs 0..2 may be inputs 2..4 exactly (in place), and nothing else may share a byte */
    const void *outs[5] = {d_out_value, d_out_moments, d_out_len, d_out_variance, d_out_flags};
    const size_t out_bytes[5] = {pixels * cb, pixels * 8, pixels * 4, pixels * 4, pixels};
    const void *ins[5] = {d_cur, d_hits, d_value, d_moments, d_len};
    const size_t in_bytes[5] = {pixels * cb, pixels * sizeof(rt_hit), pixels * cb, pixels * 8, pixels * 4};
    for (int o = 0; o < 5; ++o) {
        for (int q = o + 1; q < 5; ++q)
            if (overlap(outs[o], out_bytes[o], outs[q], out_bytes[q])) return fail(RT_ERR_INVALID, "an output overlaps another output");
        for (int q = 0; q < 5; ++q) {
            if (o < 3 && q == o + 2 && outs[o] == ins[q]) continue;     /* in place: the same buffer, the same bytes */
            if (overlap(outs[o], out_bytes[o], ins[q], in_bytes[q]))
                return fail(RT_ERR_INVALID, q < 2 ? "an output overlaps d_cur or d_hits"
                                                  : "an output overlaps an input that is not its own, or its own input partially");
        }
    }
    if ((rc = rt_internal_check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    const Buffers b{d_cur, d_hits, d_value, d_moments, d_len, d_out_value, d_out_moments, d_out_len, d_out_variance, d_out_flags};
    return enqueue(pr, Wn, H, b, static_cast<hipStream_t>(hip_stream));
}

} // extern "C"
