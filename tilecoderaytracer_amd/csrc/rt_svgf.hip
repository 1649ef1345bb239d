/*
 * rt_svgf.hip -- implementation of include/rt_svgf.h: the variance-steered a-trous filter over what rt_temporal_accumulate
 * writes.  The header is the definition; these kernels are bit-exact to it (the library's arithmetic flags: no contraction,
 * correctly rounded divide, denormals kept).
 *
 * SHAPE (rt_denoise.hip's, section 16, with what the variance adds).
 *   pack       the 48-byte records -> 16-byte planes: key = {object, colour bits (zeros without match_color)}, aux = {normal,
 *              side | dead << 2} and, with sigma_plane > 0 only, pnt = {point, 0}.  The side bits (flags & 3) ride in aux.w beside
 *              the dead bit: aux is loaded for every tap anyway, the comparison is one xor-and folded into the key's, and the
 *              object keeps all its 32 bits.
 *   estimate   header step A, one lane a pixel, and the first frame of values: {r, g, b, var0} (one channel: {v, var0}).  Only
 *              lanes with a short history walk the (2r+1)^2 window, with direct loads behind a branch: a wavefront none of
 *              whose lanes needs it skips the loop altogether.  The window read from a tile staged in LDS
 *              (RT_SVGF_ESTIMATE_LDS) measured 0.55 ms less on a first frame and 3 % more with one channel over a long
 *              history, the frame that repeats: not kept.
 *   prefilter  header step B's vf and invl = 1 / (sigma_l^2 vf + epsilon), with sigma_l > 0 only: nine unit-offset loads of the
 *              variance.  With three channels the iteration kernel makes it for its own pixels (3.4 to 4.4 % faster at five
 *              iterations than a pass that stores invl, 4 bytes a pixel); with one channel the pass is kept (the kernel making
 *              it measured 6 % slower).  RT_SVGF_FUSED_PREFILTER builds either for both.
 *   iteration  one launch per iteration, rt_denoise's kernel: the 64 lanes of a wavefront along z, a wavefront filters kPixels
 *              columns one step apart whose windows share their rows, taps are straight-line selects.  A tap's variance travels
 *              in the fourth word of its value -- {r, g, b, var}, one 16-byte load -- and the luminance is recomputed once a
 *              loaded tap (five operations shared by the up to five pixels the tap feeds); {r, g, b, lum} with the variance in
 *              a 4-byte plane (RT_SVGF_VAR_PLANE) measured 2 to 3 % faster with the luminance term and 7 % slower without, and
 *              is not kept.  The kernel holds per pixel the centre's value, variance, luminance, key, normal, point, invl and
 *              five sums: kPixels is 4 here, not rt_denoise's 8 -- 94 to 132 registers and 3 to 5 wavefronts a SIMD against 161
 *              to 222 and 2 to 3, neither with scratch; 8 measured 15 % slower with three channels and 2 to 3 % faster with
 *              one (RT_SVGF_PIXELS builds it).  profiles/svgf_experiments.txt has every number.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/rt_svgf.h"
#include "rt_host.h"

static_assert(sizeof(rt_hit) == 48, "rt_hit layout");
static_assert(sizeof(rt_svgf_params) == 36, "rt_svgf_params layout");

#ifndef RT_SVGF_PIXELS
#define RT_SVGF_PIXELS 4               /* the columns, one step apart, a wavefront filters together (4 or 8) */
#endif
#ifndef RT_SVGF_FUSED_PREFILTER
#define RT_SVGF_FUSED_PREFILTER 2      /* who makes vf: 0 a pass of its own, 1 the iteration kernel, 2 (kept) the kernel for three
                                          channels and the pass for one */
#endif
#ifndef RT_SVGF_ESTIMATE_LDS
#define RT_SVGF_ESTIMATE_LDS 0         /* 1: the estimate's window reads a tile staged in LDS -- measured and not kept */
#endif
#ifndef RT_SVGF_VAR_PLANE
#define RT_SVGF_VAR_PLANE 0            /* 1: three channels travel as {r, g, b, lum} with the variance in a 4-byte plane behind
                                          the cells -- measured and not kept */
#endif

namespace {

constexpr int kTileZ = 64, kTileX = 4;                 /* a workgroup: 4 wavefronts, each 64 consecutive z */
constexpr int kPixels = RT_SVGF_PIXELS;
constexpr double kMaxPixels = 2.0e9 * 4.0 * 4.0 / 60.0; /* rt_render_gbuffer's limit: 3.2e10 bytes of colours and records */
constexpr bool fused_prefilter(int channels) {          /* the iteration kernel makes vf itself, and there is no prefilter pass */
    return RT_SVGF_FUSED_PREFILTER == 1 || (RT_SVGF_FUSED_PREFILTER == 2 && channels == 3);
}
constexpr uint32_t kDead = 4u;                         /* aux.w: flags & 3, and this bit for a miss or a light */

} // namespace

/* a value with its variance, as it travels between the passes */
template <int kC>
struct SvgfCell;
template <>
struct SvgfCell<3> {
    float4 w;
    __device__ __forceinline__ float c(int k) const { return k == 0 ? w.x : k == 1 ? w.y : w.z; }
#if RT_SVGF_VAR_PLANE
    static constexpr bool kVarPlane = true;              /* the fourth word is the luminance, the variance lies in the plane */
    __device__ __forceinline__ float var() const { return 0.0f; }
    __device__ __forceinline__ float lum() const { return w.w; }
    static __device__ __forceinline__ SvgfCell make(const float *c, float) {
        return SvgfCell{make_float4(c[0], c[1], c[2], (0.25f * c[0] + 0.5f * c[1]) + 0.25f * c[2])};
    }
#else
    static constexpr bool kVarPlane = false;
    __device__ __forceinline__ float var() const { return w.w; }
    __device__ __forceinline__ float lum() const { return (0.25f * w.x + 0.5f * w.y) + 0.25f * w.z; }
    static __device__ __forceinline__ SvgfCell make(const float *c, float var) { return SvgfCell{make_float4(c[0], c[1], c[2], var)}; }
#endif
};
template <>
struct SvgfCell<1> {
    float2 w;
    static constexpr bool kVarPlane = false;
    __device__ __forceinline__ float c(int) const { return w.x; }
    __device__ __forceinline__ float var() const { return w.y; }
    __device__ __forceinline__ float lum() const { return w.x; }
    static __device__ __forceinline__ SvgfCell make(const float *c, float var) { return SvgfCell{make_float2(c[0], var)}; }
};
static_assert(sizeof(SvgfCell<3>) == 16 && sizeof(SvgfCell<1>) == 8, "cell layout");

/* the guide of a pixel: words {object, distance, point[3], normal[3], color[3], flags} of its rt_hit -> key, aux and (pnt not
 * NULL) pnt */
__global__ __launch_bounds__(256) void rt_svgf_pack_kernel(const uint4 *__restrict__ hits, uint4 *__restrict__ key,
                                                           uint4 *__restrict__ aux, uint4 *__restrict__ pnt, int match_color,
                                                           uint32_t n) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint4 r0 = hits[3 * (size_t)p], r1 = hits[3 * (size_t)p + 1], r2 = hits[3 * (size_t)p + 2];
    const bool dead = (int32_t)r0.x < 0 || (r2.w & (uint32_t)RT_HIT_LIGHT) != 0u;
    key[p] = match_color ? make_uint4(r0.x, r2.x, r2.y, r2.z) : make_uint4(r0.x, 0u, 0u, 0u);
    aux[p] = make_uint4(r1.y, r1.z, r1.w, (r2.w & 3u) | (dead ? kDead : 0u));
    if (pnt) pnt[p] = make_uint4(r0.z, r0.w, r1.x, 0u);
}

/* geo(p, q) of the header but for the squarings' count being a run-time one: the estimate's window */
__device__ __forceinline__ float svgf_geo(float npx, float npy, float npz, const uint4 &aq, int squarings, bool plane, float ppx,
                                          float ppy, float ppz, const uint4 &pq, float invp) {
    const float t = (npx * __uint_as_float(aq.x) + npy * __uint_as_float(aq.y)) + npz * __uint_as_float(aq.z);
    float wn = t > 0.0f ? t : 0.0f;
    for (int j = 0; j < squarings; ++j) wn = wn * wn;
    if (plane) {
        const float ex = __uint_as_float(pq.x) - ppx, ey = __uint_as_float(pq.y) - ppy, ez = __uint_as_float(pq.z) - ppz;
        const float d = (ex * npx + ey * npy) + ez * npz;
        const float u = 1.0f - (d * d) * invp;
        wn = wn * (u > 0.0f ? u : 0.0f);
    }
    return wn;
}

/* header step A and the first frame of cells: one lane a pixel.  The window is walked by the lanes with a short history only;
 * the branch around it is the wave-uniform skip. */
template <int kC>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_svgf_estimate_kernel(
    const float *__restrict__ value, const float2 *__restrict__ moments, const float *__restrict__ len,
    const uint4 *__restrict__ key, const uint4 *__restrict__ aux, const uint4 *__restrict__ pnt, SvgfCell<kC> *__restrict__ cells,
    float *__restrict__ out_estimate, int Wn, int H, int radius, int squarings, float min_history, float invp, size_t voff,
    uint32_t tiles_z) {
    const uint32_t tz = blockIdx.x % tiles_z, tx = blockIdx.x / tiles_z;
    const int64_t x64 = (int64_t)tx * kTileX + threadIdx.y, z64 = (int64_t)tz * kTileZ + threadIdx.x;
    if (x64 >= Wn || z64 >= H) return;
    const int x = (int)x64, z = (int)z64;
    const int64_t p = (int64_t)x * (int64_t)H + z;
    const uint4 ap = aux[p];
    const float2 m = moments[p];
    const float L = len[p];
    float vt = m.y - m.x * m.x;
    vt = vt > 0.0f ? vt : 0.0f;
    float var0 = vt;
    if ((ap.w & kDead) != 0u) {
        var0 = 0.0f;
    } else if (!(L >= min_history)) {
        const bool plane = pnt != nullptr;
        const uint4 kp = key[p];
        const float npx = __uint_as_float(ap.x), npy = __uint_as_float(ap.y), npz = __uint_as_float(ap.z);
        float ppx = 0.0f, ppy = 0.0f, ppz = 0.0f;
        if (plane) {
            const uint4 pp = pnt[p];
            ppx = __uint_as_float(pp.x), ppy = __uint_as_float(pp.y), ppz = __uint_as_float(pp.z);
        }
        float a1 = 0.0f, a2 = 0.0f, ws = 0.0f;
        for (int a = -radius; a <= radius; ++a) {
            const int xq = x + a;
            if (xq < 0 || xq >= Wn) continue;
            for (int b = -radius; b <= radius; ++b) {
                const int zq = z + b;
                if (zq < 0 || zq >= H) continue;
                const int64_t q = (int64_t)xq * (int64_t)H + zq;
                const uint4 kq = key[q], aq = aux[q], pq = plane ? pnt[q] : make_uint4(0u, 0u, 0u, 0u);
                const uint32_t differ = (kq.x ^ kp.x) | (kq.y ^ kp.y) | (kq.z ^ kp.z) | (kq.w ^ kp.w) | ((aq.w ^ ap.w) & 3u);
                const float w = svgf_geo(npx, npy, npz, aq, squarings, plane, ppx, ppy, ppz, pq, invp);
                if (differ == 0u && w > 0.0f) {
                    const float2 mq = moments[q];
                    a1 = a1 + w * mq.x, a2 = a2 + w * mq.y, ws = ws + w;
                }
            }
        }
        if (ws > 0.0f) {
            const float s1 = a1 / ws, s2 = a2 / ws;
            float vs = s2 - s1 * s1;
            vs = vs > 0.0f ? vs : 0.0f;
            float k = min_history / L;
            if (!(k >= 1.0f)) k = 1.0f;
            var0 = vs * k;
        }
    }
    float c[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) c[k] = value[p * kC + k];
    cells[p] = SvgfCell<kC>::make(c, var0);
    if (SvgfCell<kC>::kVarPlane) reinterpret_cast<float *>(reinterpret_cast<char *>(cells) + voff)[p] = var0;
    if (out_estimate) out_estimate[p] = var0;
}

#if RT_SVGF_ESTIMATE_LDS
/* the estimate with its window read from LDS: where any lane of the workgroup has a short history the workgroup stages the key,
 * aux, point and moments of its 4 x 64 tile and a halo of 3 -- 10 x 70 cells, 39 KiB -- and the lanes that need the window walk
 * it there.  The same arithmetic in the same order as rt_svgf_estimate_kernel. */
constexpr int kHalo = 3, kLdsX = kTileX + 2 * kHalo, kLdsZ = kTileZ + 2 * kHalo;

template <int kC>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_svgf_estimate_lds_kernel(
    const float *__restrict__ value, const float2 *__restrict__ moments, const float *__restrict__ len,
    const uint4 *__restrict__ key, const uint4 *__restrict__ aux, const uint4 *__restrict__ pnt, SvgfCell<kC> *__restrict__ cells,
    float *__restrict__ out_estimate, int Wn, int H, int radius, int squarings, float min_history, float invp, size_t voff,
    uint32_t tiles_z) {
    __shared__ uint4 s_key[kLdsX][kLdsZ], s_aux[kLdsX][kLdsZ], s_pnt[kLdsX][kLdsZ];
    __shared__ float2 s_mom[kLdsX][kLdsZ];
    const uint32_t tz = blockIdx.x % tiles_z, tx = blockIdx.x / tiles_z;
    const int64_t x0 = (int64_t)tx * kTileX, z0 = (int64_t)tz * kTileZ;
    const int64_t x64 = x0 + threadIdx.y, z64 = z0 + threadIdx.x;
    const bool mine = x64 < Wn && z64 < H;              /* (a thread without a pixel stays for the barriers) */
    const int x = (int)x64, z = (int)z64;
    const int64_t p = mine ? (int64_t)x * (int64_t)H + z : 0;
    const bool plane = pnt != nullptr;
    uint4 ap = make_uint4(0u, 0u, 0u, kDead);
    float2 m = make_float2(0.0f, 0.0f);
    float L = 0.0f;
    if (mine) ap = aux[p], m = moments[p], L = len[p];
    float vt = m.y - m.x * m.x;
    vt = vt > 0.0f ? vt : 0.0f;
    float var0 = (ap.w & kDead) != 0u ? 0.0f : vt;
    const bool need = mine && (ap.w & kDead) == 0u && !(L >= min_history);
    if (__syncthreads_or(need)) {
        for (int c = (int)(threadIdx.y * kTileZ + threadIdx.x); c < kLdsX * kLdsZ; c += kTileX * kTileZ) {
            const int i = c / kLdsZ, j = c % kLdsZ;
            const int64_t xq = x0 - kHalo + i, zq = z0 - kHalo + j;
            if (xq < 0 || xq >= Wn || zq < 0 || zq >= H) continue;
            const int64_t q = xq * (int64_t)H + zq;
            s_key[i][j] = key[q], s_aux[i][j] = aux[q], s_mom[i][j] = moments[q];
            if (plane) s_pnt[i][j] = pnt[q];
        }
        __syncthreads();
        if (need) {
            const int ci = (int)threadIdx.y + kHalo, cj = (int)threadIdx.x + kHalo;
            const uint4 kp = s_key[ci][cj];
            const float npx = __uint_as_float(ap.x), npy = __uint_as_float(ap.y), npz = __uint_as_float(ap.z);
            float ppx = 0.0f, ppy = 0.0f, ppz = 0.0f;
            if (plane) {
                const uint4 pp = s_pnt[ci][cj];
                ppx = __uint_as_float(pp.x), ppy = __uint_as_float(pp.y), ppz = __uint_as_float(pp.z);
            }
            float a1 = 0.0f, a2 = 0.0f, ws = 0.0f;
            for (int a = -radius; a <= radius; ++a) {
                const int xq = x + a;
                if (xq < 0 || xq >= Wn) continue;
                for (int b = -radius; b <= radius; ++b) {
                    const int zq = z + b;
                    if (zq < 0 || zq >= H) continue;
                    const uint4 kq = s_key[ci + a][cj + b], aq = s_aux[ci + a][cj + b];
                    const uint4 pq = plane ? s_pnt[ci + a][cj + b] : make_uint4(0u, 0u, 0u, 0u);
                    const uint32_t differ = (kq.x ^ kp.x) | (kq.y ^ kp.y) | (kq.z ^ kp.z) | (kq.w ^ kp.w) | ((aq.w ^ ap.w) & 3u);
                    const float w = svgf_geo(npx, npy, npz, aq, squarings, plane, ppx, ppy, ppz, pq, invp);
                    if (differ == 0u && w > 0.0f) {
                        const float2 mq = s_mom[ci + a][cj + b];
                        a1 = a1 + w * mq.x, a2 = a2 + w * mq.y, ws = ws + w;
                    }
                }
            }
            if (ws > 0.0f) {
                const float s1 = a1 / ws, s2 = a2 / ws;
                float vs = s2 - s1 * s1;
                vs = vs > 0.0f ? vs : 0.0f;
                float k = min_history / L;
                if (!(k >= 1.0f)) k = 1.0f;
                var0 = vs * k;
            }
        }
    }
    if (!mine) return;
    float c[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) c[k] = value[p * kC + k];
    cells[p] = SvgfCell<kC>::make(c, var0);
    if (SvgfCell<kC>::kVarPlane) reinterpret_cast<float *>(reinterpret_cast<char *>(cells) + voff)[p] = var0;
    if (out_estimate) out_estimate[p] = var0;
}
#endif

/* header step B's vf and invl of pixel (x, z): nine unit-offset taps of the variance */
template <int kC>
__device__ __forceinline__ float svgf_invl(const SvgfCell<kC> *__restrict__ in, size_t voff, int x, int z, int Wn, int H,
                                           float sl2, float epsilon) {
    constexpr float g[3] = {0.25f, 0.5f, 0.25f};
    /* the variance is a cell's last word, or the plane's */
    constexpr int kWords = SvgfCell<kC>::kVarPlane ? 1 : (int)(sizeof(SvgfCell<kC>) / sizeof(float));
    const float *var = SvgfCell<kC>::kVarPlane ? reinterpret_cast<const float *>(reinterpret_cast<const char *>(in) + voff)
                                               : reinterpret_cast<const float *>(in) + (kWords - 1);
    float gv = 0.0f, gs = 0.0f;
#pragma unroll
    for (int a = -1; a <= 1; ++a) {
#pragma unroll
        for (int b = -1; b <= 1; ++b) {
            const int xq = x + a, zq = z + b;
            if (xq < 0 || xq >= Wn || zq < 0 || zq >= H) continue;
            const int64_t q = (int64_t)xq * (int64_t)H + zq;
            gv = gv + (g[a + 1] * g[b + 1]) * var[q * kWords];
            gs = gs + g[a + 1] * g[b + 1];
        }
    }
    const float vf = gv / gs;
    return 1.0f / (sl2 * vf + epsilon);
}

/* svgf_invl of every pixel, one lane a pixel */
template <int kC>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_svgf_prefilter_kernel(const SvgfCell<kC> *__restrict__ in,
                                                                            float *__restrict__ invl, size_t voff, int Wn, int H,
                                                                            float sl2, float epsilon, uint32_t tiles_z) {
    const uint32_t tz = blockIdx.x % tiles_z, tx = blockIdx.x / tiles_z;
    const int64_t x64 = (int64_t)tx * kTileX + threadIdx.y, z64 = (int64_t)tz * kTileZ + threadIdx.x;
    if (x64 >= Wn || z64 >= H) return;
    invl[x64 * (int64_t)H + z64] = svgf_invl<kC>(in, voff, (int)x64, (int)z64, Wn, H, sl2, epsilon);
}

/* one iteration of header step B, step s = 1 << shift, over cells {value, variance}; kLum: sigma_l > 0 (invl from the
 * prefilter pass); kPlane: sigma_plane > 0 (invp = 1 / sigma_plane^2, the pnt plane); kSquarings: the normal weight's
 * squarings; last: the result goes to out_value (and out_variance, if not NULL), else to `out` as cells.
 *
 * rt_denoise_atrous_kernel's walk (its comment): a wavefront is 64 consecutive z of kPixels columns s apart, x_k = xb + k s; it
 * walks the kPixels + 4 rows r = -2 .. kPixels + 1 once, loads each row's five taps once and feeds every pixel k with
 * a = r - k in -2..2, each pixel summing its taps in the definition's order.  x, the rows and their bounds are wave-uniform; the
 * taps of a row are straight-line code, a tap that does not exist reads the lane's own row position and is dropped by a
 * select. */
template <int kC, bool kLum, bool kPlane, int kSquarings>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_svgf_atrous_kernel(
    const uint4 *__restrict__ key, const uint4 *__restrict__ aux, const uint4 *__restrict__ pnt,
    const SvgfCell<kC> *__restrict__ in, const float *__restrict__ invl, SvgfCell<kC> *__restrict__ out,
    float *__restrict__ out_value, float *__restrict__ out_variance, int Wn, int H, int shift, float invp, float sl2,
    float epsilon, int last, size_t voff, uint32_t tiles_z) {
    using Cell = SvgfCell<kC>;
    const int s = 1 << shift;
    const uint32_t tz = blockIdx.x % tiles_z, tx = blockIdx.x / tiles_z;
    /* wavefront w of the frame: column group w >> shift (kPixels s columns wide), column w & (s - 1) within the group's first s */
    const int64_t w64 = (int64_t)tx * kTileX + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int64_t xb64 = (w64 >> shift) * (int64_t)(kPixels * s) + (w64 & (s - 1));
    const int64_t z0 = (int64_t)tz * kTileZ;
    const int lane = (int)threadIdx.x;
    if (xb64 >= Wn || z0 + lane >= H) return;           /* (no barrier below: a thread without a pixel leaves) */
    const int xb = (int)xb64, z = (int)z0 + lane;
    constexpr float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    constexpr int kReach = 32;                          /* 2 s <= 32: lane offsets stay non-negative from 32 pixels before z0 */

    Cell cp[kPixels];
    uint4 kp[kPixels];
    uint32_t sp[kPixels];
    float lp[kPixels], il[kPixels], npx[kPixels], npy[kPixels], npz[kPixels], ppx[kPixels], ppy[kPixels], ppz[kPixels];
    float acc[kPixels][kC], vacc[kPixels], wsum[kPixels], vp[kPixels];
    const float *vin = reinterpret_cast<const float *>(reinterpret_cast<const char *>(in) + voff);      /* (kVarPlane only) */
    bool exists[kPixels], active[kPixels];
#pragma unroll
    for (int k = 0; k < kPixels; ++k) {
        exists[k] = xb + k * s < Wn;                    /* (wave-uniform) */
        active[k] = false;
        vacc[k] = wsum[k] = 0.0f;
#pragma unroll
        for (int c = 0; c < kC; ++c) acc[k][c] = 0.0f;
        const float zero[3] = {0.0f, 0.0f, 0.0f};
        cp[k] = Cell::make(zero, 0.0f), kp[k] = make_uint4(0u, 0u, 0u, 0u), sp[k] = 0u;
        vp[k] = lp[k] = il[k] = npx[k] = npy[k] = npz[k] = ppx[k] = ppy[k] = ppz[k] = 0.0f;
        if (exists[k]) {
            const int64_t p = (int64_t)(xb + k * s) * (int64_t)H + z;
            const uint4 ap = aux[p];
            cp[k] = in[p], kp[k] = key[p];
            vp[k] = Cell::kVarPlane ? vin[p] : cp[k].var();
            npx[k] = __uint_as_float(ap.x), npy[k] = __uint_as_float(ap.y), npz[k] = __uint_as_float(ap.z);
            sp[k] = ap.w;
            active[k] = (ap.w & kDead) == 0u;           /* (not a miss, not a light) */
            if (kLum) {
                lp[k] = cp[k].lum();
                il[k] = fused_prefilter(kC) ? svgf_invl<kC>(in, voff, xb + k * s, z, Wn, H, sl2, epsilon) : invl[p];
            }
            if (kPlane) {
                const uint4 pp = pnt[p];
                ppx[k] = __uint_as_float(pp.x), ppy[k] = __uint_as_float(pp.y), ppz[k] = __uint_as_float(pp.z);
            }
        }
    }
#pragma unroll
    for (int r = -2; r <= kPixels + 1; ++r) {
        const int xq = xb + r * s;
        if (xq < 0 || xq >= Wn) continue;               /* (wave-uniform) */
        /* the offset of pixel (xq, z0 - kReach): scalar, and only ever used with a lane offset that makes it a pixel's */
        const int64_t base = (int64_t)xq * (int64_t)H + z0 - kReach;
        const char *kb = reinterpret_cast<const char *>(key) + base * 16, *xb_ = reinterpret_cast<const char *>(aux) + base * 16,
                   *pb = reinterpret_cast<const char *>(pnt) + base * 16,
                   *cb = reinterpret_cast<const char *>(in) + base * (int64_t)sizeof(Cell),
                   *vb = reinterpret_cast<const char *>(vin) + base * 4;
#pragma unroll
        for (int b = -2; b <= 2; ++b) {
            const int zq = z + b * s;
            const bool inside = zq >= 0 && zq < H;
            const uint32_t cell = (uint32_t)((inside ? lane + b * s : lane) + kReach);
            const uint4 kq = *reinterpret_cast<const uint4 *>(kb + cell * 16u);
            const uint4 aq = *reinterpret_cast<const uint4 *>(xb_ + cell * 16u);
            const Cell cq = *reinterpret_cast<const Cell *>(cb + cell * (uint32_t)sizeof(Cell));
            uint4 pq = make_uint4(0u, 0u, 0u, 0u);
            if (kPlane) pq = *reinterpret_cast<const uint4 *>(pb + cell * 16u);
            const float lq = kLum ? cq.lum() : 0.0f;
            const float vq = Cell::kVarPlane ? *reinterpret_cast<const float *>(vb + cell * 4u) : cq.var();
#pragma unroll
            for (int k = 0; k < kPixels; ++k) {
                const int a = r - k;
                if (a < -2 || a > 2) continue;          /* (compile time) */
                const uint32_t differ = (kq.x ^ kp[k].x) | (kq.y ^ kp[k].y) | (kq.z ^ kp[k].z) | (kq.w ^ kp[k].w) |
                                        ((aq.w ^ sp[k]) & 3u);
                bool take = inside & active[k] & (differ == 0u);        /* (no short circuit: the loads stay unconditional) */
                const float t = (npx[k] * __uint_as_float(aq.x) + npy[k] * __uint_as_float(aq.y)) + npz[k] * __uint_as_float(aq.z);
                float wn = t > 0.0f ? t : 0.0f;
#pragma unroll
                for (int j = 0; j < kSquarings; ++j) wn = wn * wn;
                if (kPlane) {
                    const float ex = __uint_as_float(pq.x) - ppx[k], ey = __uint_as_float(pq.y) - ppy[k],
                                ez = __uint_as_float(pq.z) - ppz[k];
                    const float d = (ex * npx[k] + ey * npy[k]) + ez * npz[k];
                    const float u = 1.0f - (d * d) * invp;
                    wn = wn * (u > 0.0f ? u : 0.0f);
                }
                float w = (h[a + 2] * h[b + 2]) * wn;
                if (kLum) {
                    const float d = lq - lp[k];
                    const float u = 1.0f - (d * d) * il[k];
                    w = w * (u > 0.0f ? u : 0.0f);
                }
                take = take & (w > 0.0f);
#pragma unroll
                for (int c = 0; c < kC; ++c) acc[k][c] = take ? acc[k][c] + w * cq.c(c) : acc[k][c];
                vacc[k] = take ? vacc[k] + (w * w) * vq : vacc[k];
                wsum[k] = take ? wsum[k] + w : wsum[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kPixels; ++k) {
        if (!exists[k]) continue;
        const int64_t p = (int64_t)(xb + k * s) * (int64_t)H + z;
        const bool any = active[k] & (wsum[k] > 0.0f);  /* else a miss, a light or no tap: the input, bit for bit */
        float v[kC];
#pragma unroll
        for (int c = 0; c < kC; ++c) v[c] = any ? acc[k][c] / wsum[k] : cp[k].c(c);
        const float vout = any ? vacc[k] / (wsum[k] * wsum[k]) : vp[k];
        if (last) {
#pragma unroll
            for (int c = 0; c < kC; ++c) out_value[p * kC + c] = v[c];
            if (out_variance) out_variance[p] = vout;
        } else {
            out[p] = Cell::make(v, vout);
            if (Cell::kVarPlane) reinterpret_cast<float *>(reinterpret_cast<char *>(out) + voff)[p] = vout;
        }
    }
}

namespace {

/* the header's checks up to the buffers, in its order */
int check_shape(const rt_svgf_params *pr, int Wn, int H) {
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->channels != 1 && pr->channels != 3) return fail(RT_ERR_INVALID, "channels must be 1 or 3");
    if (pr->iterations < 1 || pr->iterations > 5) return fail(RT_ERR_INVALID, "iterations must be 1..5");
    if (pr->normal_squarings < 0 || pr->normal_squarings > 6) return fail(RT_ERR_INVALID, "normal_squarings must be 0..6");
    if ((pr->match_color | 1) != 1) return fail(RT_ERR_INVALID, "match_color must be 0 or 1");
    if (pr->min_history < 1 || pr->min_history > 65535) return fail(RT_ERR_INVALID, "min_history must be 1..65535");
    if (pr->spatial_radius < 1 || pr->spatial_radius > 3) return fail(RT_ERR_INVALID, "spatial_radius must be 1..3");
    if (!(pr->sigma_l >= 0.0f) || std::isinf(pr->sigma_l)) return fail(RT_ERR_INVALID, "sigma_l must be finite and >= 0");
    if (!(pr->sigma_plane >= 0.0f) || std::isinf(pr->sigma_plane)) return fail(RT_ERR_INVALID, "sigma_plane must be finite and >= 0");
    if (!(pr->epsilon > 0.0f) || std::isinf(pr->epsilon)) return fail(RT_ERR_INVALID, "epsilon must be finite and > 0");
    if (Wn <= 0 || H <= 0) return fail(RT_ERR_INVALID, "need Wn, H > 0");
    if ((double)Wn * (double)H > kMaxPixels) return fail(RT_ERR_INVALID, "rectangle too large for its values and records");
    return RT_OK;
}

/* d_scratch: key, aux, [pnt], one or two frames of cells, [invl] */
struct Scratch {
    size_t key, aux, pnt, cells[2], voff, invl, bytes;
    bool plane, lum, pass;  /* the plane term, the luminance term, the prefilter pass */
};

Scratch scratch_layout(const rt_svgf_params *pr, size_t pixels) {
    Scratch s{};
    s.plane = pr->sigma_plane > 0.0f, s.lum = pr->sigma_l > 0.0f, s.pass = s.lum && !fused_prefilter(pr->channels);
    const bool var_plane = RT_SVGF_VAR_PLANE && pr->channels == 3;       /* (a build switch: the variance behind each frame of cells) */
    s.voff = var_plane ? align256(pixels * 16) : 0;
    const size_t guide = align256(pixels * 16),
                 cells = align256(pixels * (pr->channels == 3 ? 16 : 8)) + (var_plane ? align256(pixels * 4) : 0);
    size_t at = 0;
    s.key = at, at += guide;
    s.aux = at, at += guide;
    s.pnt = at, at += s.plane ? guide : 0;
    s.cells[0] = at, at += cells;
    s.cells[1] = at, at += pr->iterations > 1 ? cells : 0;
    s.invl = at, at += s.pass ? align256(pixels * 4) : 0;
    s.bytes = at;
    return s;
}

struct Buffers {             /* the call's buffers, in device memory */
    const void *value, *hits, *moments, *len;
    void *out_value, *out_variance, *out_estimate, *scratch;
};

struct Iteration {           /* the iteration kernel's arguments */
    const uint4 *key, *aux, *pnt;
    const void *in;
    const float *invl;
    void *out;
    float *out_value, *out_variance;
    int Wn, H, shift;
    float invp, sl2, epsilon;
    int last;
    size_t voff;
    uint32_t tiles_z;
};

using Launch = void (*)(dim3, hipStream_t, const Iteration &);

template <int kC, bool kLum, bool kPlane, int kSquarings>
void launch_iteration(dim3 grid, hipStream_t stream, const Iteration &a) {
    hipLaunchKernelGGL((rt_svgf_atrous_kernel<kC, kLum, kPlane, kSquarings>), grid, dim3(kTileZ, kTileX), 0, stream, a.key, a.aux,
                       a.pnt, static_cast<const SvgfCell<kC> *>(a.in), a.invl, static_cast<SvgfCell<kC> *>(a.out), a.out_value,
                       a.out_variance, a.Wn, a.H, a.shift, a.invp, a.sl2, a.epsilon, a.last, a.voff, a.tiles_z);
}

/* the kernel of {channels, luminance term, plane term, squarings 0..6} */
#define RT_SVGF_ROW(c, l, p) {launch_iteration<c, l, p, 0>, launch_iteration<c, l, p, 1>, launch_iteration<c, l, p, 2>,          \
                              launch_iteration<c, l, p, 3>, launch_iteration<c, l, p, 4>, launch_iteration<c, l, p, 5>,          \
                              launch_iteration<c, l, p, 6>}
const Launch kLaunch[2][2][2][7] = {
    {{RT_SVGF_ROW(1, false, false), RT_SVGF_ROW(1, false, true)}, {RT_SVGF_ROW(1, true, false), RT_SVGF_ROW(1, true, true)}},
    {{RT_SVGF_ROW(3, false, false), RT_SVGF_ROW(3, false, true)}, {RT_SVGF_ROW(3, true, false), RT_SVGF_ROW(3, true, true)}}};

template <int kC>
void launch_front(dim3 grid, hipStream_t stream, const rt_svgf_params *pr, const Buffers &b, const uint4 *key, const uint4 *aux,
                  const uint4 *pnt, void *cells, int Wn, int H, float invp, size_t voff, uint32_t tiles_z) {
#if RT_SVGF_ESTIMATE_LDS
    const auto kernel = rt_svgf_estimate_lds_kernel<kC>;
#else
    const auto kernel = rt_svgf_estimate_kernel<kC>;
#endif
    hipLaunchKernelGGL(kernel, grid, dim3(kTileZ, kTileX), 0, stream, static_cast<const float *>(b.value),
                       static_cast<const float2 *>(b.moments), static_cast<const float *>(b.len), key, aux, pnt,
                       static_cast<SvgfCell<kC> *>(cells), static_cast<float *>(b.out_estimate), Wn, H, pr->spatial_radius,
                       pr->normal_squarings, (float)pr->min_history, invp, voff, tiles_z);
}

template <int kC>
void launch_prefilter(dim3 grid, hipStream_t stream, const void *cells, float *invl, size_t voff, int Wn, int H, float sl2,
                      float epsilon, uint32_t tiles_z) {
    hipLaunchKernelGGL(rt_svgf_prefilter_kernel<kC>, grid, dim3(kTileZ, kTileX), 0, stream,
                       static_cast<const SvgfCell<kC> *>(cells), invl, voff, Wn, H, sl2, epsilon, tiles_z);
}

/* the passes, enqueued on stream; every argument already checked, the device current */
int enqueue(const rt_svgf_params *pr, int Wn, int H, const Buffers &b, hipStream_t stream) {
    const size_t pixels = (size_t)Wn * (size_t)H;
    const Scratch s = scratch_layout(pr, pixels);
    char *base = static_cast<char *>(b.scratch);
    uint4 *key = reinterpret_cast<uint4 *>(base + s.key), *aux = reinterpret_cast<uint4 *>(base + s.aux);
    uint4 *pnt = s.plane ? reinterpret_cast<uint4 *>(base + s.pnt) : nullptr;
    void *cells[2] = {base + s.cells[0], base + s.cells[1]};
    float *invl = s.pass ? reinterpret_cast<float *>(base + s.invl) : nullptr;
    const float invp = s.plane ? 1.0f / (pr->sigma_plane * pr->sigma_plane) : 0.0f;
    const float sl2 = pr->sigma_l * pr->sigma_l;
    const bool three = pr->channels == 3;
    hipLaunchKernelGGL(rt_svgf_pack_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const uint4 *>(b.hits), key, aux, pnt, pr->match_color, (uint32_t)pixels);
    HIP_TRY(hipGetLastError());
    const uint32_t tiles_z = (uint32_t)((H + kTileZ - 1) / kTileZ);
    const dim3 per_pixel(tiles_z * (uint32_t)(((int64_t)Wn + kTileX - 1) / kTileX));
    three ? launch_front<3>(per_pixel, stream, pr, b, key, aux, pnt, cells[0], Wn, H, invp, s.voff, tiles_z)
          : launch_front<1>(per_pixel, stream, pr, b, key, aux, pnt, cells[0], Wn, H, invp, s.voff, tiles_z);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < pr->iterations; ++i) {
        const void *in = cells[i & 1];
        if (s.pass) {
            three ? launch_prefilter<3>(per_pixel, stream, in, invl, s.voff, Wn, H, sl2, pr->epsilon, tiles_z)
                  : launch_prefilter<1>(per_pixel, stream, in, invl, s.voff, Wn, H, sl2, pr->epsilon, tiles_z);
            HIP_TRY(hipGetLastError());
        }
        /* wavefronts across x: s for every group of kPixels s columns (the kernel's comment) */
        const int64_t waves_x = (((int64_t)Wn + (kPixels << i) - 1) / (kPixels << i)) << i;
        const dim3 grid(tiles_z * (uint32_t)((waves_x + kTileX - 1) / kTileX));
        const Iteration a{key, aux, pnt, in, invl, cells[(i + 1) & 1] /* (not written by the last iteration) */,
                          static_cast<float *>(b.out_value), static_cast<float *>(b.out_variance), Wn, H, i, invp,
                          sl2, pr->epsilon, i == pr->iterations - 1, s.voff, tiles_z};
        kLaunch[three][s.lum][s.plane][pr->normal_squarings](grid, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

} // namespace

extern "C" {

int rt_capi_svgf_version(void) { return RT_CAPI_SVGF_VERSION; }

uint64_t rt_svgf_scratch_bytes(const rt_svgf_params *pr, int Wn, int H) {
    if (check_shape(pr, Wn, H)) return 0;
    return scratch_layout(pr, (size_t)Wn * (size_t)H).bytes;
}

int rt_svgf_filter(int device, const rt_svgf_params *pr, int Wn, int H, const float *value, const rt_hit *hits, const float *moments,
                   const float *len, float *out_value, float *out_variance, float *out_estimate, double *kernel_ms) {
    int rc = check_shape(pr, Wn, H);
    if (rc) return rc;
    if (!value || !hits || !moments || !len || !out_value)
        return fail(RT_ERR_INVALID, "value / hits / moments / len / out_value is NULL");
    if ((rc = rt_internal_check_device(device))) return rc;
    const size_t pixels = (size_t)Wn * (size_t)H, cb = (size_t)pr->channels * sizeof(float);
    const HostIn in[4] = {{value, pixels * cb}, {hits, pixels * sizeof(rt_hit)}, {moments, pixels * 8}, {len, pixels * 4}};
    const HostOut out[3] = {{out_value, pixels * cb}, {out_variance, pixels * 4}, {out_estimate, pixels * 4}};
    return staged_call(device, in, 4, out, 3, scratch_layout(pr, pixels).bytes, kernel_ms,
                       [&](void *const *d_in, void *const *d_out, void *d_scratch) {
                           const Buffers b{d_in[0], d_in[1], d_in[2], d_in[3], d_out[0], d_out[1], d_out[2], d_scratch};
                           return enqueue(pr, Wn, H, b, nullptr);
                       });
}

int rt_svgf_filter_device(int device, const rt_svgf_params *pr, int Wn, int H, const void *d_value, const void *d_hits,
                          const void *d_moments, const void *d_len, void *d_out_value, void *d_out_variance, void *d_out_estimate,
                          void *d_scratch, void *hip_stream) {
    int rc = check_shape(pr, Wn, H);
    if (rc) return rc;
    if (!d_value || !d_hits || !d_moments || !d_len || !d_out_value || !d_scratch)
        return fail(RT_ERR_INVALID, "d_value / d_hits / d_moments / d_len / d_out_value / d_scratch is NULL");
    if ((((uintptr_t)d_hits | (uintptr_t)d_scratch) & 15u) != 0)
        return fail(RT_ERR_INVALID, "d_hits and d_scratch must be 16-byte aligned");
    if ((((uintptr_t)d_value | (uintptr_t)d_moments | (uintptr_t)d_len | (uintptr_t)d_out_value | (uintptr_t)d_out_variance |
          (uintptr_t)d_out_estimate) & 3u) != 0)
        return fail(RT_ERR_INVALID, "the float buffers must be 4-byte aligned");
    const size_t pixels = (size_t)Wn * (size_t)H, cb = (size_t)pr->channels * sizeof(float);
    /* the outputs and the scratch, then the inputs: none of the first four may overlap anything else */
    const void *bufs[8] = {d_out_value, d_out_variance, d_out_estimate, d_scratch, d_value, d_hits, d_moments, d_len};
    const size_t bytes[8] = {pixels * cb, pixels * 4, pixels * 4, scratch_layout(pr, pixels).bytes,
                             pixels * cb, pixels * sizeof(rt_hit), pixels * 8, pixels * 4};
    for (int o = 0; o < 4; ++o)
        for (int q = o + 1; q < 8; ++q)
            if (overlap(bufs[o], bytes[o], bufs[q], bytes[q]))
                return fail(RT_ERR_INVALID, "an output or the scratch overlaps another buffer");
    if ((rc = rt_internal_check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    const Buffers b{d_value, d_hits, d_moments, d_len, d_out_value, d_out_variance, d_out_estimate, d_scratch};
    return enqueue(pr, Wn, H, b, static_cast<hipStream_t>(hip_stream));
}

} // extern "C"
