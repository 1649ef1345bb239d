/*
 * rt_denoise.hip -- implementation of include/rt_capi_denoise.h: the edge-avoiding a-trous filter over a frame's colours, guided
 * by its hit records.  The header is the definition; these kernels are bit-exact to it (the library's arithmetic flags: no
 * contraction, correctly rounded divide, denormals kept).
 *
 * SHAPE.  One pass packs the guide: of a 48-byte rt_hit the filter needs the object, the three albedo
 * words, the normal and whether the pixel passes through -- 32 bytes, as two 16-byte planes (key = {object, colour bits},
 * aux = {normal, pass-through}), each one 16-byte load a tap.  Then one launch per iteration: the 64 lanes of a wavefront lie
 * along z (the contiguous axis), so every tap is a coalesced load at any step, and a wavefront filters kPixels columns one step
 * apart, whose windows share their rows (the kernel's comment).  Between iterations the colours travel as {r, g, b, lum} -- one
 * 16-byte load a tap and the luminance computed once a pixel, by the iteration that wrote it -- in two frames of scratch; the
 * last iteration writes d_out_rgb, and d_rgb is only read (by the pack).
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/rt_capi_denoise.h"
#include "rt_host.h"

static_assert(sizeof(rt_hit) == 48, "rt_hit layout");
static_assert(sizeof(rt_denoise_params) == 12, "rt_denoise_params layout");

namespace {

constexpr int kTileZ = 64, kTileX = 4;                 /* a workgroup: 4 wavefronts, each 64 consecutive z */
constexpr int kPixels = 8;                             /* the columns, one step apart, a wavefront filters together */
constexpr double kMaxPixels = 2.0e9 * 4.0 * 4.0 / 60.0; /* rt_render_gbuffer's limit: 3.2e10 bytes of colours and records */

} // namespace

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.25f * r + 0.5f * g) + 0.25f * b; }

/* the guide of a pixel: words {object, distance, point[3], normal[3], color[3], flags} of its rt_hit -> key and aux; its colour
 * with the luminance the colour term compares -> col */
__global__ __launch_bounds__(256) void rt_denoise_pack_kernel(const uint4 *__restrict__ hits, const float *__restrict__ rgb,
                                                              uint4 *__restrict__ key, uint4 *__restrict__ aux,
                                                              float4 *__restrict__ col, uint32_t n) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint4 r0 = hits[3 * (size_t)p], r1 = hits[3 * (size_t)p + 1], r2 = hits[3 * (size_t)p + 2];
    const bool pass = (int32_t)r0.x < 0 || (r2.w & (uint32_t)RT_HIT_LIGHT) != 0u;
    key[p] = make_uint4(r0.x, r2.x, r2.y, r2.z);
    aux[p] = make_uint4(r1.y, r1.z, r1.w, pass ? 1u : 0u);
    const float r = rgb[3 * (size_t)p], g = rgb[3 * (size_t)p + 1], b = rgb[3 * (size_t)p + 2];
    col[p] = make_float4(r, g, b, lum(r, g, b));
}

/* one iteration of the definition, step s = 1 << shift, over colours {r, g, b, lum}; kColor: sigma_color > 0 (inv = 1 /
 * (sigma_color 2^-i)^2); kLast: the result goes to out_rgb, 12 bytes a pixel, else to out with its luminance for the next
 * iteration; kSquarings: the normal weight's squarings.
 *
 * A wavefront is 64 consecutive z of kPixels columns s apart, x_k = xb + k s: their 5 x 5 windows share rows -- x_k + a s is row
 * xb + (k + a) s -- so the wavefront walks the kPixels + 4 rows r = -2 .. kPixels + 1 once, loads each row's five taps once and
 * feeds every pixel k with a = r - k in -2..2: 7.5 tap loads a pixel instead of 25, at any step, and each pixel still sums its
 * taps in the definition's order (a ascending with r, b ascending within the row).  x, the rows and their bounds are
 * wave-uniform, so a tap's address is a scalar base plus a lane offset.  The taps of a row are straight-line code -- a tap that
 * does not exist reads the lane's own row position instead and is dropped by a select, like a tap of another key or of no weight
 * -- so that a row's loads are in flight together; a skip written as a branch serialises the memory latencies (DESIGN.md
 * section 16). */
template <bool kColor, bool kLast, int kSquarings>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_denoise_atrous_kernel(const uint4 *__restrict__ key,
                                                                           const uint4 *__restrict__ aux,
                                                                           const float4 *__restrict__ in, float4 *__restrict__ out,
                                                                           float *__restrict__ out_rgb, int Wn, int H, int shift,
                                                                           float inv, uint32_t tiles_z) {
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

    float4 cp[kPixels];
    uint4 kp[kPixels];
    float npx[kPixels], npy[kPixels], npz[kPixels], ar[kPixels], ag[kPixels], ab[kPixels], wsum[kPixels];
    bool exists[kPixels], active[kPixels];
#pragma unroll
    for (int k = 0; k < kPixels; ++k) {
        exists[k] = xb + k * s < Wn;                    /* (wave-uniform) */
        active[k] = false;
        ar[k] = ag[k] = ab[k] = wsum[k] = 0.0f;
        cp[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f), kp[k] = make_uint4(0u, 0u, 0u, 0u), npx[k] = npy[k] = npz[k] = 0.0f;
        if (exists[k]) {
            const int64_t p = (int64_t)(xb + k * s) * (int64_t)H + z;
            const uint4 ap = aux[p];
            cp[k] = in[p], kp[k] = key[p];
            npx[k] = __uint_as_float(ap.x), npy[k] = __uint_as_float(ap.y), npz[k] = __uint_as_float(ap.z);
            active[k] = ap.w == 0u;                     /* (not a miss, not a light) */
        }
    }
#pragma unroll
    for (int r = -2; r <= kPixels + 1; ++r) {
        const int xq = xb + r * s;
        if (xq < 0 || xq >= Wn) continue;               /* (wave-uniform) */
        /* the byte offset of pixel (xq, z0 - kReach): scalar, and only ever used with a lane offset that makes it a pixel's */
        const int64_t base = ((int64_t)xq * (int64_t)H + z0 - kReach) * 16;
        const char *kb = reinterpret_cast<const char *>(key) + base, *xb_ = reinterpret_cast<const char *>(aux) + base,
                   *cb = reinterpret_cast<const char *>(in) + base;
#pragma unroll
        for (int b = -2; b <= 2; ++b) {
            const int zq = z + b * s;
            const bool inside = zq >= 0 && zq < H;
            const uint32_t off = (uint32_t)((inside ? lane + b * s : lane) + kReach) * 16u;
            const uint4 kq = *reinterpret_cast<const uint4 *>(kb + off);
            const uint4 aq = *reinterpret_cast<const uint4 *>(xb_ + off);
            const float4 cq = *reinterpret_cast<const float4 *>(cb + off);
#pragma unroll
            for (int k = 0; k < kPixels; ++k) {
                const int a = r - k;
                if (a < -2 || a > 2) continue;          /* (compile time) */
                const uint32_t differ = (kq.x ^ kp[k].x) | (kq.y ^ kp[k].y) | (kq.z ^ kp[k].z) | (kq.w ^ kp[k].w);
                bool take = inside & active[k] & (differ == 0u);        /* (no short circuit: the loads stay unconditional) */
                const float t = (npx[k] * __uint_as_float(aq.x) + npy[k] * __uint_as_float(aq.y)) + npz[k] * __uint_as_float(aq.z);
                float wn = t > 0.0f ? t : 0.0f;
#pragma unroll
                for (int j = 0; j < kSquarings; ++j) wn = wn * wn;
                float w = (h[a + 2] * h[b + 2]) * wn;
                if (kColor) {
                    const float d = cq.w - cp[k].w;
                    const float u = 1.0f - (d * d) * inv;
                    w = w * (u > 0.0f ? u : 0.0f);
                }
                take = take & (w > 0.0f);
                ar[k] = take ? ar[k] + w * cq.x : ar[k], ag[k] = take ? ag[k] + w * cq.y : ag[k];
                ab[k] = take ? ab[k] + w * cq.z : ab[k], wsum[k] = take ? wsum[k] + w : wsum[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kPixels; ++k) {
        if (!exists[k]) continue;
        const int64_t p = (int64_t)(xb + k * s) * (int64_t)H + z;
        const bool any = active[k] & (wsum[k] > 0.0f);  /* else a miss, a light or no tap: the input, bit for bit */
        const float r = any ? ar[k] / wsum[k] : cp[k].x, g = any ? ag[k] / wsum[k] : cp[k].y, bl = any ? ab[k] / wsum[k] : cp[k].z;
        if (kLast) {
            float *o = out_rgb + 3 * p;
            o[0] = r, o[1] = g, o[2] = bl;
        } else {
            out[p] = make_float4(r, g, bl, any ? lum(r, g, bl) : cp[k].w);
        }
    }
}

namespace {

/* the header's checks up to the buffers, in its order */
int check_shape(const rt_denoise_params *pr, int Wn, int H) {
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->iterations < 1 || pr->iterations > 5) return fail(RT_ERR_INVALID, "iterations must be 1..5");
    if (pr->normal_squarings < 0 || pr->normal_squarings > 6) return fail(RT_ERR_INVALID, "normal_squarings must be 0..6");
    if (!(pr->sigma_color >= 0.0f) || std::isinf(pr->sigma_color))
        return fail(RT_ERR_INVALID, "sigma_color must be finite and >= 0");
    if (Wn <= 0 || H <= 0) return fail(RT_ERR_INVALID, "need Wn, H > 0");
    if ((double)Wn * (double)H > kMaxPixels) return fail(RT_ERR_INVALID, "rectangle too large for its colours and records");
    return RT_OK;
}

/* d_scratch: the guide's two planes, then one or two frames of {r, g, b, lum} */
size_t scratch_bytes(const rt_denoise_params *pr, size_t pixels) {
    return align256(pixels * 16) * (pr->iterations > 1 ? 4 : 3);
}

using Launch = void (*)(dim3, hipStream_t, const uint4 *, const uint4 *, const float4 *, float4 *, float *, int, int, int, float,
                        uint32_t);

template <bool kColor, bool kLast, int kSquarings>
void launch_iteration(dim3 grid, hipStream_t stream, const uint4 *key, const uint4 *aux, const float4 *in, float4 *out,
                      float *out_rgb, int Wn, int H, int s, float inv, uint32_t tiles_z) {
    hipLaunchKernelGGL((rt_denoise_atrous_kernel<kColor, kLast, kSquarings>), grid, dim3(kTileZ, kTileX), 0, stream, key, aux, in,
                       out, out_rgb, Wn, H, s, inv, tiles_z);
}

/* the kernel of {colour term, last iteration, squarings 0..6} */
#define RT_DENOISE_ROW(c, l) {launch_iteration<c, l, 0>, launch_iteration<c, l, 1>, launch_iteration<c, l, 2>,                  \
                              launch_iteration<c, l, 3>, launch_iteration<c, l, 4>, launch_iteration<c, l, 5>,                  \
                              launch_iteration<c, l, 6>}
const Launch kLaunch[2][2][7] = {{RT_DENOISE_ROW(false, false), RT_DENOISE_ROW(false, true)},
                                 {RT_DENOISE_ROW(true, false), RT_DENOISE_ROW(true, true)}};

/* the pack and the iterations, enqueued on stream; every argument already checked, the device current */
int enqueue(const rt_denoise_params *pr, int Wn, int H, const void *d_rgb, const void *d_hits, void *d_out, void *d_scratch,
            hipStream_t stream) {
    const size_t pixels = (size_t)Wn * (size_t)H, plane = align256(pixels * 16);
    char *base = static_cast<char *>(d_scratch);
    uint4 *key = reinterpret_cast<uint4 *>(base), *aux = reinterpret_cast<uint4 *>(base + plane);
    float4 *col[2] = {reinterpret_cast<float4 *>(base + 2 * plane), reinterpret_cast<float4 *>(base + 3 * plane)};
    hipLaunchKernelGGL(rt_denoise_pack_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const uint4 *>(d_hits), static_cast<const float *>(d_rgb), key, aux, col[0], (uint32_t)pixels);
    HIP_TRY(hipGetLastError());
    const uint32_t tiles_z = (uint32_t)((H + kTileZ - 1) / kTileZ);
    const bool colour = pr->sigma_color > 0.0f;
    for (int i = 0; i < pr->iterations; ++i) {
        const bool last = i == pr->iterations - 1;
        /* wavefronts across x: s for every group of kPixels s columns (the kernel's comment) */
        const int64_t waves_x = (((int64_t)Wn + (kPixels << i) - 1) / (kPixels << i)) << i;
        const dim3 grid(tiles_z * (uint32_t)((waves_x + kTileX - 1) / kTileX));
        const float sc = pr->sigma_color * (1.0f / (float)(1 << i));
        const float inv = colour ? 1.0f / (sc * sc) : 0.0f;
        const float4 *in = col[i & 1];
        float4 *out = col[(i + 1) & 1];                  /* (not written by the last iteration) */
        kLaunch[colour][last][pr->normal_squarings](grid, stream, key, aux, in, out, static_cast<float *>(d_out), Wn, H, i, inv,
                                                    tiles_z);
        HIP_TRY(hipGetLastError());
    }
    return RT_OK;
}

} // namespace

extern "C" {

int rt_capi_denoise_version(void) { return RT_CAPI_DENOISE_VERSION; }

uint64_t rt_denoise_scratch_bytes(const rt_denoise_params *pr, int Wn, int H) {
    if (check_shape(pr, Wn, H)) return 0;
    return scratch_bytes(pr, (size_t)Wn * (size_t)H);
}

int rt_denoise(int device, const rt_denoise_params *pr, int Wn, int H, const float *rgb, const rt_hit *hits, float *out_rgb,
               double *kernel_ms) {
    int rc = check_shape(pr, Wn, H);
    if (rc) return rc;
    if (!rgb || !hits || !out_rgb) return fail(RT_ERR_INVALID, "rgb / hits / out_rgb is NULL");
    if ((rc = rt_internal_check_device(device))) return rc;
    const size_t pixels = (size_t)Wn * (size_t)H;
    const HostIn in[2] = {{rgb, pixels * 12}, {hits, pixels * sizeof(rt_hit)}};
    const HostOut out[1] = {{out_rgb, pixels * 12}};
    return staged_call(device, in, 2, out, 1, scratch_bytes(pr, pixels), kernel_ms,
                       [&](void *const *d_in, void *const *d_out, void *d_scratch) {
                           return enqueue(pr, Wn, H, d_in[0], d_in[1], d_out[0], d_scratch, nullptr);
                       });
}

int rt_denoise_device(int device, const rt_denoise_params *pr, int Wn, int H, const void *d_rgb, const void *d_hits,
                      void *d_out_rgb, void *d_scratch, void *hip_stream) {
    int rc = check_shape(pr, Wn, H);
    if (rc) return rc;
    if (!d_rgb || !d_hits || !d_out_rgb || !d_scratch)
        return fail(RT_ERR_INVALID, "d_rgb / d_hits / d_out_rgb / d_scratch is NULL");
    if (((uintptr_t)d_hits & 15u) != 0 || ((uintptr_t)d_scratch & 15u) != 0)
        return fail(RT_ERR_INVALID, "d_hits and d_scratch must be 16-byte aligned");
    if (((uintptr_t)d_rgb & 3u) != 0 || ((uintptr_t)d_out_rgb & 3u) != 0)
        return fail(RT_ERR_INVALID, "d_rgb and d_out_rgb must be 4-byte aligned");
    const size_t bytes = (size_t)Wn * (size_t)H * 12;
    if (overlap(d_rgb, bytes, d_out_rgb, bytes)) return fail(RT_ERR_INVALID, "d_out_rgb overlaps d_rgb");
    if ((rc = rt_internal_check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue(pr, Wn, H, d_rgb, d_hits, d_out_rgb, d_scratch, static_cast<hipStream_t>(hip_stream));
}

} // extern "C"
