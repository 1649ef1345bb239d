/*
 * rt_lens.hip -- implementation of include/rt_capi_lens.h: depth of field from a thin-lens camera.  The header is the
 * definition; these kernels are bit-exact to it (the library's arithmetic flags: no contraction, correctly rounded divide and
 * square root, denormals kept).
 *
 * SHAPE.  The render kernels are rt_capi.hip's: every sample is traced by its ray-batch launch, through
 * rt_internal.h -- every launch decision stays there.  Around it, here, per chunk of columns:
 *   raygen   one lane per sample: the pixel's hash, the sample's target on the focal plane and its point of the lens ->
 *            {O, T}, 24 bytes a lane, consecutive lanes consecutive rays;
 *   trace    rt_internal_launch_rays;
 *   resolve  per pixel the sequential sum of its S colours and the divide, stored once at the pixel's place.
 * Nothing is read back: the launches depend on the arguments alone, and the call never waits for the device.
 *
 * THE BATCH'S LAYOUT (RT_LENS_PLANES; measured in profiles/lens_experiments.txt, the default is what was kept).  A chunk of m
 * pixels has m S rays.
 *   list   (0)  pixel-major, KEPT: ray p S + s, one flat list (rows = n: 1 x 64 tiles of 64 / S pixels), what rt_adaptive.hip
 *               keeps for its scattered pixels; one launch a chunk; the resolve reads the samples as the consecutive words
 *               they are and sums from LDS;
 *   planes (1)  sample-major: ray s m + p, S planes of the chunk's columns x H pixels, each traced on its own with rows = H --
 *               a wavefront tile is an 8 x 8 pixel tile of ONE sample index; the resolve reads S planes, a word a lane,
 *               coalesced along z, and needs no LDS.  S launches a chunk, each of 1 / S of its rays: the trace stage
 *               measured 1.5 to 7 times the list's at 4096^2.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_capi_lens.h"
#include "rt_host.h"

#pragma clang fp contract(off)

#ifndef RT_LENS_PLANES
#define RT_LENS_PLANES 0
#endif

static_assert(sizeof(rt_lens_params) == 20 && sizeof(rt_lens_info) == 48, "rt_capi_lens.h layouts");

/* the camera as createEyeRay reads it (a named type: the ray-generation kernel is an exported symbol) */
struct RtLensCam { float so[3], ch[3], cv[3], eye[3], sw, sh, shw, shh; };

namespace {

constexpr int kBlock = 256;                            /* raygen: rays a workgroup; resolve: words (planes) */
constexpr int kResolveSamples = 1024;                  /* resolve (list): samples a workgroup -- 1024 / S pixels */
constexpr int kMaxSamples = 8;                         /* n */
constexpr size_t kChunkBytes = (size_t)256 << 20;      /* the default chunk: its rays and sample colours within 256 MiB */
constexpr long long kMaxBatchRays = 0x7fffffffLL - 64; /* rt_trace_rays' grid limit for a flat list (include/rt_capi_rays.h) */
constexpr double kMaxRayFloats = 2.0e9 * 4.0;          /* rt_render's limit for one output, in floats */

/* resolve (list): a pixel's 3 S floats in LDS, padded to an odd stride so that the sums' reads spread over the banks */
constexpr int lds_stride(int S) { return (3 * S) | 1; }
constexpr int lds_floats() {
    int most = 0;
    for (int n = 1; n <= kMaxSamples; ++n) most = std::max(most, (kResolveSamples / (n * n)) * lds_stride(n * n));
    return most;
}
static_assert(lds_floats() * 4 <= 16384, "resolve: LDS");

RtLensCam cam_of(const rt_camera_desc *cam) {
    RtLensCam c;
    for (int k = 0; k < 3; ++k) {
        c.so[k] = cam->screen_origin[k], c.ch[k] = cam->vector_horizontal[k];
        c.cv[k] = cam->vector_vertical[k], c.eye[k] = cam->eye_origin[k];
    }
    c.sw = cam->screen_width, c.sh = cam->screen_height, c.shw = cam->screen_halfwidth, c.shh = cam->screen_halfheight;
    return c;
}

} // namespace

/* the 32-bit integer hash "lowbias32" (include/rt_capi_soft.h) */
__device__ __forceinline__ uint32_t rt_lens_hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

/* Ray r of a chunk of m pixels (m S rays, r < 2^31), whose first pixel is pixel 0 of frame column xc: {O, T} of the header at
 * rays[6 r ..].  planes: r = s m + p, else r = p S + s -- either way consecutive lanes write consecutive rays.  One lane per
 * sample: the pixel's two hashes are computed by each of its S lanes, which sit in S different wavefronts (planes) or share
 * one with other pixels' (list, S no power of two for n = 3, 5, 6, 7) -- sharing them would cost more than they do. */
__global__ __launch_bounds__(kBlock) void rt_lens_raygen_kernel(RtLensCam cam, int W, int H, int n, uint32_t seed, float aperture, float g,
                                                                int xc, uint32_t m, int planes, float *__restrict__ rays) {
    const uint32_t S = (uint32_t)(n * n);
    const uint32_t r = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (r >= m * S) return;
    const uint32_t p = planes ? r % m : r / S, s = planes ? r / m : r - p * S;
    const uint32_t xl = p / (uint32_t)H;
    const int z = (int)(p - xl * (uint32_t)H), x = xc + (int)xl;
    const int i = (int)(s / (uint32_t)n), j = (int)(s - (uint32_t)i * (uint32_t)n);
    /* the target: createEyeRay's pixel point of sub-pixel (n x + i, n z + j), pushed out to the focal plane */
    const float dx_percent = ((float)(n * x + i)) / (float)(n * W);
    const float dy_percent = ((float)(n * z + j)) / (float)(n * H);
    const float scalar_x = dx_percent * cam.sw - cam.shw;
    const float scalar_y = dy_percent * cam.sh - cam.shh;
    /* the lens point: stratum (s + rot) % S, jittered by the sample's own hash */
    const uint32_t h = rt_lens_hash(rt_lens_hash(seed ^ 0x9e3779b9u) ^ ((uint32_t)x * (uint32_t)H + (uint32_t)z));
    const uint32_t sp = (s + h % S) % S;
    const uint32_t li = sp / (uint32_t)n, lj = sp - li * (uint32_t)n;
    const uint32_t hs = rt_lens_hash(h ^ s);
    const float xi1 = (float)(hs >> 8) * 0x1p-24f;
    const float xi2 = (float)(rt_lens_hash(hs ^ 0x9e3779b9u) >> 8) * 0x1p-24f;
    const float step = 2.0f / (float)n;
    const float a = ((float)li + xi1) * step - 1.0f, b = ((float)lj + xi2) * step - 1.0f;
    const float u = a * sqrtf(1.0f - (b * b) * 0.5f), v = b * sqrtf(1.0f - (a * a) * 0.5f);
    const float au = aperture * u, av = aperture * v;
    float *o = rays + 6 * (size_t)r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float pixel = cam.so[c] + cam.ch[c] * scalar_x;
        pixel = pixel + cam.cv[c] * scalar_y;
        const float along = (pixel - cam.eye[c]) * g;
        o[c] = aperture == 0.0f ? cam.eye[c] : cam.eye[c] + (cam.ch[c] * au + cam.cv[c] * av);
        o[3 + c] = pixel + along;
    }
}

/* out[p] = the average of pixel p's S sample colours, summed in their order, for the m pixels of a chunk.
 * planes: sample s of pixel p is samples[3 (s m + p) ..]; one lane per output WORD t = 3 p + c < 3 m, which reads word t of
 * each plane in turn -- every load and the store coalesced, no LDS.
 * list: sample s of pixel p is samples[3 (p S + s) ..]; a workgroup takes kResolveSamples / S pixels, reads their samples'
 * floats as the consecutive words they are into LDS (lds_stride(S) floats a pixel), then one lane per pixel and channel sums
 * its S values in order and divides -- a pixel's three lanes store its 12 bytes.
 * Either way a word of the output is stored once. */
__global__ __launch_bounds__(kBlock) void rt_lens_resolve_kernel(uint32_t m, int S, int planes, const float *__restrict__ samples,
                                                                 float *__restrict__ out) {
    __shared__ float lds[lds_floats()];
    if (planes) {
        const size_t words = 3 * (size_t)m;
        const size_t t = blockIdx.x * (size_t)kBlock + threadIdx.x;
        if (t >= words) return;
        float acc = samples[t];
        for (int s = 1; s < S; ++s) acc = acc + samples[(size_t)s * words + t];
        out[t] = acc / (float)S;
        return;
    }
    const uint32_t group = (uint32_t)kResolveSamples / (uint32_t)S;
    const uint32_t g0 = blockIdx.x * group;
    const uint32_t pixels = min(group, m - g0);                          /* (g0 < m: the grid is ceil(m / group)) */
    const uint32_t per = 3u * (uint32_t)S, stride = (uint32_t)lds_stride(S), words = pixels * per;
    const float *src = samples + (size_t)per * (size_t)g0;
    for (uint32_t i = threadIdx.x; i < words; i += (uint32_t)kBlock) {
        const uint32_t px = i / per;
        lds[px * stride + (i - px * per)] = src[i];
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < 3u * pixels; t += (uint32_t)kBlock) {
        const uint32_t px = t / 3u, c = t - 3u * px;
        const float *v = lds + px * stride + c;
        float acc = v[0];
        for (int s = 1; s < S; ++s) acc = acc + v[3 * s];
        out[3 * (size_t)(g0 + px) + c] = acc / (float)S;
    }
}

namespace {

/* the handle's scratch, which only grows, and the last call's bookkeeping */
struct RtLensState {
    Buffer rays, samples, out_rgb;                         /* (out_rgb: the host variant's output) */
    StageClock clock;                                      /* the last call's start, then per chunk rays generated, traced, resolved */
    rt_lens_info info{};
    ~RtLensState() { clock.release(); }
};

unsigned blocks_of(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

/* the header's checks (2) .. (7) */
int check_params(const rt_lens_params *pr, int W, int H) {
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->samples < 1 || pr->samples > kMaxSamples)
        return fail(RT_ERR_INVALID, "samples must be 1.." + std::to_string(kMaxSamples) + " (got " + std::to_string(pr->samples) + ")");
    if (pr->chunk_columns < 0) return fail(RT_ERR_INVALID, "chunk_columns must not be negative");
    if (!(pr->aperture >= 0.0f) || std::isinf(pr->aperture)) return fail(RT_ERR_INVALID, "aperture must be finite and >= 0");
    if (!(pr->focus > 0.0f) || std::isinf(pr->focus)) return fail(RT_ERR_INVALID, "focus must be finite and > 0");
    if ((long long)pr->samples * W > 0x7fffffffLL || (long long)pr->samples * H > 0x7fffffffLL)
        return fail(RT_ERR_INVALID, "samples * W and samples * H must stay below 2^31");
    return RT_OK;
}

/* rt_lens_rays*: the header's checks up to the device */
int check_rays_args(const rt_camera_desc *cam, int W, int H, int x0, int x1, const rt_lens_params *pr, const void *out, bool device) {
    int rc = rt_internal_check_strip(cam, W, H, x0, x1, 0, out);
    if (rc == RT_OK) rc = check_params(pr, W, H);
    if (rc) return rc;
    if ((double)(x1 - x0) * (double)H * (double)(pr->samples * pr->samples) * 6.0 > kMaxRayFloats)
        return fail(RT_ERR_INVALID, "strip too large for its rays");
    if (device && ((uintptr_t)out & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_rays must be 4-byte aligned");
    return RT_OK;
}

/* rt_render_lens*'s checks in the header's order (device: the device variant's alignment as well) */
int check_render_args(const rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                      const rt_lens_params *pr, const void *out_rgb, bool device) {
    int rc = rt_internal_check_frame(s, cam, W, H, x0, x1, max_depth, out_rgb);
    if (rc == RT_OK) rc = check_params(pr, W, H);
    if (rc) return rc;
    if ((long long)H * pr->samples * pr->samples > kMaxBatchRays)
        return fail(RT_ERR_INVALID, "one column's rays (H * samples^2) exceed a ray batch");
    if (device && ((uintptr_t)out_rgb & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_rgb must be 4-byte aligned");
    if (rt_internal_scene_soft(s))
        return fail(RT_ERR_INVALID, "the lens camera refuses a scene with area lights: a ray batch keys their shadow samples by the "
                                    "ray index (include/rt_capi_soft.h), so the frame would change with chunk_columns");
    return RT_OK;
}

/* the columns a launch traces: the caller's chunk_columns, or the default -- as many as keep the rays and the sample colours
 * (36 S bytes a pixel) within kChunkBytes, at least one -- never more than kMaxBatchRays rays' worth, nor than the strip has */
int chunk_columns(const rt_lens_params &pr, int H, int columns) {
    const long long per_column = (long long)H * pr.samples * pr.samples;            /* rays; <= kMaxBatchRays (checked) */
    long long c = pr.chunk_columns > 0 ? pr.chunk_columns : std::max<long long>(1, (long long)(kChunkBytes / 36) / per_column);
    c = std::min(c, kMaxBatchRays / per_column);
    return (int)std::min<long long>(c, columns);
}

/* the last call's stage times from its events, once: interval i is stage i % 3 of chunk i / 3 */
int collect(RtLensState *a) {
    if (a->clock.collected) return RT_OK;
    std::vector<float> t;
    const int rc = a->clock.intervals(&t);
    if (rc) return rc;
    double ms[3] = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < t.size(); ++i) ms[i % 3] += t[i];
    a->info.raygen_ms = ms[0], a->info.trace_ms = ms[1], a->info.resolve_ms = ms[2];
    return RT_OK;
}

void lens_free(void *state) { delete static_cast<RtLensState *>(state); }

double lens_ms(void *state, uint64_t seq) {
    RtLensState *a = static_cast<RtLensState *>(state);
    if (!a || a->clock.seq != seq || a->clock.n_events == 0 || collect(a) != RT_OK) return -1.0;
    return a->info.raygen_ms + a->info.trace_ms + a->info.resolve_ms;
}

RtLensState *state_of(rt_scene *s) { return unit_state<RtLensState>(s, RT_INTERNAL_UNIT_LENS, lens_free, lens_ms); }

/* the rays of m pixels from frame column xc on, into d_rays, on stream */
int enqueue_raygen(const rt_camera_desc *cam, int W, int H, const rt_lens_params &pr, int xc, uint32_t m, int planes, void *d_rays,
                   hipStream_t stream) {
    const size_t n_rays = (size_t)m * (size_t)(pr.samples * pr.samples);
    hipLaunchKernelGGL(rt_lens_raygen_kernel, dim3(blocks_of(n_rays)), dim3(kBlock), 0, stream, cam_of(cam), W, H, pr.samples, pr.seed,
                       pr.aperture, pr.focus - 1.0f, xc, m, planes, static_cast<float *>(d_rays));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

/* the call, every argument checked, the handle locked, the strip not empty: into device memory, on stream.  The events of
 * the call before are recorded anew without being waited for: its stage times, if nobody asked for them, are lost. */
int run(rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth, const rt_lens_params &pr,
        void *d_out_rgb, hipStream_t stream) {
    RtLensState *a = state_of(s);
    const int S = pr.samples * pr.samples;
    const int chunk = chunk_columns(pr, H, x1 - x0);
    const size_t most = (size_t)chunk * (size_t)H * (size_t)S;            /* rays of the largest chunk, the first */
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    int rc = a->rays.grow(most * 24);
    if (rc == RT_OK) rc = a->samples.grow(most * 12);
    /* the ray generation below writes the rays that the call before, on another stream, may not have traced yet */
    if (rc == RT_OK) rc = rt_internal_order_stream(s, stream);
    if (rc) return rc;
    a->clock.n_events = 0;
    a->clock.collected = true;
    a->info = rt_lens_info{};
    a->info.pixels = (int64_t)(x1 - x0) * H;
    if ((rc = a->clock.mark(stream))) return rc;
    for (int xc = x0; xc < x1; xc += chunk) {
        const int columns = std::min(chunk, x1 - xc);
        const uint32_t m = (uint32_t)((size_t)columns * (size_t)H);
        const int n_rays = (int)(m * (uint32_t)S);                        /* <= kMaxBatchRays */
        rc = enqueue_raygen(cam, W, H, pr, xc, m, RT_LENS_PLANES, a->rays.p, stream);
        if (rc == RT_OK) rc = a->clock.mark(stream);
        if (rc) return rc;
#if RT_LENS_PLANES
        for (int k = 0; k < S && rc == RT_OK; ++k)
            rc = rt_internal_launch_rays(s, (int)m, H, static_cast<const char *>(a->rays.p) + (size_t)k * m * 24, max_depth,
                                         static_cast<char *>(a->samples.p) + (size_t)k * m * 12, stream);
        const unsigned resolve_blocks = blocks_of(3 * (size_t)m);
#else
        rc = rt_internal_launch_rays(s, n_rays, n_rays, a->rays.p, max_depth, a->samples.p, stream);
        const unsigned resolve_blocks = (m + kResolveSamples / S - 1) / (kResolveSamples / S);
#endif
        if (rc == RT_OK) rc = a->clock.mark(stream);
        if (rc) return rc;
        hipLaunchKernelGGL(rt_lens_resolve_kernel, dim3(resolve_blocks), dim3(kBlock), 0, stream, m, S, RT_LENS_PLANES,
                           static_cast<const float *>(a->samples.p),
                           static_cast<float *>(d_out_rgb) + 3 * (size_t)(xc - x0) * (size_t)H);
        HIP_TRY(hipGetLastError());
        if ((rc = a->clock.mark(stream))) return rc;
        a->info.chunks += 1;
        a->info.rays += (int64_t)n_rays;
    }
    a->clock.collected = false;
    a->clock.seq = rt_internal_launch_seq(s);
    return RT_OK;
}

} // namespace

extern "C" {

int rt_capi_lens_version(void) { return RT_CAPI_LENS_VERSION; }

int rt_lens_rays_device(const rt_camera_desc *cam, int W, int H, int x0, int x1, const rt_lens_params *pr, int device,
                        void *d_out_rays, void *hip_stream) {
    int rc = check_rays_args(cam, W, H, x0, x1, pr, d_out_rays, true);
    if (rc == RT_OK) rc = rt_internal_check_device(device);
    if (rc || x0 == x1) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue_raygen(cam, W, H, *pr, x0, (uint32_t)((size_t)(x1 - x0) * (size_t)H), 0, d_out_rays,
                          static_cast<hipStream_t>(hip_stream));
}

int rt_lens_rays(const rt_camera_desc *cam, int W, int H, int x0, int x1, const rt_lens_params *pr, int device, float *out_rays) {
    int rc = check_rays_args(cam, W, H, x0, x1, pr, out_rays, false);
    if (rc == RT_OK) rc = rt_internal_check_device(device);
    if (rc || x0 == x1) return rc;
    const uint32_t m = (uint32_t)((size_t)(x1 - x0) * (size_t)H);
    const HostOut out[1] = {{out_rays, (size_t)m * (size_t)(pr->samples * pr->samples) * 24}};
    return staged_call(device, nullptr, 0, out, 1, 0, nullptr, [&](void *const *, void *const *d_out, void *) {
        return enqueue_raygen(cam, W, H, *pr, x0, m, 0, d_out[0], nullptr);
    });
}

int rt_render_lens_device(rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                          const rt_lens_params *pr, void *d_out_rgb, void *hip_stream) {
    const int rc = check_render_args(s, cam, W, H, x0, x1, max_depth, pr, d_out_rgb, true);
    if (rc || x0 == x1) return rc;
    const rt_lens_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    return run(s, cam, W, H, x0, x1, max_depth, p, d_out_rgb, static_cast<hipStream_t>(hip_stream));
}

int rt_render_lens(rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth, const rt_lens_params *pr,
                   float *out_rgb) {
    int rc = check_render_args(s, cam, W, H, x0, x1, max_depth, pr, out_rgb, false);
    if (rc || x0 == x1) return rc;
    const rt_lens_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    RtLensState *a = state_of(s);
    const size_t n = (size_t)(x1 - x0) * (size_t)H;
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    rc = a->out_rgb.grow(n * 12);
    if (rc == RT_OK) rc = run(s, cam, W, H, x0, x1, max_depth, p, a->out_rgb.p, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_rgb, a->out_rgb.p, n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return RT_OK;
}

int rt_get_lens_info(const rt_scene *cs, rt_lens_info *out) {
    if (!cs || !out) return fail(RT_ERR_INVALID, "scene/out is NULL");
    rt_scene *s = const_cast<rt_scene *>(cs);
    rt_internal_lock(s);
    Unlock unlock{s};
    RtLensState *a = static_cast<RtLensState *>(rt_internal_unit_slot(s, RT_INTERNAL_UNIT_LENS)->state);
    if (!a) {
        *out = rt_lens_info{};
        return RT_OK;
    }
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    const int rc = collect(a);
    if (rc) return rc;
    *out = a->info;
    return RT_OK;
}

} // extern "C"
