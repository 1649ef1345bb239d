/*
 * rt_adaptive.hip -- implementation of include/rt_capi_adaptive.h: supersampling for the pixels an edge passes through and
 * for no others.  The header is the definition; these kernels are bit-exact to it (the library's arithmetic flags: no
 * contraction, correctly rounded divide, denormals kept).
 *
 * SHAPE.  The render kernels are rt_capi.hip's: the first pass is its G-buffer launch, the second
 * its ray-batch launches, both through rt_internal.h -- every launch decision stays there.  Between them, here:
 *   flag     one lane per pixel, z (the contiguous axis) along the wavefront: the pixel's colour, object and normal and those
 *            of the three other corners of its footprint (two of them the next lane's loads) -> one byte, the first pass's
 *            colour copied to the output unless it was rendered there, and per workgroup the number of flagged pixels (a
 *            ballot and a population count per wavefront);
 *   scan     the exclusive scan of the workgroups' counts in two small kernels -- groups of 1024 counts each on their own,
 *            then the groups' sums -- and the total;
 *   list     each flagged pixel's number at offset[workgroup] + its rank in the workgroup: the list is in pixel order, so
 *            the launches are deterministic and neighbouring pixels' rays share a wavefront tile;
 *   -- the host reads the total (the call's one synchronisation) --
 *   raygen   per chunk of the list, one lane per sample: {eye, pixel point} in createEyeRay's arithmetic, a pixel's k x k
 *            samples contiguous in the batch, which is then traced as a flat list (rows = n: 1 x 64 tiles of 64 / k^2 pixels);
 *   resolve  per flagged pixel the sequential sum of its k x k colours and the divide, stored at the pixel's place; the
 *            samples are read as the consecutive words they are and summed from LDS.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_capi_adaptive.h"
#include "rt_host.h"

#pragma clang fp contract(off)

/* Build switches (speed only; measured in profiles/adaptive_experiments.txt, the defaults are what was kept):
 * RT_ADAPTIVE_ROWS          the rows of the second pass's ray batches: 0 = a flat list (rows = n, 1 x 64 tiles of consecutive
 *                           rays: 64 / k^2 listed pixels a wavefront), r > 0 = an n / r x r grid tiled like an image;
 * RT_ADAPTIVE_DIRECT_FIRST  1: a strip without a halo column (x1 = W) renders its first pass's colours straight into the
 *                           output and the flag kernel copies nothing; 0: always into scratch, copied by the flag kernel. */
#ifndef RT_ADAPTIVE_ROWS
#define RT_ADAPTIVE_ROWS 0
#endif
#ifndef RT_ADAPTIVE_DIRECT_FIRST
#define RT_ADAPTIVE_DIRECT_FIRST 1
#endif

static_assert(sizeof(rt_hit) == 48, "rt_hit layout");
static_assert(sizeof(rt_adaptive_params) == 20 && sizeof(rt_adaptive_info) == 64, "rt_capi_adaptive.h layouts");

namespace {

constexpr int kBlock = 256;                            /* flag, list, raygen, resolve: pixels (or rays) a workgroup */
constexpr int kScanBlock = 1024;
constexpr int kResolveSamples = 1024;                  /* resolve: samples a workgroup: 256 listed pixels with k = 2, 64 with k = 4 */
static_assert((kResolveSamples / 16) * (3 * 16 + 1) <= (kResolveSamples / 4) * (3 * 4 + 1), "resolve: LDS sized by k = 2");
constexpr long long kMaxRectPixels = 533333333;        /* rt_render_gbuffer's limit: 3.2e10 bytes of colours and records */
constexpr size_t kChunkBytes = (size_t)256 << 20;      /* the default chunk: its rays and sample colours within 256 MiB */
constexpr int kMaxChunk = 1 << 26;                     /* pixels a launch at most: 2^30 rays with k = 4 */

/* the camera as createEyeRay reads it */
struct Cam { float so[3], ch[3], cv[3], eye[3], sw, sh, shw, shh; };

} // namespace

/* what the flag test reads of a pixel: its record's object and normal (words 0 and 5..7 of the 48 bytes, as the first two of
 * its three 16-byte quads) and its colour */
struct RtAdaptivePixel { int obj; float nx, ny, nz, r, g, b; };

__device__ __forceinline__ RtAdaptivePixel rt_adaptive_load(const float *__restrict__ rgb, const uint4 *__restrict__ hits, size_t q) {
    const uint4 h0 = hits[3 * q], h1 = hits[3 * q + 1];
    RtAdaptivePixel v;
    v.obj = (int)h0.x;
    v.nx = __uint_as_float(h1.y), v.ny = __uint_as_float(h1.z), v.nz = __uint_as_float(h1.w);
    v.r = rgb[3 * q], v.g = rgb[3 * q + 1], v.b = rgb[3 * q + 2];
    return v;
}

/* the next lane's pixel (the last lane's own) */
__device__ __forceinline__ RtAdaptivePixel rt_adaptive_next_lane(const RtAdaptivePixel v) {
    RtAdaptivePixel w;
    w.obj = __shfl_down(v.obj, 1u, 64);
    w.nx = __shfl_down(v.nx, 1u, 64), w.ny = __shfl_down(v.ny, 1u, 64), w.nz = __shfl_down(v.nz, 1u, 64);
    w.r = __shfl_down(v.r, 1u, 64), w.g = __shfl_down(v.g, 1u, 64), w.b = __shfl_down(v.b, 1u, 64);
    return w;
}

/* differ(p, q) of the header */
__device__ __forceinline__ bool rt_adaptive_differ(const RtAdaptivePixel p, const RtAdaptivePixel q, float thr, float cosn) {
    const float t = (p.nx * q.nx + p.ny * q.ny) + p.nz * q.nz;
    bool d = p.obj != q.obj;
    d |= (p.obj >= 0) & !(t >= cosn);
    d |= !(fabsf(p.r - q.r) <= thr) || !(fabsf(p.g - q.g) <= thr) || !(fabsf(p.b - q.b) <= thr);
    return d;
}

/* FLAGS of the first Wn columns of a Wh x H rectangle (Wh = Wn, or Wn + 1: the halo column), n = Wn H pixels.  flags2 (or
 * NULL): a second copy of the bytes, the caller's; copy_rgb (or NULL): the pixels' colours, copied; counts (or NULL): the
 * workgroup's number of flagged pixels.
 * A lane loads its own pixel and the one beside it in the next column, (x+1, z); the two corners above them, (x, z+1) and
 * (x+1, z+1), are what the NEXT lane has loaded -- z is the lanes' axis -- and come by a lane shift: two pixels loaded per pixel
 * flagged instead of four, each as two 16-byte loads of its record and three words of colour.  Only a wavefront's last lane
 * has no next lane and loads its upper corners itself. */
__global__ __launch_bounds__(kBlock) void rt_adaptive_flag_kernel(const float *__restrict__ rgb, const uint4 *__restrict__ hits,
                                                                  int Wh, int H, int flag_all, float thr, float cosn,
                                                                  uint8_t *__restrict__ flags, uint8_t *__restrict__ flags2,
                                                                  float *__restrict__ copy_rgb, uint32_t *__restrict__ counts,
                                                                  uint32_t n) {
    __shared__ uint32_t wave_count[kBlock / 64];
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const bool inside = p < n;
    const size_t P = inside ? p : n - 1u;                /* (lanes past the end read the last pixel and write nothing) */
    const uint32_t x = (uint32_t)P / (uint32_t)H, z = (uint32_t)P - x * (uint32_t)H;
    const bool right = x + 1u < (uint32_t)Wh, up = z + 1u < (uint32_t)H;
    const RtAdaptivePixel own = rt_adaptive_load(rgb, hits, P);
    const RtAdaptivePixel beside = right ? rt_adaptive_load(rgb, hits, P + (size_t)H) : own;
    RtAdaptivePixel above = rt_adaptive_next_lane(own), diagonal = rt_adaptive_next_lane(beside);
    if ((threadIdx.x & 63u) == 63u) {                    /* (no next lane) */
        if (up) above = rt_adaptive_load(rgb, hits, P + 1);
        if (up && right) diagonal = rt_adaptive_load(rgb, hits, P + (size_t)H + 1);
    }
    bool f = flag_all != 0;
    if (right) f |= rt_adaptive_differ(own, beside, thr, cosn);
    if (up) f |= rt_adaptive_differ(own, above, thr, cosn);
    if (right && up) f |= rt_adaptive_differ(own, diagonal, thr, cosn);
    f = f && inside;
    if (inside) {
        if (copy_rgb) copy_rgb[3 * P] = own.r, copy_rgb[3 * P + 1] = own.g, copy_rgb[3 * P + 2] = own.b;
        flags[P] = f ? 1 : 0;
        if (flags2) flags2[P] = f ? 1 : 0;
    }
    if (counts) {                                       /* (uniform) */
        const unsigned long long ballot = __ballot(f);
        if ((threadIdx.x & 63u) == 0u) wave_count[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
        __syncthreads();
        if (threadIdx.x == 0u) {
            uint32_t c = 0;
            for (int k = 0; k < kBlock / 64; ++k) c += wave_count[k];
            counts[blockIdx.x] = c;
        }
    }
}

/* The exclusive scan of the flag kernel's counts, in two small kernels.  Both scan kScanBlock values a step: a wavefront's
 * inclusive scan by lane shifts, the wavefronts' sums through LDS.
 * Level 1: workgroup b scans counts[b kScanBlock ..) on its own -- offsets[i] = the sum of the group's counts before i -- and
 * writes the group's sum to group_sums[b]. */
__device__ __forceinline__ uint32_t rt_adaptive_scan_step(uint32_t v, uint32_t *wave_sum, uint32_t *all) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, (unsigned)d, 64);
        if (lane >= (uint32_t)d) incl += up;
    }
    if (lane == 63u) wave_sum[w] = incl;
    __syncthreads();
    uint32_t before = 0, sum = 0;
    for (uint32_t k = 0; k < (uint32_t)(kScanBlock / 64); ++k) {
        const uint32_t c = wave_sum[k];
        before += k < w ? c : 0u;
        sum += c;
    }
    __syncthreads();                                    /* (wave_sum is written again by the next step) */
    *all = sum;
    return before + (incl - v);
}

__global__ __launch_bounds__(kScanBlock) void rt_adaptive_scan_groups_kernel(const uint32_t *__restrict__ counts,
                                                                             uint32_t *__restrict__ offsets, uint32_t n_blocks,
                                                                             uint32_t *__restrict__ group_sums) {
    __shared__ uint32_t wave_sum[kScanBlock / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kScanBlock + threadIdx.x;
    uint32_t all = 0;
    const uint32_t at = rt_adaptive_scan_step(i < n_blocks ? counts[i] : 0u, wave_sum, &all);
    if (i < n_blocks) offsets[i] = at;
    if (threadIdx.x == 0u) group_sums[blockIdx.x] = all;
}

/* Level 2: one workgroup walks the groups' sums kScanBlock at a time -- group_base[g] = the sum of the groups before g -- and
 * writes the total (a frame of 2^28 pixels has 1024 groups: one step) */
__global__ __launch_bounds__(kScanBlock) void rt_adaptive_scan_kernel(const uint32_t *__restrict__ group_sums,
                                                                      uint32_t *__restrict__ group_base, uint32_t n_groups,
                                                                      uint32_t *__restrict__ total) {
    __shared__ uint32_t wave_sum[kScanBlock / 64];
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < n_groups; i0 += (uint32_t)kScanBlock) {
        const uint32_t i = i0 + threadIdx.x;
        uint32_t all = 0;
        const uint32_t at = rt_adaptive_scan_step(i < n_groups ? group_sums[i] : 0u, wave_sum, &all);
        if (i < n_groups) group_base[i] = base + at;
        base += all;
    }
    if (threadIdx.x == 0u) *total = base;
}

/* the flagged pixels' numbers, in pixel order: the flag kernel's workgroups again, workgroup b's first at
 * group_base[b / kScanBlock] + offsets[b] */
__global__ __launch_bounds__(kBlock) void rt_adaptive_list_kernel(const uint8_t *__restrict__ flags, const uint32_t *__restrict__ offsets,
                                                                  const uint32_t *__restrict__ group_base,
                                                                  uint32_t *__restrict__ list, uint32_t n) {
    __shared__ uint32_t wave_count[kBlock / 64];
    const uint32_t p = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const bool f = p < n && flags[p] != 0;
    const unsigned long long ballot = __ballot(f);
    if (lane == 0u) wave_count[w] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t at = group_base[blockIdx.x / (uint32_t)kScanBlock] + offsets[blockIdx.x];
    for (uint32_t k = 0; k < w; ++k) at += wave_count[k];
    at += (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    if (f) list[at] = p;
}

/* the k x k rays {E, T} of m listed pixels, ray (g << 2 kl) + i k + j sample (i, j) of list[g]: the pixel point of
 * Camera::createEyeRay (src/Camera.cpp:71-84) at dx = (float)(k x + i) / (float)(k W), dz = (float)(k z + j) / (float)(k H), as
 * the supersampling kernels build it for pixel (k x + i, k z + j) of the virtual image */
__global__ __launch_bounds__(kBlock) void rt_adaptive_raygen_kernel(const uint32_t *__restrict__ list, uint32_t m, int kl, Cam cam,
                                                                    int W, int H, int x0, float *__restrict__ rays) {
    const uint32_t r = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (r >= (m << (2 * kl))) return;
    const uint32_t g = r >> (2 * kl), s = r & ((1u << (2 * kl)) - 1u);
    const int i = (int)(s >> kl), j = (int)(s & ((1u << kl) - 1u));
    const uint32_t p = list[g];
    const uint32_t xl = p / (uint32_t)H;
    const int z = (int)(p - xl * (uint32_t)H), x = x0 + (int)xl;
    const float dx_percent = ((float)((x << kl) + i)) / (float)(W << kl);
    const float dy_percent = ((float)((z << kl) + j)) / (float)(H << kl);
    const float scalar_x = dx_percent * cam.sw - cam.shw;
    const float scalar_y = dy_percent * cam.sh - cam.shh;
    float *o = rays + 6 * (size_t)r;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float pixel = cam.so[c] + cam.ch[c] * scalar_x;
        pixel = pixel + cam.cv[c] * scalar_y;
        o[c] = cam.eye[c];
        o[3 + c] = pixel;
    }
}

/* out[list[g]] = the average of the listed pixel's kk sample colours, summed in their order (include/rt_capi_ssaa.h).  A
 * workgroup takes kResolveSamples / kk listed pixels: their samples' floats are consecutive in `samples` and are read as
 * such, a word a lane, into LDS (a pixel's 3 kk floats and one of padding, so that the sums' reads spread over the banks);
 * then one lane per pixel and channel sums its kk values in order and divides -- a pixel's three lanes store its 12 bytes. */
__global__ __launch_bounds__(kBlock) void rt_adaptive_resolve_kernel(const uint32_t *__restrict__ list, uint32_t m, int kk,
                                                                     const float *__restrict__ samples, float *__restrict__ out) {
    __shared__ float lds[(kResolveSamples / 4) * (3 * 4 + 1)];           /* (k = 2 needs the most: 256 pixels of 13 floats) */
    const uint32_t group = (uint32_t)kResolveSamples / (uint32_t)kk;
    const uint32_t g0 = blockIdx.x * group;
    const uint32_t pixels = min(group, m - g0);                          /* (g0 < m: the grid is ceil(m / group)) */
    const uint32_t per = 3u * (uint32_t)kk, words = pixels * per;
    const float *src = samples + (size_t)per * (size_t)g0;
    for (uint32_t i = threadIdx.x; i < words; i += (uint32_t)kBlock) {
        const uint32_t px = i / per;
        lds[px * (per + 1u) + (i - px * per)] = src[i];
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < 3u * pixels; t += (uint32_t)kBlock) {
        const uint32_t px = t / 3u, c = t - 3u * px;
        const float *v = lds + px * (per + 1u) + c;
        float acc = v[0];
        for (int s = 1; s < kk; ++s) acc = acc + v[3 * s];
        out[3 * (size_t)list[g0 + px] + c] = acc / (float)kk;
    }
}

/* the unit's place in the handle (rt_internal.h): how its state is freed, and its last call's stage times (named symbols: the
 * host-side program scripts/asan_adaptive_host.hip calls them) */
extern "C" void rt_internal_adaptive_free(void *state);
extern "C" double rt_internal_adaptive_ms(void *state, uint64_t seq);

namespace {

/* the handle's scratch, which only grows, and the last call's bookkeeping */
struct RtAdaptiveState {
    Buffer first_rgb, first_hits, flags, counts, list, rays, samples, out_rgb, out_flags;   /* (out_*: the host variant's outputs) */
    uint32_t *d_total = nullptr, *h_total = nullptr;     /* the number of flagged pixels: on the device, and pinned */
    /* the last call's start, first pass done, flags and list done; second pass begun, then per chunk traced, resolved */
    StageClock clock;
    rt_adaptive_info info{};
    ~RtAdaptiveState() {
        clock.release();
        if (d_total) (void)hipFree(d_total);
        if (h_total) (void)hipHostFree(h_total);
    }
};

/* the header's checks of the params, in its order */
int check_params(const rt_adaptive_params *pr) {
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->samples != 1 && pr->samples != 2 && pr->samples != 4)
        return fail(RT_ERR_INVALID, "samples must be 1, 2 or 4 (got " + std::to_string(pr->samples) + ")");
    if (pr->flag_all != 0 && pr->flag_all != 1) return fail(RT_ERR_INVALID, "flag_all must be 0 or 1");
    if (pr->chunk_pixels < 0) return fail(RT_ERR_INVALID, "chunk_pixels must not be negative");
    if (!(pr->color_threshold >= 0.0f) || std::isinf(pr->color_threshold))
        return fail(RT_ERR_INVALID, "color_threshold must be finite and >= 0");
    if (!(pr->normal_cos >= -1.0f && pr->normal_cos <= 1.0f)) return fail(RT_ERR_INVALID, "normal_cos must be in [-1, 1]");
    return RT_OK;
}

/* rt_adaptive_flags*: the header's checks up to the device */
int check_flags_args(const rt_adaptive_params *pr, int Wn, int H, const void *rgb, const void *hits, const void *out, bool device) {
    const int rc = check_params(pr);
    if (rc) return rc;
    if (Wn <= 0 || H <= 0) return fail(RT_ERR_INVALID, "need Wn, H > 0");
    if ((long long)Wn * (long long)H > kMaxRectPixels) return fail(RT_ERR_INVALID, "rectangle too large for its colours and records");
    if (!rgb || !hits || !out) return fail(RT_ERR_INVALID, "rgb / hits / out_flags is NULL");
    if (device && ((uintptr_t)hits & 15u) != 0) return fail(RT_ERR_INVALID, "d_hits must be 16-byte aligned");
    if (device && ((uintptr_t)rgb & 3u) != 0) return fail(RT_ERR_INVALID, "d_rgb must be 4-byte aligned");
    return RT_OK;
}

unsigned blocks_of(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

/* the flag kernel over the first Wn columns of a Wh x H rectangle */
int enqueue_flags(const rt_adaptive_params &pr, int Wn, int Wh, int H, const void *d_rgb, const void *d_hits, void *d_flags,
                  void *d_flags2, void *d_copy_rgb, void *d_counts, hipStream_t stream) {
    const size_t n = (size_t)Wn * (size_t)H;
    hipLaunchKernelGGL(rt_adaptive_flag_kernel, dim3(blocks_of(n)), dim3(kBlock), 0, stream, static_cast<const float *>(d_rgb),
                       static_cast<const uint4 *>(d_hits), Wh, H, pr.flag_all, pr.color_threshold, pr.normal_cos,
                       static_cast<uint8_t *>(d_flags), static_cast<uint8_t *>(d_flags2), static_cast<float *>(d_copy_rgb),
                       static_cast<uint32_t *>(d_counts), (uint32_t)n);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

/* the flagged pixels a launch traces: the caller's chunk_pixels, or the default -- as many as keep the rays and the sample
 * colours (36 k^2 bytes a pixel) within kChunkBytes -- and never more than kMaxChunk */
long long chunk_size(const rt_adaptive_params &pr) {
    const long long kk = (long long)pr.samples * pr.samples;
    const long long chunk = pr.chunk_pixels > 0 ? pr.chunk_pixels : (long long)(kChunkBytes / (size_t)(36 * kk));
    return std::min<long long>(chunk, kMaxChunk);
}

RtAdaptiveState *state_of(rt_scene *s) {
    return unit_state<RtAdaptiveState>(s, RT_INTERNAL_UNIT_ADAPTIVE, rt_internal_adaptive_free, rt_internal_adaptive_ms);
}

/* the last call's stage times from its events, once */
int collect(RtAdaptiveState *a) {
    if (a->clock.collected) return RT_OK;
    std::vector<float> t;
    const int rc = a->clock.intervals(&t);
    if (rc) return rc;
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = 0; i < t.size(); ++i) {
        if (i == 2) continue;                           /* (flags done -> second pass begun: the host's wait) */
        ms[i < 2 ? i : 2 + ((i - 3) & 1)] += t[i];
    }
    a->info.first_pass_ms = ms[0], a->info.flag_ms = ms[1], a->info.trace_ms = ms[2], a->info.resolve_ms = ms[3];
    return RT_OK;
}

/* rt_render_adaptive*'s checks in the header's order (device: the device variant's alignment as well); the soft-shadow
 * refusal comes last */
int check_render_args(const rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                      const rt_adaptive_params *pr, const void *out_rgb, bool device) {
    int rc = rt_internal_check_frame(s, cam, W, H, x0, x1, max_depth, out_rgb);
    if (rc == RT_OK) rc = check_params(pr);
    if (rc == RT_OK && pr->samples > 1) rc = rt_internal_check_virtual(cam, W, H, x0, x1, max_depth, pr->samples, out_rgb);
    if (rc == RT_OK) rc = rt_internal_check_gbuffer_size((long long)std::min(x1 + 1, W) - x0, H);
    if (rc) return rc;
    if (device && ((uintptr_t)out_rgb & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_rgb must be 4-byte aligned");
    if (rt_internal_scene_soft(s))
        return fail(RT_ERR_INVALID, "adaptive supersampling refuses a scene with area lights: their shadow samples are keyed by the "
                                    "pixel number in camera launches and by the ray index in ray batches (include/rt_capi_soft.h), "
                                    "so a refined pixel would not be rt_render_ssaa's and would change with chunk_pixels");
    return RT_OK;
}

/* the call, every argument checked, the handle locked, the strip not empty: into device memory, on stream */
int run(rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth, const rt_adaptive_params &pr,
        void *d_out_rgb, void *d_out_flags, hipStream_t stream) {
    RtAdaptiveState *a = state_of(s);
    const int Wn = x1 - x0, x1h = std::min(x1 + 1, W), Wh = x1h - x0;
    const size_t n = (size_t)Wn * (size_t)H, nh = (size_t)Wh * (size_t)H;
    const unsigned n_blocks = blocks_of(n);
    const int kl = pr.samples == 4 ? 2 : pr.samples - 1, kk = pr.samples * pr.samples;
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    const bool direct = RT_ADAPTIVE_DIRECT_FIRST != 0 && Wh == Wn;        /* no halo: the first pass's colours go where they stay */
    int rc = collect(a);                                  /* (the events are about to be recorded again) */
    if (rc == RT_OK && !direct) rc = a->first_rgb.grow(nh * 12);
    if (rc == RT_OK) rc = a->first_hits.grow(nh * sizeof(rt_hit));
    if (rc == RT_OK) rc = a->flags.grow(n);
    const unsigned n_groups = (n_blocks + kScanBlock - 1) / kScanBlock;
    if (rc == RT_OK) rc = a->counts.grow(((size_t)n_blocks + n_groups) * 8);      /* counts, offsets, the groups' sums and bases */
    if (rc == RT_OK) rc = a->list.grow(n * 4);
    if (rc == RT_OK) rc = rt_internal_order_stream(s, stream);           /* (before anything is enqueued, whatever comes first) */
    if (rc) return rc;
    if (!a->d_total) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&a->d_total), 4));
    if (!a->h_total) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&a->h_total), 4, hipHostMallocDefault));
    a->clock.n_events = 0;
    a->info = rt_adaptive_info{};
    a->info.pixels = (int64_t)n;

    /* the first pass: into scratch, from where the flag kernel, which reads the colours anyway, copies the strip's to the
     * output -- or, without a halo column, straight into the output */
    void *first_rgb = direct ? d_out_rgb : a->first_rgb.p;
    if ((rc = a->clock.mark(stream))) return rc;
    rc = rt_internal_launch_gbuffer(s, cam, W, H, x0, x1h, max_depth, first_rgb, a->first_hits.p, stream);
    if (rc == RT_OK) rc = a->clock.mark(stream);
    if (rc) return rc;
    uint32_t *counts = static_cast<uint32_t *>(a->counts.p), *offsets = counts + n_blocks;
    uint32_t *group_sums = offsets + n_blocks, *group_base = group_sums + n_groups;
    uint32_t *list = static_cast<uint32_t *>(a->list.p);
    rc = enqueue_flags(pr, Wn, Wh, H, first_rgb, a->first_hits.p, a->flags.p, d_out_flags, direct ? nullptr : d_out_rgb, counts,
                       stream);
    if (rc) return rc;
    hipLaunchKernelGGL(rt_adaptive_scan_groups_kernel, dim3(n_groups), dim3(kScanBlock), 0, stream, counts, offsets,
                       (uint32_t)n_blocks, group_sums);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rt_adaptive_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, group_sums, group_base, (uint32_t)n_groups,
                       a->d_total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a->h_total, a->d_total, 4, hipMemcpyDeviceToHost, stream));
    if (pr.samples > 1) {                                 /* (samples = 1: no second pass, the count alone, for the info) */
        hipLaunchKernelGGL(rt_adaptive_list_kernel, dim3(n_blocks), dim3(kBlock), 0, stream,
                           static_cast<const uint8_t *>(a->flags.p), offsets, group_base, list, (uint32_t)n);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = a->clock.mark(stream))) return rc;
    HIP_TRY(hipStreamSynchronize(stream));                /* THE call's one synchronisation: how many pixels the second pass has */
    const uint32_t flagged = *a->h_total;
    a->info.flagged = (int64_t)flagged;
    if (pr.samples > 1 && flagged > 0) {
        const long long chunk = chunk_size(pr);
        const size_t most = (size_t)std::min<long long>(chunk, flagged);
        rc = a->rays.grow(most * (size_t)kk * 24);
        if (rc == RT_OK) rc = a->samples.grow(most * (size_t)kk * 12);
        if (rc == RT_OK) rc = a->clock.mark(stream);
        if (rc) return rc;
        Cam c;
        for (int k = 0; k < 3; ++k) {
            c.so[k] = cam->screen_origin[k], c.ch[k] = cam->vector_horizontal[k];
            c.cv[k] = cam->vector_vertical[k], c.eye[k] = cam->eye_origin[k];
        }
        c.sw = cam->screen_width, c.sh = cam->screen_height, c.shw = cam->screen_halfwidth, c.shh = cam->screen_halfheight;
        for (long long g0 = 0; g0 < (long long)flagged; g0 += chunk) {
            const uint32_t m = (uint32_t)std::min<long long>(chunk, (long long)flagged - g0);
            const int n_rays = (int)(m * (uint32_t)kk);
            hipLaunchKernelGGL(rt_adaptive_raygen_kernel, dim3(blocks_of((size_t)n_rays)), dim3(kBlock), 0, stream, list + g0, m, kl,
                               c, W, H, x0, static_cast<float *>(a->rays.p));
            HIP_TRY(hipGetLastError());
            rc = rt_internal_launch_rays(s, n_rays, RT_ADAPTIVE_ROWS > 0 ? RT_ADAPTIVE_ROWS : n_rays, a->rays.p, max_depth,
                                         a->samples.p, stream);
            if (rc == RT_OK) rc = a->clock.mark(stream);
            if (rc) return rc;
            hipLaunchKernelGGL(rt_adaptive_resolve_kernel, dim3((m + kResolveSamples / kk - 1) / (kResolveSamples / kk)), dim3(kBlock), 0, stream,
                               list + g0, m, kk,
                               static_cast<const float *>(a->samples.p), static_cast<float *>(d_out_rgb));
            HIP_TRY(hipGetLastError());
            if ((rc = a->clock.mark(stream))) return rc;
            a->info.chunks += 1;
            a->info.rays += (int64_t)n_rays;
        }
    }
    a->clock.collected = false;
    a->clock.seq = rt_internal_launch_seq(s);
    return RT_OK;
}

} // namespace

extern "C" {

void rt_internal_adaptive_free(void *state) { delete static_cast<RtAdaptiveState *>(state); }

double rt_internal_adaptive_ms(void *state, uint64_t seq) {
    RtAdaptiveState *a = static_cast<RtAdaptiveState *>(state);
    if (!a || a->clock.seq != seq || a->clock.n_events == 0 || collect(a) != RT_OK) return -1.0;
    return a->info.first_pass_ms + a->info.flag_ms + a->info.trace_ms + a->info.resolve_ms;
}

int rt_capi_adaptive_version(void) { return RT_CAPI_ADAPTIVE_VERSION; }

int rt_adaptive_flags(int device, const rt_adaptive_params *pr, int Wn, int H, const float *rgb, const rt_hit *hits,
                      uint8_t *out_flags) {
    int rc = check_flags_args(pr, Wn, H, rgb, hits, out_flags, false);
    if (rc == RT_OK) rc = rt_internal_check_device(device);
    if (rc) return rc;
    const size_t pixels = (size_t)Wn * (size_t)H;
    const HostIn in[2] = {{rgb, pixels * 12}, {hits, pixels * sizeof(rt_hit)}};
    const HostOut out[1] = {{out_flags, pixels}};
    return staged_call(device, in, 2, out, 1, 0, nullptr, [&](void *const *d_in, void *const *d_out, void *) {
        return enqueue_flags(*pr, Wn, Wn, H, d_in[0], d_in[1], d_out[0], nullptr, nullptr, nullptr, nullptr);
    });
}

int rt_adaptive_flags_device(int device, const rt_adaptive_params *pr, int Wn, int H, const void *d_rgb, const void *d_hits,
                             void *d_out_flags, void *hip_stream) {
    int rc = check_flags_args(pr, Wn, H, d_rgb, d_hits, d_out_flags, true);
    if (rc == RT_OK) rc = rt_internal_check_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue_flags(*pr, Wn, Wn, H, d_rgb, d_hits, d_out_flags, nullptr, nullptr, nullptr, static_cast<hipStream_t>(hip_stream));
}

int rt_render_adaptive_device(rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                              const rt_adaptive_params *pr, void *d_out_rgb, void *d_out_flags, void *hip_stream) {
    const int rc = check_render_args(s, cam, W, H, x0, x1, max_depth, pr, d_out_rgb, true);
    if (rc || x0 == x1) return rc;
    const rt_adaptive_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    return run(s, cam, W, H, x0, x1, max_depth, p, d_out_rgb, d_out_flags, static_cast<hipStream_t>(hip_stream));
}

int rt_render_adaptive(rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                       const rt_adaptive_params *pr, float *out_rgb, uint8_t *out_flags) {
    int rc = check_render_args(s, cam, W, H, x0, x1, max_depth, pr, out_rgb, false);
    if (rc || x0 == x1) return rc;
    const rt_adaptive_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    RtAdaptiveState *a = state_of(s);
    const size_t n = (size_t)(x1 - x0) * (size_t)H;
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    rc = a->out_rgb.grow(n * 12);
    if (rc == RT_OK && out_flags) rc = a->out_flags.grow(n);
    if (rc == RT_OK) rc = run(s, cam, W, H, x0, x1, max_depth, p, a->out_rgb.p, out_flags ? a->out_flags.p : nullptr, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out_rgb, a->out_rgb.p, n * 12, hipMemcpyDeviceToHost));
    if (out_flags) HIP_TRY(hipMemcpy(out_flags, a->out_flags.p, n, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return RT_OK;
}

int rt_get_adaptive_info(const rt_scene *cs, rt_adaptive_info *out) {
    if (!cs || !out) return fail(RT_ERR_INVALID, "scene/out is NULL");
    rt_scene *s = const_cast<rt_scene *>(cs);
    rt_internal_lock(s);
    Unlock unlock{s};
    RtAdaptiveState *a = static_cast<RtAdaptiveState *>(rt_internal_unit_slot(s, RT_INTERNAL_UNIT_ADAPTIVE)->state);
    if (!a) {
        *out = rt_adaptive_info{};
        return RT_OK;
    }
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    const int rc = collect(a);
    if (rc) return rc;
    *out = a->info;
    return RT_OK;
}

} // extern "C"
