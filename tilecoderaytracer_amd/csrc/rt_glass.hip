/*
 * rt_glass.hip -- implementation of include/rt_glass.h: the chain of every ray of a batch through the scene's mirrors and its
 * glass, walked on the GPU.  The header is the definition; the kernel is bit-exact to it (the library's arithmetic flags: no
 * contraction, correctly rounded divide and square root, denormals kept).
 *
 * SHAPE: rt_mirror.hip's, launch for launch.  Per chunk of rays and for bounce s = 0 .. max_bounces, a hit
 * query of the chunk's current rays through rt_internal_launch_hits and a step kernel after it.  The step is rt_glass_body.h's
 * (rt_glass_step_kernel), built from rt_mirror_body.h's helpers: a lane whose hit is a candidate
 * reads its object's three table rows (rt_internal_object_glass), computes the transmitted child and, if it exists, goes on
 * along it.  In place only; the compacting form is rt_glass_compact.hip's (include/rt_glass_compact.h).  Nothing is read back, the launches depend on the
 * arguments alone, and the call never waits for the device.  The scratch is a unit slot's of its own, so that a mirror call and a
 * glass call of one handle keep their own bookkeeping (rt_get_mirror_info, rt_get_glass_info).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_glass.h"
#include "rt_host.h"
#include "rt_glass_body.h"

#pragma clang fp contract(off)

static_assert(sizeof(rt_glass_params) == 16 && sizeof(rt_glass_info) == 32, "rt_glass.h layouts");
static_assert(sizeof(rt_hit) == 48, "rt_capi_query.h layout");

namespace {

constexpr int kBlock = kMirrorBlock;                   /* rays a workgroup */
constexpr size_t kChunkBytes = (size_t)256 << 20;      /* the default chunk: its scratch within 256 MiB (rt_mirror.hip's) */
constexpr int kStateWords = 14;                        /* a ray's state: the word, w, L, A -- each a plane of the chunk */
constexpr int kStateWordsNoGuide = 4;                  /* without a guide: the word and w */
constexpr size_t kRayBytes = 48 + 24 + 4 * kStateWords;   /* a ray's scratch: its record, its next ray, its state */

/* the handle's scratch, which only grows, and the last call's bookkeeping */
struct RtGlassState {
    Buffer records, rays, state;                           /* a chunk's records, its next rays, its state planes */
    StageClock clock;                                      /* the last call's start, then per chunk and bounce query, step */
    rt_glass_info info{};
    ~RtGlassState() { clock.release(); }
};

int chunk_rays(const rt_glass_params &pr, int n) {
    const long long c = pr.chunk_rays > 0 ? pr.chunk_rays : (long long)(kChunkBytes / kRayBytes);
    return (int)std::min<long long>(c, n);
}

/* the last call's stage times from its events, once: the intervals alternate query, step */
int collect(RtGlassState *a) {
    if (a->clock.collected) return RT_OK;
    std::vector<float> t;
    const int rc = a->clock.intervals(&t);
    if (rc) return rc;
    double ms[2] = {0.0, 0.0};
    for (size_t i = 0; i < t.size(); ++i) ms[i & 1] += t[i];
    a->info.query_ms = ms[0], a->info.step_ms = ms[1];
    return RT_OK;
}

void glass_free(void *state) { delete static_cast<RtGlassState *>(state); }

double glass_ms(void *state, uint64_t seq) {
    RtGlassState *a = static_cast<RtGlassState *>(state);
    if (!a || a->clock.seq != seq || a->clock.n_events == 0 || collect(a) != RT_OK) return -1.0;
    return a->info.query_ms + a->info.step_ms;
}

RtGlassState *state_of(rt_scene *s) { return unit_state<RtGlassState>(s, RT_INTERNAL_UNIT_GLASS, glass_free, glass_ms); }

template <bool FIRST, bool GUIDE>
void launch_step(uint32_t m, uint32_t stride, int last, const rt_glass_params &pr, const float *rf, const float4 *glass, int n_objects,
                 const void *records, const void *rays_k, const void *rays0, void *rays_next, void *state, void *out_hits,
                 void *out_guide, void *out_weight, void *out_path, hipStream_t stream) {
    hipLaunchKernelGGL((rt_glass_step_kernel<FIRST, GUIDE>), dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m, stride, last,
                       pr.min_reflective, pr.min_transmissive, rf, glass, n_objects, static_cast<const float4 *>(records),
                       static_cast<const float *>(rays_k), static_cast<const float *>(rays0), static_cast<float *>(rays_next),
                       static_cast<uint32_t *>(state), static_cast<float4 *>(out_hits), static_cast<float4 *>(out_guide),
                       static_cast<float *>(out_weight), static_cast<uint32_t *>(out_path));
}

/* the call, every argument checked, the handle locked, n > 0: device memory, on stream.  The events of the call before are
 * recorded anew without being waited for: its stage times, if nobody asked for them, are lost. */
int run(rt_scene *s, const rt_glass_params &pr, int n, int rows, const void *d_rays, void *d_hits, void *d_guide, void *d_weight,
        void *d_path, hipStream_t stream) {
    RtGlassState *a = state_of(s);
    const int chunk = chunk_rays(pr, n);
    const bool guide = d_guide != nullptr;
    const float *d_rf = nullptr;
    const float4 *d_glass = nullptr;
    int n_objects = 0;
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    int rc = rt_internal_object_reflective(s, &d_rf, &n_objects);
    if (rc == RT_OK) rc = rt_internal_object_glass(s, &d_glass, &n_objects);
    if (rc == RT_OK) rc = a->records.grow((size_t)chunk * 48);
    if (rc == RT_OK) rc = a->rays.grow((size_t)chunk * 24);
    if (rc == RT_OK) rc = a->state.grow((size_t)chunk * 4 * (size_t)(guide ? kStateWords : kStateWordsNoGuide));
    if (rc == RT_OK) rc = rt_internal_order_stream(s, stream);           /* (before anything is enqueued, whatever comes first) */
    if (rc) return rc;
    a->clock.n_events = 0;
    a->clock.collected = true;
    a->info = rt_glass_info{};
    a->info.rays = n;
    if ((rc = a->clock.mark(stream))) return rc;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        const char *rays0 = static_cast<const char *>(d_rays) + (size_t)i0 * 24;
        void *hits = static_cast<char *>(d_hits) + (size_t)i0 * 48;
        void *gd = guide ? static_cast<char *>(d_guide) + (size_t)i0 * 48 : nullptr;
        void *wt = d_weight ? static_cast<char *>(d_weight) + (size_t)i0 * 12 : nullptr;
        void *pa = d_path ? static_cast<char *>(d_path) + (size_t)i0 * 4 : nullptr;
        for (int b = 0; b <= pr.max_bounces; ++b) {
            const void *rays_k = b == 0 ? static_cast<const void *>(rays0) : a->rays.p;
            rc = rt_internal_launch_hits(s, m, rows, rays_k, a->records.p, stream);
            if (rc == RT_OK) rc = a->clock.mark(stream);
            if (rc) return rc;
            const int last = b == pr.max_bounces;
            auto step = b == 0 ? (guide ? launch_step<true, true> : launch_step<true, false>)
                               : (guide ? launch_step<false, true> : launch_step<false, false>);
            step((uint32_t)m, (uint32_t)chunk, last, pr, d_rf, d_glass, n_objects, a->records.p, rays_k, rays0, a->rays.p, a->state.p,
                 hits, gd, wt, pa, stream);
            HIP_TRY(hipGetLastError());
            if ((rc = a->clock.mark(stream))) return rc;
            a->info.queries += 1;
        }
        a->info.chunks += 1;
    }
    a->clock.collected = false;
    a->clock.seq = rt_internal_launch_seq(s);
    return RT_OK;
}

} // namespace

extern "C" {

int rt_glass_version(void) { return RT_GLASS_VERSION; }

int rt_glass_records_device(rt_scene *s, const rt_glass_params *pr, int n, int rows, const void *d_rays, void *d_out_hits,
                            void *d_out_guide, void *d_out_weight, void *d_out_path, void *hip_stream) {
    const int rc = rt_mirror_check_args(s, pr, n, rows, d_rays, d_out_hits, d_out_guide, d_out_weight, d_out_path, true);
    if (rc || n == 0) return rc;
    const rt_glass_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    return run(s, p, n, rows, d_rays, d_out_hits, d_out_guide, d_out_weight, d_out_path, static_cast<hipStream_t>(hip_stream));
}

int rt_glass_records(rt_scene *s, const rt_glass_params *pr, int n, int rows, const float *rays, rt_hit *out_hits, rt_hit *out_guide,
                     float *out_weight, uint32_t *out_path) {
    const int rc = rt_mirror_check_args(s, pr, n, rows, rays, out_hits, out_guide, out_weight, out_path, false);
    if (rc || n == 0) return rc;
    const rt_glass_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    const HostIn in[1] = {{rays, (size_t)n * 24}};
    const HostOut out[4] = {{out_hits, (size_t)n * 48}, {out_guide, (size_t)n * 48}, {out_weight, (size_t)n * 12},
                            {out_path, (size_t)n * 4}};
    return staged_call(rt_internal_scene_device(s), in, 1, out, 4, 0, nullptr, [&](void *const *d_in, void *const *d_out, void *) {
        return run(s, p, n, rows, d_in[0], d_out[0], d_out[1], d_out[2], d_out[3], nullptr);
    });
}

int rt_get_glass_info(const rt_scene *cs, rt_glass_info *out) {
    if (!cs || !out) return fail(RT_ERR_INVALID, "scene/out is NULL");
    rt_scene *s = const_cast<rt_scene *>(cs);
    rt_internal_lock(s);
    Unlock unlock{s};
    RtGlassState *a = static_cast<RtGlassState *>(rt_internal_unit_slot(s, RT_INTERNAL_UNIT_GLASS)->state);
    if (!a) {
        *out = rt_glass_info{};
        return RT_OK;
    }
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    const int rc = collect(a);
    if (rc) return rc;
    *out = a->info;
    return RT_OK;
}

} // extern "C"
