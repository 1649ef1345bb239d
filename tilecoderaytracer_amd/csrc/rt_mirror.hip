/*
 * rt_mirror.hip -- implementation of include/rt_mirror.h: the mirror chain of every ray of a batch, walked on the GPU.  The
 * header is the definition; the kernel is bit-exact to it (the library's arithmetic flags: no contraction, correctly rounded
 * divide and square root, denormals kept).
 *
 * SHAPE, modelled on rt_indirect.hip.  The query kernels are rt_capi.hip's: every ray of the chain is
 * asked for its nearest hit by its hit query, through rt_internal.h -- every launch decision stays there.  Around them, here,
 * per chunk of rays and for bounce s = 0 .. max_bounces:
 *   query   rt_internal_launch_hits of the chunk's current rays (s == 0: the caller's, read where they are);
 *   step    one lane a ray: its record, its ray and its state -> the next ray and state, or the terminal outputs, after which
 *           the ray is retired: six +0.0f as its next ray, a flag in its state word, and nothing more is read or written for
 *           it.  The instance after the last query finalises every ray still alive (cut).
 * There is no init kernel: the first step is compiled with the starting state as constants (w = 1, L = 0, A = I, tag = 0),
 * so nothing writes that state only to have it read back.  d is not carried: it is normalize(T - E) of the ray the lane reads
 * anyway, and d0 and E of the guide come from the caller's rays, which outlive the call.  Nothing is read back: the launches
 * depend on the arguments alone, and the call never waits for the device.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_mirror.h"
#include "rt_host.h"
#include "rt_mirror_body.h"

#pragma clang fp contract(off)

/* -DRT_MIRROR_VARIANTS=1 (scripts/mirror_experiments.py) builds both ways of reading the records and exports the switch
 * between them, rt_internal_mirror_variant(); the library proper has the kept one alone. */
#ifndef RT_MIRROR_VARIANTS
#define RT_MIRROR_VARIANTS 0
#endif

static_assert(sizeof(rt_mirror_params) == 12 && sizeof(rt_mirror_info) == 32, "rt_mirror.h layouts");
static_assert(sizeof(rt_hit) == 48, "rt_capi_query.h layout");

namespace {

constexpr int kBlock = kMirrorBlock;                   /* rays a workgroup */
constexpr size_t kChunkBytes = (size_t)256 << 20;      /* the default chunk: its scratch within 256 MiB */
constexpr int kStateWords = 14;                        /* a ray's state: the word, w, L, A -- each a plane of the chunk */
constexpr int kStateWordsNoGuide = 4;                  /* without a guide: the word and w */
constexpr size_t kRayBytes = 48 + 24 + 4 * kStateWords;   /* a ray's scratch: its record, its next ray, its state */
/* How the step kernel (rt_mirror_body.h's, which rt_mirror_compact.hip instantiates as well; here in place, COMPACT false)
 * reads its 48-byte-strided records.  false: three 16-byte loads a lane.  true: the workgroup's records as
 * the consecutive words they are through LDS (rt_accumulate_body.h's and rt_upsample.hip's way).  Both were measured
 * (profiles/mirror_experiments.txt); this is the one kept. */
constexpr bool kStageLds = false;

} // namespace

namespace {

/* the handle's scratch, which only grows, and the last call's bookkeeping */
struct RtMirrorState {
    Buffer records, rays, state;                           /* a chunk's records, its next rays, its state planes */
    StageClock clock;                                      /* the last call's start, then per chunk and bounce query, step */
    rt_mirror_info info{};
    ~RtMirrorState() { clock.release(); }
};

/* the header's checks (1) .. (10): rt_mirror_body.h's, which rt_mirror_compact.hip makes as well */
int check_args(const rt_scene *s, const rt_mirror_params *pr, int n, int rows, const void *rays, const void *out_hits,
               const void *out_guide, const void *out_weight, const void *out_path, bool device) {
    return rt_mirror_check_args(s, pr, n, rows, rays, out_hits, out_guide, out_weight, out_path, device);
}

/* the rays a launch walks: the caller's chunk_rays, or the default -- as many as keep the scratch within kChunkBytes -- never
 * more than the batch has */
int chunk_rays(const rt_mirror_params &pr, int n) {
    const long long c = pr.chunk_rays > 0 ? pr.chunk_rays : (long long)(kChunkBytes / kRayBytes);
    return (int)std::min<long long>(c, n);
}

/* the last call's stage times from its events, once: the intervals alternate query, step */
int collect(RtMirrorState *a) {
    if (a->clock.collected) return RT_OK;
    std::vector<float> t;
    const int rc = a->clock.intervals(&t);
    if (rc) return rc;
    double ms[2] = {0.0, 0.0};
    for (size_t i = 0; i < t.size(); ++i) ms[i & 1] += t[i];
    a->info.query_ms = ms[0], a->info.step_ms = ms[1];
    return RT_OK;
}

void mirror_free(void *state) { delete static_cast<RtMirrorState *>(state); }

double mirror_ms(void *state, uint64_t seq) {
    RtMirrorState *a = static_cast<RtMirrorState *>(state);
    if (!a || a->clock.seq != seq || a->clock.n_events == 0 || collect(a) != RT_OK) return -1.0;
    return a->info.query_ms + a->info.step_ms;
}

RtMirrorState *state_of(rt_scene *s) { return unit_state<RtMirrorState>(s, RT_INTERNAL_UNIT_MIRROR, mirror_free, mirror_ms); }

#if RT_MIRROR_VARIANTS
bool g_stage_lds = kStageLds;
#else
constexpr bool g_stage_lds = kStageLds;
#endif

template <bool FIRST, bool GUIDE, bool STAGE = kStageLds>
void launch_step(uint32_t m, uint32_t stride, int last, float min_reflective, const float *rf, int n_objects, const void *records,
                 const void *rays_k, const void *rays0, void *rays_next, void *state, void *out_hits, void *out_guide,
                 void *out_weight, void *out_path, hipStream_t stream) {
#if RT_MIRROR_VARIANTS
    if (STAGE == kStageLds && g_stage_lds != kStageLds)
        return launch_step<FIRST, GUIDE, !kStageLds>(m, stride, last, min_reflective, rf, n_objects, records, rays_k, rays0, rays_next,
                                                     state, out_hits, out_guide, out_weight, out_path, stream);
#endif
    hipLaunchKernelGGL((rt_mirror_step_kernel<FIRST, GUIDE, STAGE, false>), dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m, stride,
                       last, min_reflective, rf, n_objects, static_cast<const float4 *>(records), static_cast<const float *>(rays_k),
                       static_cast<const float *>(rays0), static_cast<float *>(rays_next), static_cast<uint32_t *>(state),
                       static_cast<float4 *>(out_hits), static_cast<float4 *>(out_guide), static_cast<float *>(out_weight),
                       static_cast<uint32_t *>(out_path), nullptr, nullptr, nullptr, nullptr, nullptr);
}

/* the call, every argument checked, the handle locked, n > 0: device memory, on stream.  The events of the call before are
 * recorded anew without being waited for: its stage times, if nobody asked for them, are lost. */
int run(rt_scene *s, const rt_mirror_params &pr, int n, int rows, const void *d_rays, void *d_hits, void *d_guide, void *d_weight,
        void *d_path, hipStream_t stream) {
    RtMirrorState *a = state_of(s);
    const int chunk = chunk_rays(pr, n);
    const bool guide = d_guide != nullptr;
    const float *d_rf = nullptr;
    int n_objects = 0;
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    int rc = rt_internal_object_reflective(s, &d_rf, &n_objects);
    if (rc == RT_OK) rc = a->records.grow((size_t)chunk * 48);
    if (rc == RT_OK) rc = a->rays.grow((size_t)chunk * 24);
    if (rc == RT_OK) rc = a->state.grow((size_t)chunk * 4 * (size_t)(guide ? kStateWords : kStateWordsNoGuide));
    if (rc == RT_OK) rc = rt_internal_order_stream(s, stream);           /* (before anything is enqueued, whatever comes first) */
    if (rc) return rc;
    a->clock.n_events = 0;
    a->clock.collected = true;
    a->info = rt_mirror_info{};
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
            step((uint32_t)m, (uint32_t)chunk, last, pr.min_reflective, d_rf, n_objects, a->records.p, rays_k, rays0, a->rays.p,
                 a->state.p, hits, gd, wt, pa, stream);
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

int rt_mirror_version(void) { return RT_MIRROR_VERSION; }

#if RT_MIRROR_VARIANTS
/* 0: three 16-byte loads a lane; 1: through LDS; returns what was set before */
int rt_internal_mirror_variant(int stage_lds) {
    const int before = g_stage_lds;
    g_stage_lds = stage_lds != 0;
    return before;
}
#endif

int rt_mirror_records_device(rt_scene *s, const rt_mirror_params *pr, int n, int rows, const void *d_rays, void *d_out_hits,
                             void *d_out_guide, void *d_out_weight, void *d_out_path, void *hip_stream) {
    const int rc = check_args(s, pr, n, rows, d_rays, d_out_hits, d_out_guide, d_out_weight, d_out_path, true);
    if (rc || n == 0) return rc;
    const rt_mirror_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    return run(s, p, n, rows, d_rays, d_out_hits, d_out_guide, d_out_weight, d_out_path, static_cast<hipStream_t>(hip_stream));
}

int rt_mirror_records(rt_scene *s, const rt_mirror_params *pr, int n, int rows, const float *rays, rt_hit *out_hits,
                      rt_hit *out_guide, float *out_weight, uint32_t *out_path) {
    const int rc = check_args(s, pr, n, rows, rays, out_hits, out_guide, out_weight, out_path, false);
    if (rc || n == 0) return rc;
    const rt_mirror_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    const HostIn in[1] = {{rays, (size_t)n * 24}};
    const HostOut out[4] = {{out_hits, (size_t)n * 48}, {out_guide, (size_t)n * 48}, {out_weight, (size_t)n * 12},
                            {out_path, (size_t)n * 4}};
    return staged_call(rt_internal_scene_device(s), in, 1, out, 4, 0, nullptr, [&](void *const *d_in, void *const *d_out, void *) {
        return run(s, p, n, rows, d_in[0], d_out[0], d_out[1], d_out[2], d_out[3], nullptr);
    });
}

int rt_get_mirror_info(const rt_scene *cs, rt_mirror_info *out) {
    if (!cs || !out) return fail(RT_ERR_INVALID, "scene/out is NULL");
    rt_scene *s = const_cast<rt_scene *>(cs);
    rt_internal_lock(s);
    Unlock unlock{s};
    RtMirrorState *a = static_cast<RtMirrorState *>(rt_internal_unit_slot(s, RT_INTERNAL_UNIT_MIRROR)->state);
    if (!a) {
        *out = rt_mirror_info{};
        return RT_OK;
    }
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    const int rc = collect(a);
    if (rc) return rc;
    *out = a->info;
    return RT_OK;
}

} // extern "C"
