/*
 * rt_glass_compact.hip -- implementation of include/rt_glass_compact.h: rt_glass_records over the rays still alive.  The
 * definition is rt_glass.h's; the device code is rt_glass_compact_body.h's -- one decision function (rt_glass_decide: rt_glass.h's
 * steps 3 to 8), a count kernel and a step kernel that both call it -- over rt_glass_body.h's child; the argument checks are
 * rt_mirror_body.h's, the one copy (the library's arithmetic flags: no contraction, correctly rounded divide and square root,
 * denormals kept).
 *
 * SHAPE: rt_mirror_compact.hip's, launch for launch.  Per chunk of m rays the live rays of bounce b are a
 * dense list of cnt entries in ray order -- an entry is its ray (24 bytes), its state planes (16 or 56) and the ray's index in
 * the chunk -- and bounce 0's list is the chunk itself (cnt = m, the caller's rays, no state, index = entry).  For
 * b = 0 .. max_bounces, while cnt > 0:
 *   query   rt_internal_launch_hits of the list's cnt rays (b == 0: the caller's rows; later flat, rows = cnt);
 *   count   (not on bounce max_bounces) one lane an entry decides `follow` -- two words of its record, its object's rf and tf,
 *           and for a candidate the rest: distance, point, ray, 48 table bytes, the refraction -- and a ballot and a population
 *           count per wavefront give each workgroup's number of chains that go on;
 *   scan    rt_mirror_compact.hip's instantiation of rt_scan.h's two-level exclusive scan (rt_internal_mirror_compact_scan);
 *   step    one lane an entry: a chain that ends writes out_*[index] -- each output word exactly once, here -- and one that
 *           goes on writes its next ray, state and index to place scan[workgroup] + its rank in the workgroup of the OTHER
 *           list: nothing is written where another lane may still be reading, and the next list is in ray order again;
 *   -- unless b == max_bounces the host waits for the stream and reads the total: the next bounce's cnt --
 * The total is copied to pinned memory between the scan and the step, so the step is the last thing the wait waits for.  No
 * workgroup waits for another anywhere: every dependency is the stream's order.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_glass_compact.h"
#include "rt_host.h"
#include "rt_glass_compact_body.h"

#pragma clang fp contract(off)

static_assert(sizeof(rt_glass_params) == 16 && sizeof(rt_glass_compact_info) == 568, "rt_glass_compact.h layouts");
static_assert(offsetof(rt_glass_compact_info, alive) == 48, "rt_glass_compact.h layouts");
static_assert(sizeof(rt_hit) == 48, "rt_capi_query.h layout");

namespace {

constexpr int kBlock = kMirrorBlock;                   /* entries a workgroup */
constexpr size_t kChunkBytes = (size_t)256 << 20;      /* the default chunk: its scratch within 256 MiB */
constexpr int kStateWords = 14;                        /* an entry's state: the word (which carries g), w, L, A -- each a plane */
constexpr int kStateWordsNoGuide = 4;                  /* without a guide: the word and w */
/* a ray's scratch: its record, and in each of the two lists a ray, a state and an index; and, reckoned as one byte, the 8 bytes
 * per kBlock rays of the counts and their scan (and 8 per kBlock * kScanBlock of the groups') */
constexpr size_t kRayBytes = 48 + 2 * (24 + 4 * kStateWords + 4) + 1;
static_assert(kRayBytes == 217, "the figure include/rt_glass_compact.h states");
static_assert(kChunkBytes / kRayBytes == 1237029, "the default chunk include/rt_glass_compact.h states");

/* the handle's scratch, which only grows, and the last call's bookkeeping */
struct RtGlassCompactState {
    Buffer records, rays[2], state[2], idx[2], counts;     /* a chunk's records, the two lists, the counts and their scans */
    uint32_t *d_total = nullptr, *h_total = nullptr;       /* the chains that go on: on the device, and pinned */
    StageClock clock;                                      /* per chunk and bounce: before the query, after it, after the step */
    rt_glass_compact_info info{};
    ~RtGlassCompactState() {
        clock.release();
        if (d_total) (void)hipFree(d_total);
        if (h_total) (void)hipHostFree(h_total);
    }
};

/* the rays a chunk has: the caller's chunk_rays, or the default -- as many as keep the scratch within kChunkBytes -- never
 * more than the batch has */
int chunk_rays(const rt_glass_params &pr, int n) {
    const long long c = pr.chunk_rays > 0 ? pr.chunk_rays : (long long)(kChunkBytes / kRayBytes);
    return (int)std::min<long long>(c, n);
}

/* the last call's stage times from its events, once: the intervals go query, step, the host's wait */
int collect(RtGlassCompactState *a) {
    if (a->clock.collected) return RT_OK;
    std::vector<float> t;
    const int rc = a->clock.intervals(&t);
    if (rc) return rc;
    double ms[3] = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < t.size(); ++i) ms[i % 3] += t[i];
    a->info.query_ms = ms[0], a->info.step_ms = ms[1];
    return RT_OK;
}

void compact_free(void *state) { delete static_cast<RtGlassCompactState *>(state); }

double compact_ms(void *state, uint64_t seq) {
    RtGlassCompactState *a = static_cast<RtGlassCompactState *>(state);
    if (!a || a->clock.seq != seq || a->clock.n_events == 0 || collect(a) != RT_OK) return -1.0;
    return a->info.query_ms + a->info.step_ms;
}

RtGlassCompactState *state_of(rt_scene *s) {
    return unit_state<RtGlassCompactState>(s, RT_INTERNAL_UNIT_GLASS_COMPACT, compact_free, compact_ms);
}

unsigned blocks_of(uint32_t n) { return (n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock; }

template <bool FIRST, bool GUIDE>
void launch_step(uint32_t cnt, uint32_t stride, int last, const rt_glass_params &pr, const float *rf, const float4 *glass, int n_objects,
                 const void *records, const void *rays_k, const void *rays0, const void *state_k, const void *idx_k, void *rays_next,
                 void *state_next, void *idx_next, const uint32_t *offsets, const uint32_t *group_base, void *out_hits,
                 void *out_guide, void *out_weight, void *out_path, hipStream_t stream) {
    hipLaunchKernelGGL((rt_glass_compact_step_kernel<FIRST, GUIDE>), dim3(blocks_of(cnt)), dim3(kBlock), 0, stream, cnt, stride, last,
                       pr.min_reflective, pr.min_transmissive, rf, glass, n_objects, static_cast<const float4 *>(records),
                       static_cast<const float *>(rays_k), static_cast<const float *>(rays0), static_cast<const uint32_t *>(state_k),
                       static_cast<const uint32_t *>(idx_k), static_cast<float *>(rays_next), static_cast<uint32_t *>(state_next),
                       static_cast<uint32_t *>(idx_next), offsets, group_base, static_cast<float4 *>(out_hits),
                       static_cast<float4 *>(out_guide), static_cast<float *>(out_weight), static_cast<uint32_t *>(out_path));
}

/* the call, every argument checked, the handle locked, n > 0: device memory, on stream, which is waited for.  The events of the
 * call before are recorded anew without being waited for: its stage times, if nobody asked for them, are lost. */
int run(rt_scene *s, const rt_glass_params &pr, int n, int rows, const void *d_rays, void *d_hits, void *d_guide, void *d_weight,
        void *d_path, hipStream_t stream) {
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    if (stream) {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing(stream, &capturing));
        if (capturing != hipStreamCaptureStatusNone)
            return fail(RT_ERR_INVALID, "the stream is capturing: rt_glass_records_compact_device waits for its stream and cannot "
                                        "be recorded into a graph (rt_glass_records_device can)");
    }
    RtGlassCompactState *a = state_of(s);
    const int chunk = chunk_rays(pr, n);
    const bool guide = d_guide != nullptr;
    const size_t words = (size_t)(guide ? kStateWords : kStateWordsNoGuide);
    const unsigned max_blocks = blocks_of((uint32_t)chunk), max_groups = (max_blocks + kScanBlock - 1) / kScanBlock;
    const float *d_rf = nullptr;
    const float4 *d_glass = nullptr;
    int n_objects = 0;
    int rc = rt_internal_object_reflective(s, &d_rf, &n_objects);
    if (rc == RT_OK) rc = rt_internal_object_glass(s, &d_glass, &n_objects);
    if (rc == RT_OK) rc = a->records.grow((size_t)chunk * 48);
    if (pr.max_bounces > 0)                               /* (no list without a second bounce) */
        for (int l = 0; l < 2; ++l) {
            if (rc == RT_OK) rc = a->rays[l].grow((size_t)chunk * 24);
            if (rc == RT_OK) rc = a->state[l].grow((size_t)chunk * 4 * words);
            if (rc == RT_OK) rc = a->idx[l].grow((size_t)chunk * 4);
        }
    if (rc == RT_OK) rc = a->counts.grow(((size_t)max_blocks + max_groups) * 8);      /* counts, offsets, the groups' sums and bases */
    if (rc == RT_OK) rc = rt_internal_order_stream(s, stream);           /* (before anything is enqueued, whatever comes first) */
    if (rc) return rc;
    if (!a->d_total) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&a->d_total), 4));
    if (!a->h_total) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&a->h_total), 4, hipHostMallocDefault));
    uint32_t *counts = static_cast<uint32_t *>(a->counts.p), *offsets = counts + max_blocks;
    uint32_t *group_sums = offsets + max_blocks, *group_base = group_sums + max_groups;
    a->clock.n_events = 0;
    a->clock.collected = true;
    a->info = rt_glass_compact_info{};
    a->info.rays = n;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        const char *rays0 = static_cast<const char *>(d_rays) + (size_t)i0 * 24;
        void *hits = static_cast<char *>(d_hits) + (size_t)i0 * 48;
        void *gd = guide ? static_cast<char *>(d_guide) + (size_t)i0 * 48 : nullptr;
        void *wt = d_weight ? static_cast<char *>(d_weight) + (size_t)i0 * 12 : nullptr;
        void *pa = d_path ? static_cast<char *>(d_path) + (size_t)i0 * 4 : nullptr;
        uint32_t cnt = (uint32_t)m;
        for (int b = 0; b <= pr.max_bounces && cnt > 0; ++b) {
            const int to = b & 1, from = to ^ 1;          /* the list this bounce writes, and the one it reads (b >= 1) */
            const void *rays_k = b == 0 ? static_cast<const void *>(rays0) : a->rays[from].p;
            const int last = b == pr.max_bounces;
            if ((rc = a->clock.mark(stream))) return rc;
            rc = rt_internal_launch_hits(s, (int)cnt, b == 0 ? rows : (int)cnt, rays_k, a->records.p, stream);
            if (rc == RT_OK) rc = a->clock.mark(stream);
            if (rc) return rc;
            a->info.queries += 1;
            a->info.alive[b] += (int64_t)cnt;
            a->info.rays_queried += (int64_t)cnt;
            if (!last) {
                const unsigned n_blocks = blocks_of(cnt);
                hipLaunchKernelGGL(rt_glass_compact_count_kernel, dim3(n_blocks), dim3(kBlock), 0, stream, cnt, pr.min_reflective,
                                   pr.min_transmissive, d_rf, d_glass, n_objects, static_cast<const float *>(a->records.p),
                                   static_cast<const float *>(rays_k), counts);
                HIP_TRY(hipGetLastError());
                if ((rc = rt_internal_mirror_compact_scan(counts, n_blocks, offsets, group_sums, group_base, a->d_total, stream))) return rc;
                HIP_TRY(hipMemcpyAsync(a->h_total, a->d_total, 4, hipMemcpyDeviceToHost, stream));
            }
            auto step = b == 0 ? (guide ? launch_step<true, true> : launch_step<true, false>)
                               : (guide ? launch_step<false, true> : launch_step<false, false>);
            step(cnt, (uint32_t)chunk, last, pr, d_rf, d_glass, n_objects, a->records.p, rays_k, rays0, a->state[from].p, a->idx[from].p,
                 a->rays[to].p, a->state[to].p, a->idx[to].p, offsets, group_base, hits, gd, wt, pa, stream);
            HIP_TRY(hipGetLastError());
            if ((rc = a->clock.mark(stream))) return rc;
            if (last) break;
            HIP_TRY(hipStreamSynchronize(stream));        /* the bounce's one wait: how many rays the next query has */
            a->info.syncs += 1;
            const uint32_t next = *a->h_total;
            if (next > cnt) return fail(RT_ERR_HIP, "rt_glass_records_compact: more chains go on than the bounce had");
            cnt = next;
        }
        a->info.chunks += 1;
    }
    a->clock.collected = false;
    a->clock.seq = rt_internal_launch_seq(s);
    return RT_OK;
}

} // namespace

extern "C" {

int rt_glass_compact_version(void) { return RT_GLASS_COMPACT_VERSION; }

int rt_glass_records_compact_device(rt_scene *s, const rt_glass_params *pr, int n, int rows, const void *d_rays, void *d_out_hits,
                                    void *d_out_guide, void *d_out_weight, void *d_out_path, void *hip_stream) {
    const int rc = rt_mirror_check_args(s, pr, n, rows, d_rays, d_out_hits, d_out_guide, d_out_weight, d_out_path, true);
    if (rc || n == 0) return rc;
    const rt_glass_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    return run(s, p, n, rows, d_rays, d_out_hits, d_out_guide, d_out_weight, d_out_path, static_cast<hipStream_t>(hip_stream));
}

int rt_glass_records_compact(rt_scene *s, const rt_glass_params *pr, int n, int rows, const float *rays, rt_hit *out_hits,
                             rt_hit *out_guide, float *out_weight, uint32_t *out_path) {
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

int rt_get_glass_compact_info(const rt_scene *cs, rt_glass_compact_info *out) {
    if (!cs || !out) return fail(RT_ERR_INVALID, "scene/out is NULL");
    rt_scene *s = const_cast<rt_scene *>(cs);
    rt_internal_lock(s);
    Unlock unlock{s};
    RtGlassCompactState *a = static_cast<RtGlassCompactState *>(rt_internal_unit_slot(s, RT_INTERNAL_UNIT_GLASS_COMPACT)->state);
    if (!a) {
        *out = rt_glass_compact_info{};
        return RT_OK;
    }
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    const int rc = collect(a);
    if (rc) return rc;
    *out = a->info;
    return RT_OK;
}

} // extern "C"
