/*
 * rt_paths_compact.hip -- implementation of include/rt_paths_compact.h: rt_indirect_paths over the paths still alive.  The
 * definition is rt_paths.h's and the arithmetic of a step is rt_paths_body.h's -- the mask and the accumulation, the decision
 * (rt_paths_decide), the next ray, the resolve, the argument checks; what this unit adds is where a step reads and writes, and a
 * total the host reads back (the library's arithmetic flags: no contraction, correctly rounded divide and square root, denormals
 * kept).
 *
 * SHAPE: rt_mirror_compact.hip's loop around rt_paths.hip's stages.  Per chunk of m records the paths
 * alive at bounce b are a dense list of cnt entries in path order -- an entry is its ray (24 bytes) and the path's SLOT r in the
 * chunk (4) -- and bounce 0's list is the chunk itself (cnt = m S, the ray generation's rays, slot = entry).  What a bounce's ray
 * batch and hit query return, the colour (12) and the record (48), is dense, one per entry; the path's throughput T and its sum
 * acc stay at its slot, so that the resolve reads acc where rt_paths.hip's does and nothing is carried from list to list but the
 * ray and the slot.  For b = 0 .. B-1, while cnt > 0:
 *   trace   rt_internal_launch_rays of the list's cnt rays, flat (rows = cnt);
 *   query   rt_internal_launch_hits of the same rays (left out at bounce B-1 with emitters == 1);
 *   count   (not at bounce B-1) one lane an entry decides whether its path goes on -- four words of its record, its object's kd,
 *           T at its slot, at bounce 0 its record's liveness -- and a ballot and a population count per wavefront give each
 *           workgroup's number;
 *   scan    rt_mirror_compact.hip's instantiation of rt_scan.h's two-level exclusive scan (rt_internal_mirror_compact_scan);
 *   step    one lane an entry: the mask, the accumulation at the slot, and for a path that goes on T at the slot and its next
 *           ray and slot at place scan[workgroup] + its rank in the workgroup of the OTHER list: nothing is written where another
 *           lane may still be reading, and the next list is in path order again.  A path that ends writes nothing more: being on
 *           the list is what "alive" means here;
 *   -- unless b == B-1 the host waits for the stream and reads the total: the next bounce's cnt --
 * and the resolve, rt_paths_body.h's, over the m records.  The total is copied to pinned memory between the scan and the step, so
 * the step is the last thing the wait waits for.  The count and the step decide by the same function of the same words
 * (rt_paths_decide), so the ranks the step derives are those the count counted.  No workgroup waits for another anywhere: every
 * dependency is the stream's order.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_paths_compact.h"
#include "rt_host.h"
#include "rt_paths_body.h"
#include "rt_scan.h"

#pragma clang fp contract(off)

static_assert(sizeof(rt_paths_params) == 32, "rt_paths.h: rt_paths_params");
static_assert(sizeof(rt_paths_compact_info) == 136 && offsetof(rt_paths_compact_info, records) == 0 &&
              offsetof(rt_paths_compact_info, rays) == 8 && offsetof(rt_paths_compact_info, chunks) == 16 &&
              offsetof(rt_paths_compact_info, traces) == 20 && offsetof(rt_paths_compact_info, queries) == 24 &&
              offsetof(rt_paths_compact_info, syncs) == 28 && offsetof(rt_paths_compact_info, raygen_ms) == 32 &&
              offsetof(rt_paths_compact_info, trace_ms) == 40 && offsetof(rt_paths_compact_info, query_ms) == 48 &&
              offsetof(rt_paths_compact_info, step_ms) == 56 && offsetof(rt_paths_compact_info, resolve_ms) == 64 &&
              offsetof(rt_paths_compact_info, alive) == 72, "rt_paths_compact.h: rt_paths_compact_info");
static_assert(sizeof(rt_hit) == 48, "rt_capi_query.h layout");

namespace {

constexpr int kBlock = kPathsBlock;                    /* entries a workgroup */
static_assert(kBlock == kRankBlock, "rt_scan_rank's workgroup");
constexpr size_t kChunkBytes = (size_t)256 << 20;      /* the default chunk: its scratch within 256 MiB */
/* a path's scratch: in each of the two lists a ray and a slot; a colour and a record per entry; T and acc at the slot; and,
 * reckoned as one byte, the 8 bytes per kBlock paths of the counts and their scan (and 8 per kBlock * kScanBlock of the groups') */
constexpr size_t kPathBytes = 2 * (24 + 4) + 12 + 48 + 12 + 12 + 1;
static_assert(kPathBytes == 141, "the figure include/rt_paths_compact.h states");
constexpr size_t kCountWords = (size_t)kPathsCountSlots * kPathsCountStride;   /* alive[0]'s partial counts, 64-bit words */

} // namespace

/* Of a list's cnt entries, the paths that go on, per workgroup of the step kernel.  Entry e's record is gather[12 e ..], of which
 * the object (word 0), the colour (8 .. 10) and the flags (11) are read; its throughput is T[3 r ..] at its slot r = idx[e].
 * FIRST: r = e, T is (1, 1, 1) and not read, and an entry whose record hits[e / S] is dead does not go on and reads nothing else.
 * Lanes past the end count as ended and read nothing. */
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void rt_paths_compact_count_kernel(uint32_t cnt, uint32_t S, float gain,
                                                                        const int32_t *__restrict__ hits,
                                                                        const float *__restrict__ gather,
                                                                        const float *__restrict__ kd, int n_objects,
                                                                        const float *__restrict__ T, const uint32_t *__restrict__ idx,
                                                                        uint32_t *__restrict__ counts) {
    __shared__ uint32_t wave_count[kBlock / 64];
    const uint32_t e = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    bool on = false;
    if (e < cnt) {
        float Tx = 1.0f, Ty = 1.0f, Tz = 1.0f;
        bool live = true;
        if (FIRST) {
            live = rt_paths_record_live(hits, e / S);
        } else {
            const size_t r = idx[e];
            Tx = T[3 * r], Ty = T[3 * r + 1], Tz = T[3 * r + 2];
        }
        if (live) {
            const float *w = gather + 12 * (size_t)e;
            on = rt_paths_decide(__float_as_int(w[0]), __float_as_int(w[11]), w[8], w[9], w[10], kd, n_objects, gain, Tx, Ty, Tz).goes_on;
        }
    }
    uint32_t count;
    (void)rt_scan_rank(on, wave_count, &count);
    if (threadIdx.x == 0u) counts[blockIdx.x] = count;
}

/* The step after bounce b of the cnt entries of a chunk's dense list, one lane an entry (e < cnt < 2^31).  The list holds the
 * paths still alive, in path order: entry e is the path at slot r = idx_from[e] of the chunk (FIRST: r = e, the list is the chunk;
 * a dead record's path is on it and has acc = 0 written).  colours[3 e ..] and gather[3 e ..] (three float4) are what the bounce's
 * ray batch and hit query returned for the entry's ray; T[3 r ..] and acc[3 r ..] are the path's own, read and written by this
 * lane alone.  FIRST: T and acc are not read -- T_0 = 1 and acc = colour_0.  LAST (b == B-1): the colour is masked and
 * accumulated and nothing else is read or written; gather may then be NULL (emitters == 1: no query was launched).  Otherwise
 * a path that goes on (rt_paths_decide) stores T_{b+1} at its slot and writes its next ray and r to place p of rays_to and idx_to
 * -- the OTHER list, never the one being read -- where p = group_base[blk / kScanBlock] + offsets[blk] + the lane's rank among
 * workgroup blk's paths that go on; the counts scanned are rt_paths_compact_count_kernel's, which decides by the same function of
 * the same words.  The next ray's hash is keyed by key + r, the SLOT, as rt_paths.hip's is.  A path that ends writes nothing
 * more.  FIRST adds the live paths to alive's kPathsCountSlots partial counts.  p < the scan's total <= cnt <= the lists' size;
 * every address is the entry's, its slot's, its object's kd (object < n_objects is checked first) or its place's own.  Every
 * offset is 64-bit. */
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kBlock) void rt_paths_compact_step_kernel(
    uint32_t cnt, uint32_t S, int emitters, float gain, uint32_t seed, uint32_t key, const int32_t *__restrict__ hits,
    const float *__restrict__ colours, const float4 *__restrict__ gather, const float *__restrict__ kd, int n_objects,
    float *__restrict__ T, float *__restrict__ acc, const uint32_t *__restrict__ idx_from, float *__restrict__ rays_to,
    uint32_t *__restrict__ idx_to, const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ group_base,
    unsigned long long *__restrict__ alive) {
    __shared__ uint32_t wave_count[kBlock / 64];
    const uint32_t e = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const bool in = e < cnt;
    uint32_t r = e;
    bool live = in;
    if (in) {
        if (FIRST) live = rt_paths_record_live(hits, e / S);
        else r = idx_from[e];
    }
    if (FIRST) {
        const unsigned long long mask = __ballot(live);
        if ((threadIdx.x & 63u) == 0 && mask != 0) {
            const uint32_t wave = blockIdx.x * (uint32_t)(kBlock / 64) + (threadIdx.x >> 6);
            atomicAdd(alive + (size_t)(wave & (kPathsCountSlots - 1u)) * kPathsCountStride, (unsigned long long)__popcll(mask));
        }
    }
    float *t = T + 3 * (size_t)r, *a = acc + 3 * (size_t)r;
    float4 q0 = {}, q1 = {}, q2 = {};
    int32_t flags = 0;
    RtPathsDecision d = {false, 0.0f, 0.0f, 0.0f};
    if (live) {
        float Tx = 1.0f, Ty = 1.0f, Tz = 1.0f;
        if (!FIRST) Tx = t[0], Ty = t[1], Tz = t[2];
        const float cx = colours[3 * (size_t)e], cy = colours[3 * (size_t)e + 1], cz = colours[3 * (size_t)e + 2];
        if (LAST) {
            if (!emitters) q2.w = gather[3 * (size_t)e + 2].w;
        } else {
            const float4 *src = gather + 3 * (size_t)e;
            q0 = src[0], q1 = src[1], q2 = src[2];
        }
        flags = __float_as_int(q2.w);
        rt_paths_accumulate<FIRST>(cx, cy, cz, flags, emitters, Tx, Ty, Tz, a);
        if (!LAST) d = rt_paths_decide(__float_as_int(q0.x), flags, q2.x, q2.y, q2.z, kd, n_objects, gain, Tx, Ty, Tz);
    } else if (FIRST && in) {
        a[0] = 0.0f, a[1] = 0.0f, a[2] = 0.0f;                               /* a dead record's path */
    }
    if (LAST) return;
    uint32_t count;                                                          /* (every lane of the workgroup ranks) */
    uint32_t p = rt_scan_rank(d.goes_on, wave_count, &count);
    if (!d.goes_on) return;
    p += group_base[blockIdx.x / (uint32_t)kScanBlock] + offsets[blockIdx.x];
    t[0] = d.Tx, t[1] = d.Ty, t[2] = d.Tz;
    idx_to[p] = r;
    rt_paths_next_ray(q0, q1, flags, seed, key, r, rays_to + 6 * (size_t)p);
}

/* the resolve of the m records of a chunk: rt_paths_body.h's rt_paths_resolve, the grid ceil(m / (kPathsResolveSamples / S)) */
__global__ __launch_bounds__(kBlock) void rt_paths_compact_resolve_kernel(uint32_t m, int S, float gain, const float *__restrict__ acc,
                                                                          const int32_t *__restrict__ hits,
                                                                          const float *__restrict__ kd, int n_objects,
                                                                          const float *base, float *out) {
    __shared__ float lds[rt_paths_lds_floats()];
    rt_paths_resolve(lds, m, S, gain, acc, hits, kd, n_objects, base, out);
}

namespace {

/* kIdle: from a bounce's last kernel to the next thing enqueued after the host's wait -- in no stage */
enum Stage { kRaygen, kTrace, kQuery, kStep, kResolve, kIdle, kStages };

/* the handle's scratch, which only grows, and the last call's bookkeeping */
struct RtPathsCompactState {
    Buffer rays[2], idx[2];                                /* the two lists: a ray and a slot an entry */
    Buffer colours, gather;                                /* a bounce's colours and records, one per entry */
    Buffer T, acc;                                         /* a chunk's paths' throughputs and sums, at their slots */
    Buffer counts;                                         /* the counts and their scans */
    Buffer counters;                                       /* kCountWords 64-bit words of the last call: alive[0]'s partial counts */
    uint32_t *d_total = nullptr, *h_total = nullptr;       /* the paths that go on: on the device, and pinned */
    StageClock clock;                                      /* the last call's start, then one event after every stage */
    std::vector<uint8_t> stage_of;                         /* which Stage interval i of the clock is */
    rt_paths_compact_info info{};
    ~RtPathsCompactState() {
        clock.release();
        if (d_total) (void)hipFree(d_total);
        if (h_total) (void)hipHostFree(h_total);
    }
};

unsigned blocks_of(uint32_t n) { return (n + (uint32_t)kBlock - 1u) / (uint32_t)kBlock; }

/* the last call's stage times from its events and alive[0] from the device, once */
int collect(RtPathsCompactState *a) {
    if (a->clock.collected) return RT_OK;
    std::vector<float> t;
    const int rc = a->clock.intervals(&t);
    if (rc) return rc;
    double ms[kStages] = {};
    for (size_t i = 0; i < t.size() && i < a->stage_of.size(); ++i) ms[a->stage_of[i]] += t[i];
    a->info.raygen_ms = ms[kRaygen], a->info.trace_ms = ms[kTrace], a->info.query_ms = ms[kQuery];
    a->info.step_ms = ms[kStep], a->info.resolve_ms = ms[kResolve];
    /* (the call's last event has been waited for: its counts are final) */
    std::vector<unsigned long long> partial(kCountWords);
    HIP_TRY(hipMemcpy(partial.data(), a->counters.p, kCountWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long sum = 0;
    for (uint32_t k = 0; k < kPathsCountSlots; ++k) sum += partial[(size_t)k * kPathsCountStride];
    a->info.alive[0] = (int64_t)sum;
    return RT_OK;
}

void compact_free(void *state) { delete static_cast<RtPathsCompactState *>(state); }

double compact_ms(void *state, uint64_t seq) {
    RtPathsCompactState *a = static_cast<RtPathsCompactState *>(state);
    if (!a || a->clock.seq != seq || a->clock.n_events == 0 || collect(a) != RT_OK) return -1.0;
    return a->info.raygen_ms + a->info.trace_ms + a->info.query_ms + a->info.step_ms + a->info.resolve_ms;
}

RtPathsCompactState *state_of(rt_scene *s) {
    return unit_state<RtPathsCompactState>(s, RT_INTERNAL_UNIT_PATHS_COMPACT, compact_free, compact_ms);
}

struct StepArgs {                                          /* what every step of a chunk is launched with */
    uint32_t S;
    int emitters;
    float gain;
    uint32_t key;
    const int32_t *hits;
    const float *colours;
    const float4 *gather;
    const float *kd;
    int n_objects;
    float *T, *acc;
    const uint32_t *offsets, *group_base;
    unsigned long long *alive;
};

template <bool FIRST, bool LAST>
void launch_step(uint32_t cnt, uint32_t seed, const StepArgs &g, bool queried, const void *idx_from, void *rays_to, void *idx_to,
                 hipStream_t stream) {
    hipLaunchKernelGGL((rt_paths_compact_step_kernel<FIRST, LAST>), dim3(blocks_of(cnt)), dim3(kBlock), 0, stream, cnt, g.S, g.emitters,
                       g.gain, seed, g.key, g.hits, g.colours, queried ? g.gather : nullptr, g.kd, g.n_objects, g.T, g.acc,
                       static_cast<const uint32_t *>(idx_from), static_cast<float *>(rays_to), static_cast<uint32_t *>(idx_to),
                       g.offsets, g.group_base, g.alive);
}

/* the call, every argument checked, the handle locked, n > 0: device memory, on stream, which is waited for.  The events of the
 * call before are recorded anew without being waited for: its stage times, if nobody asked for them, are lost. */
int run(rt_scene *s, const rt_paths_params &pr, int n, const void *d_hits, const void *d_base, void *d_out, hipStream_t stream) {
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    if (stream) {
        hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
        HIP_TRY(hipStreamIsCapturing(stream, &capturing));
        if (capturing != hipStreamCaptureStatusNone)
            return fail(RT_ERR_INVALID, "the stream is capturing: rt_indirect_paths_compact_device waits for its stream and cannot "
                                        "be recorded into a graph (rt_indirect_paths_device can)");
    }
    RtPathsCompactState *a = state_of(s);
    const int S = pr.samples * pr.samples, B = pr.bounces;
    const int chunk = rt_paths_chunk_records(pr, n, kPathBytes, kChunkBytes);
    const size_t most = (size_t)chunk * (size_t)S;                        /* paths of the largest chunk, the first: a list's size */
    const bool any_query = !pr.emitters || B > 1;
    const unsigned max_blocks = blocks_of((uint32_t)most), max_groups = (max_blocks + kScanBlock - 1) / kScanBlock;
    const float *d_kd = nullptr;
    int n_objects = 0;
    int rc = rt_internal_object_diffuse(s, &d_kd, &n_objects);
    if (rc == RT_OK) rc = a->rays[1].grow(most * 24);                     /* (the list bounce 0 reads: the ray generation's) */
    if (B > 1) {                                                          /* (no second list and no slots without a second bounce) */
        if (rc == RT_OK) rc = a->rays[0].grow(most * 24);
        for (int l = 0; l < 2; ++l)
            if (rc == RT_OK) rc = a->idx[l].grow(most * 4);
        if (rc == RT_OK) rc = a->counts.grow(((size_t)max_blocks + max_groups) * 8);   /* counts, offsets, the groups' sums and bases */
    }
    if (rc == RT_OK) rc = a->colours.grow(most * 12);
    if (rc == RT_OK && any_query) rc = a->gather.grow(most * 48);
    if (rc == RT_OK) rc = a->T.grow(most * 12);
    if (rc == RT_OK) rc = a->acc.grow(most * 12);
    if (rc == RT_OK) rc = a->counters.grow(sizeof(unsigned long long) * kCountWords);
    /* everything below writes scratch that the call before, on another stream, may not have finished with */
    if (rc == RT_OK) rc = rt_internal_order_stream(s, stream);
    if (rc) return rc;
    if (!a->d_total) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&a->d_total), 4));
    if (!a->h_total) HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&a->h_total), 4, hipHostMallocDefault));
    uint32_t *counts = static_cast<uint32_t *>(a->counts.p), *offsets = nullptr, *group_sums = nullptr, *group_base = nullptr;
    if (B > 1) offsets = counts + max_blocks, group_sums = offsets + max_blocks, group_base = group_sums + max_groups;
    a->clock.n_events = 0;
    a->clock.collected = true;
    a->stage_of.clear();
    a->info = rt_paths_compact_info{};
    a->info.records = n;
    unsigned long long *counters = static_cast<unsigned long long *>(a->counters.p);
    HIP_TRY(hipMemsetAsync(counters, 0, sizeof(unsigned long long) * kCountWords, stream));
    if ((rc = a->clock.mark(stream))) return rc;
    auto stage = [&](Stage which) {
        a->stage_of.push_back((uint8_t)which);
        return a->clock.mark(stream);
    };
    const unsigned group = (unsigned)(kPathsResolveSamples / S);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - i0);
        const uint32_t total = m * (uint32_t)S;                           /* <= kPathsMaxBatchRays */
        const char *hits = static_cast<const char *>(d_hits) + (size_t)i0 * 48;
        const uint32_t key = pr.key0 + (uint32_t)i0;                      /* the chunk's first record's; its first path's: */
        const StepArgs g = {(uint32_t)S, pr.emitters, pr.gain, key * (uint32_t)S, reinterpret_cast<const int32_t *>(hits),
                            static_cast<const float *>(a->colours.p), static_cast<const float4 *>(a->gather.p), d_kd, n_objects,
                            static_cast<float *>(a->T.p), static_cast<float *>(a->acc.p), offsets, group_base, counters};
        rc = rt_internal_indirect_raygen(pr.samples, pr.seed, key, m, hits, a->rays[1].p, stream);
        if (rc == RT_OK) rc = stage(kRaygen);
        if (rc) return rc;
        uint32_t cnt = total;
        for (int b = 0; b < B && cnt > 0; ++b) {
            const int to = b & 1, from = to ^ 1;                          /* the list this bounce writes, and the one it reads */
            const bool first = b == 0, last = b == B - 1, queried = !(last && pr.emitters);
            rc = rt_internal_launch_rays(s, (int)cnt, (int)cnt, a->rays[from].p, pr.gather_depth, a->colours.p, stream);
            if (rc == RT_OK) rc = stage(kTrace);
            if (rc) return rc;
            a->info.traces += 1;
            a->info.rays += (int64_t)cnt;
            if (!first) a->info.alive[b] += (int64_t)cnt;
            if (queried) {
                rc = rt_internal_launch_hits(s, (int)cnt, (int)cnt, a->rays[from].p, a->gather.p, stream);
                if (rc == RT_OK) rc = stage(kQuery);
                if (rc) return rc;
                a->info.queries += 1;
            }
            if (!last) {
                const unsigned n_blocks = blocks_of(cnt);
                auto count = first ? rt_paths_compact_count_kernel<true> : rt_paths_compact_count_kernel<false>;
                hipLaunchKernelGGL(count, dim3(n_blocks), dim3(kBlock), 0, stream, cnt, g.S, g.gain, g.hits,
                                   static_cast<const float *>(a->gather.p), d_kd, n_objects, static_cast<const float *>(a->T.p),
                                   static_cast<const uint32_t *>(a->idx[from].p), counts);
                HIP_TRY(hipGetLastError());
                if ((rc = rt_internal_mirror_compact_scan(counts, n_blocks, offsets, group_sums, group_base, a->d_total, stream))) return rc;
                HIP_TRY(hipMemcpyAsync(a->h_total, a->d_total, 4, hipMemcpyDeviceToHost, stream));
            }
            const uint32_t next_seed = pr.seed + (uint32_t)(b + 1) * kPathsGolden;
            auto step = first ? (last ? launch_step<true, true> : launch_step<true, false>)
                              : (last ? launch_step<false, true> : launch_step<false, false>);
            step(cnt, next_seed, g, queried, a->idx[from].p, a->rays[to].p, a->idx[to].p, stream);
            HIP_TRY(hipGetLastError());
            if ((rc = stage(kStep))) return rc;
            if (last) break;
            HIP_TRY(hipStreamSynchronize(stream));                        /* the bounce's one wait: how many rays the next trace has */
            a->info.syncs += 1;
            const uint32_t next = *a->h_total;
            if (next > cnt) return fail(RT_ERR_HIP, "rt_indirect_paths_compact: more paths go on than the bounce had");
            cnt = next;
            if ((rc = stage(kIdle))) return rc;
        }
        hipLaunchKernelGGL(rt_paths_compact_resolve_kernel, dim3((m + group - 1) / group), dim3(kBlock), 0, stream, m, S, pr.gain,
                           static_cast<const float *>(a->acc.p), reinterpret_cast<const int32_t *>(hits), d_kd, n_objects,
                           d_base ? static_cast<const float *>(d_base) + 3 * (size_t)i0 : nullptr,
                           static_cast<float *>(d_out) + 3 * (size_t)i0);
        HIP_TRY(hipGetLastError());
        if ((rc = stage(kResolve))) return rc;
        a->info.chunks += 1;
    }
    a->clock.collected = false;
    a->clock.seq = rt_internal_launch_seq(s);
    return RT_OK;
}

} // namespace

extern "C" {

int rt_paths_compact_version(void) { return RT_PATHS_COMPACT_VERSION; }

int rt_indirect_paths_compact_device(rt_scene *s, const rt_paths_params *pr, int n, const void *d_hits, const void *d_base_rgb,
                                     void *d_out_rgb, void *hip_stream) {
    const int rc = rt_paths_check_args(s, pr, n, d_hits, d_base_rgb, d_out_rgb, true);
    if (rc || n == 0) return rc;
    const rt_paths_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    return run(s, p, n, d_hits, d_base_rgb, d_out_rgb, static_cast<hipStream_t>(hip_stream));
}

int rt_indirect_paths_compact(rt_scene *s, const rt_paths_params *pr, int n, const rt_hit *hits, const float *base_rgb,
                              float *out_rgb) {
    const int rc = rt_paths_check_args(s, pr, n, hits, base_rgb, out_rgb, false);
    if (rc || n == 0) return rc;
    const rt_paths_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    const HostIn in[2] = {{hits, (size_t)n * 48}, {base_rgb, (size_t)n * 12}};
    const HostOut out[1] = {{out_rgb, (size_t)n * 12}};
    return staged_call(rt_internal_scene_device(s), in, 2, out, 1, 0, nullptr, [&](void *const *d_in, void *const *d_out, void *) {
        return run(s, p, n, d_in[0], d_in[1], d_out[0], nullptr);
    });
}

int rt_get_paths_compact_info(const rt_scene *cs, rt_paths_compact_info *out) {
    if (!cs || !out) return fail(RT_ERR_INVALID, "scene/out is NULL");
    rt_scene *s = const_cast<rt_scene *>(cs);
    rt_internal_lock(s);
    Unlock unlock{s};
    RtPathsCompactState *a = static_cast<RtPathsCompactState *>(rt_internal_unit_slot(s, RT_INTERNAL_UNIT_PATHS_COMPACT)->state);
    if (!a) {
        *out = rt_paths_compact_info{};
        return RT_OK;
    }
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    const int rc = collect(a);
    if (rc) return rc;
    *out = a->info;
    return RT_OK;
}

} // extern "C"
