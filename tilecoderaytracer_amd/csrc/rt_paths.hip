/*
 * rt_paths.hip -- implementation of include/rt_paths.h: diffuse light paths of more than one bounce from hit records.  The
 * header is the definition; these kernels are bit-exact to it (the library's arithmetic flags: no contraction, correctly rounded
 * divide and square root, denormals kept).
 *
 * SHAPE, modelled on rt_indirect.hip.  Bounce 0's rays are rt_indirect.hip's ray generation
 * (rt_internal_indirect_raygen), every bounce's rays are traced and queried by rt_capi.hip's ray batch and hit query through
 * rt_internal.h.  Around them, here, per chunk of records:
 *   step     one lane a path, after every bounce's trace and query: the path's state is its slot of the chunk's five arrays --
 *            its ray (24 bytes), the ray's colour (12), the ray's record (48), its throughput T (12) and its sum acc (12), 108
 *            bytes a path.  A path that has ended is one whose stored T is (0, 0, 0): that is what the definition's third stop
 *            rule makes of it anyway, so aliveness costs no word of its own.  The step masks a light's colour, accumulates,
 *            multiplies T, decides, and writes the next ray (rt_capi_ao.h's arithmetic for n = 1, s = 0) or six zeros -- a text
 *            of its own, as rt_glass_step_kernel's is; rt_paths_body.h holds the same arithmetic as functions for
 *            rt_paths_compact.hip (THE STEP KEEPS ITS OWN TEXT, below, says why there are two).  The first step reads no T and no acc (T_0 = 1: the path lives if its
 *            record does), the last one writes neither T nor a ray.
 *   resolve  per record the sequential sum of its S paths' acc, the divide, the weight, the base: rt_indirect_resolve_kernel's
 *            arithmetic with no gather records.
 * Each step counts its live paths: one ballot a wavefront, one atomicAdd on one of the bounce's 128 partial 64-bit counters.
 * Nothing is read back: the launches depend on the arguments alone, and the call never waits for the device.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_paths.h"
#include "rt_host.h"
#include "rt_paths_body.h"

#pragma clang fp contract(off)

static_assert(sizeof(rt_paths_params) == 32 && offsetof(rt_paths_params, gain) == 24 && offsetof(rt_paths_params, bounces) == 28,
              "rt_paths.h: rt_paths_params");
static_assert(offsetof(rt_paths_params, samples) == offsetof(rt_indirect_params, samples) &&
              offsetof(rt_paths_params, gather_depth) == offsetof(rt_indirect_params, gather_depth) &&
              offsetof(rt_paths_params, chunk_records) == offsetof(rt_indirect_params, chunk_records) &&
              offsetof(rt_paths_params, emitters) == offsetof(rt_indirect_params, emitters) &&
              offsetof(rt_paths_params, seed) == offsetof(rt_indirect_params, seed) &&
              offsetof(rt_paths_params, key0) == offsetof(rt_indirect_params, key0) &&
              offsetof(rt_paths_params, gain) == offsetof(rt_indirect_params, gain), "rt_paths.h: rt_indirect_params' fields first");
static_assert(sizeof(rt_paths_info) == 128 && offsetof(rt_paths_info, records) == 0 && offsetof(rt_paths_info, rays) == 8 &&
              offsetof(rt_paths_info, chunks) == 16 && offsetof(rt_paths_info, raygen_ms) == 24 &&
              offsetof(rt_paths_info, trace_ms) == 32 && offsetof(rt_paths_info, query_ms) == 40 &&
              offsetof(rt_paths_info, step_ms) == 48 && offsetof(rt_paths_info, resolve_ms) == 56 &&
              offsetof(rt_paths_info, alive) == 64, "rt_paths.h: rt_paths_info");
static_assert(sizeof(rt_hit) == 48, "rt_capi_query.h layout");

namespace {

constexpr int kBlock = kPathsBlock;                    /* step: paths a workgroup; resolve: lanes a workgroup */
constexpr int kResolveSamples = kPathsResolveSamples;  /* resolve: paths a workgroup -- 1024 / S records */
constexpr int kMaxBounces = kPathsMaxBounces;          /* B */
constexpr size_t kPathBytes = 108;                     /* a path's scratch: ray 24, colour 12, record 48, T 12, acc 12 */
constexpr size_t kChunkBytes = (size_t)256 << 20;      /* the default chunk: its scratch within 256 MiB */
constexpr uint32_t kGolden = kPathsGolden;
constexpr uint32_t kCountSlots = kPathsCountSlots, kCountStride = kPathsCountStride;   /* alive[]'s partial counts (rt_paths_body.h) */
constexpr size_t kCountWords = (size_t)kMaxBounces * kCountSlots * kCountStride;

} // namespace

/* THE STEP KEEPS ITS OWN TEXT.  Its arithmetic -- the mask, the accumulation, the throughput, the stop rule, the next ray -- is
 * also rt_paths_body.h's rt_paths_accumulate, rt_paths_decide and rt_paths_next_ray, which rt_paths_compact.hip's kernels are made
 * of.  This kernel was written before them, and calling any of the three from it changed the instructions of its two
 * instantiations that are not LAST (the scheduler moved the multiplications and the key's addition; five forms were tried,
 * DESIGN.md section 35), so by the rule of DESIGN.md section 31 it stays as it was measured.  The two texts are held together by
 * tests/test_paths_compact_gpu.py, which compares the two units' outputs word for word on every frame. */
/* The step after bounce b of the `total` paths of a chunk (total < 2^31), one lane a path, path r = p S + s of the chunk at
 * slot r of every array: colours[3 r ..] and gather[3 r ..] (three float4: the record, read as three 16-byte loads a lane) are
 * what the bounce's ray batch and hit query returned for rays[6 r ..]; T[3 r ..] and acc[3 r ..] are the path's own.
 * FIRST (b == 0): T and acc are not read -- T_0 = 1 and acc = colour_0 -- and the path lives if its record hits[p] does.
 * LAST (b == B-1): the colour is masked and accumulated and nothing else is written; gather may then be NULL (emitters == 1:
 * no query was launched).  Otherwise the throughput is multiplied, stored -- (0, 0, 0) for a path that ends here, which is how a
 * later step knows it -- and the next ray written: from the record g with the hash H(H(seed ^ golden) ^ (key + r)), seed the
 * NEXT bounce's and key the chunk's first path's key, or six zeros.  The paths alive at this bounce are added to alive's
 * kCountSlots partial counts. */
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kBlock) void rt_paths_step_kernel(uint32_t total, uint32_t S, int emitters, float gain, uint32_t seed,
                                                               uint32_t key, const int32_t *__restrict__ hits,
                                                               const float *__restrict__ colours, const float4 *__restrict__ gather,
                                                               const float *__restrict__ kd, int n_objects, float *__restrict__ T,
                                                               float *__restrict__ acc, float *__restrict__ rays,
                                                               unsigned long long *__restrict__ alive) {
    const uint32_t r = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    const bool in = r < total;
    float Tx = 1.0f, Ty = 1.0f, Tz = 1.0f;
    bool live = false;
    if (in) {
        if (FIRST) {
            const int32_t *h = hits + (size_t)(r / S) * kPathsHitWords;
            live = h[0] >= 0 && (h[kPathsHitFlagsWord] & RT_HIT_LIGHT) == 0;
        } else {
            Tx = T[3 * (size_t)r], Ty = T[3 * (size_t)r + 1], Tz = T[3 * (size_t)r + 2];
            live = !(Tx == 0.0f && Ty == 0.0f && Tz == 0.0f);
        }
    }
    const unsigned long long mask = __ballot(live);
    if ((threadIdx.x & 63u) == 0 && mask != 0) {
        const uint32_t wave = blockIdx.x * (uint32_t)(kBlock / 64) + (threadIdx.x >> 6);
        atomicAdd(alive + (size_t)(wave & (kCountSlots - 1u)) * kCountStride, (unsigned long long)__popcll(mask));
    }
    if (!in) return;
    float *t = T + 3 * (size_t)r, *a = acc + 3 * (size_t)r, *o = rays + 6 * (size_t)r;
    if (!live) {
        /* a later step: the path's T is zero and its ray was zeroed when it ended.  The first: a dead record's path */
        if (FIRST) {
            a[0] = 0.0f, a[1] = 0.0f, a[2] = 0.0f;
            if (!LAST) t[0] = 0.0f, t[1] = 0.0f, t[2] = 0.0f;     /* (its rays are zeros already: the ray generation's) */
        }
        return;
    }
    float cx = colours[3 * (size_t)r], cy = colours[3 * (size_t)r + 1], cz = colours[3 * (size_t)r + 2];
    float4 q0 = {}, q1 = {}, q2 = {};
    if (LAST) {
        if (!emitters) q2.w = gather[3 * (size_t)r + 2].w;
    } else {
        const float4 *src = gather + 3 * (size_t)r;
        q0 = src[0], q1 = src[1], q2 = src[2];
    }
    const int32_t flags = __float_as_int(q2.w);
    const bool light = (flags & RT_HIT_LIGHT) != 0;
    if (!emitters && light) cx = 0.0f, cy = 0.0f, cz = 0.0f;
    if (FIRST) {
        a[0] = cx, a[1] = cy, a[2] = cz;
    } else {
        a[0] = a[0] + Tx * cx, a[1] = a[1] + Ty * cy, a[2] = a[2] + Tz * cz;
    }
    if (LAST) return;
    const int32_t object = __float_as_int(q0.x);
    const float k = object >= 0 && object < n_objects ? kd[object] : 0.0f;
    Tx = Tx * ((q2.x * k) * gain), Ty = Ty * ((q2.y * k) * gain), Tz = Tz * ((q2.z * k) * gain);
    if (object < 0 || light || (Tx == 0.0f && Ty == 0.0f && Tz == 0.0f)) {
        t[0] = 0.0f, t[1] = 0.0f, t[2] = 0.0f;
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = 0.0f;
        return;
    }
    t[0] = Tx, t[1] = Ty, t[2] = Tz;
    /* the record's frame: rt_indirect_raygen_kernel's arithmetic (ao_tile()'s, rt_kernel.hip), operation for operation */
    const float Px = q0.z, Py = q0.w, Pz = q1.x;
    const bool flip = (flags & RT_HIT_INSIDE) != 0;
    const float Nx = flip ? -q1.y : q1.y, Ny = flip ? -q1.z : q1.z, Nz = flip ? -q1.w : q1.w;
    const bool ax = fabsf(Nx) < 0.5f;
    const float Ax = ax ? 1.0f : 0.0f, Ay = ax ? 0.0f : 1.0f, Az = 0.0f;
    const float ux = Ay * Nz - Az * Ny, uy = Az * Nx - Ax * Nz, uz = Ax * Ny - Ay * Nx;
    const float len = sqrtf(ux * ux + uy * uy + uz * uz);
    const float Ux = ux / len, Uy = uy / len, Uz = uz / len;
    const float Vx = Ny * Uz - Nz * Uy, Vy = Nz * Ux - Nx * Uz, Vz = Nx * Uy - Ny * Ux;
    /* the one sample of n = 1: s = 0, i = j = 0, step = 2 / 1 */
    const uint32_t hs = rt_paths_hash(rt_paths_hash(rt_paths_hash(seed ^ kGolden) ^ (key + r)) ^ 0u);
    const float xi1 = (float)(hs >> 8) * 0x1p-24f;
    const float xi2 = (float)(rt_paths_hash(hs ^ kGolden) >> 8) * 0x1p-24f;
    const float step = 2.0f / 1.0f;
    const float pa = (0.0f + xi1) * step - 1.0f, pb = (0.0f + xi2) * step - 1.0f;
    const float dx = pa * sqrtf(1.0f - (pb * pb) * 0.5f), dy = pb * sqrtf(1.0f - (pa * pa) * 0.5f);
    const float w = (1.0f - dx * dx) - dy * dy;
    const float dz = w > 0.0f ? sqrtf(w) : 0.0f;
    const float Dx = (Ux * dx + Vx * dy) + Nx * dz, Dy = (Uy * dx + Vy * dy) + Ny * dz, Dz = (Uz * dx + Vz * dy) + Nz * dz;
    o[0] = Px, o[1] = Py, o[2] = Pz;
    o[3] = Px + Dx, o[4] = Py + Dy, o[5] = Pz + Dz;
}

/* the resolve of the m records of a chunk: rt_paths_body.h's rt_paths_resolve, the grid ceil(m / (kResolveSamples / S)) */
__global__ __launch_bounds__(kBlock) void rt_paths_resolve_kernel(uint32_t m, int S, float gain, const float *__restrict__ acc,
                                                                  const int32_t *__restrict__ hits, const float *__restrict__ kd,
                                                                  int n_objects, const float *base, float *out) {
    __shared__ float lds[rt_paths_lds_floats()];
    rt_paths_resolve(lds, m, S, gain, acc, hits, kd, n_objects, base, out);
}

namespace {

enum Stage { kRaygen, kTrace, kQuery, kStep, kResolve, kStages };

/* the handle's scratch, which only grows, and the last call's bookkeeping */
struct RtPathsState {
    Buffer rays, colours, gather, T, acc;                  /* a chunk's paths: 24 + 12 + 48 + 12 + 12 bytes each */
    Buffer counters;                                       /* kCountWords 64-bit words of the last call: alive[]'s partial counts */
    Buffer hits, out_rgb;                                  /* the host variant's records and its base / output */
    StageClock clock;                                      /* the last call's start, then one event after every stage */
    std::vector<uint8_t> stage_of;                         /* which Stage interval i of the clock is */
    rt_paths_info info{};
    ~RtPathsState() { clock.release(); }
};

unsigned blocks_of(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

/* the records a launch gathers for (rt_paths_body.h) */
int chunk_records(const rt_paths_params &pr, int n) { return rt_paths_chunk_records(pr, n, kPathBytes, kChunkBytes); }

/* the last call's stage times from its events and its counts from the device, once */
int collect(RtPathsState *a) {
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
    for (int b = 0; b < kMaxBounces; ++b) {
        unsigned long long sum = 0;
        for (uint32_t k = 0; k < kCountSlots; ++k) sum += partial[((size_t)b * kCountSlots + k) * kCountStride];
        a->info.alive[b] = (int64_t)sum;
    }
    return RT_OK;
}

void paths_free(void *state) { delete static_cast<RtPathsState *>(state); }

double paths_ms(void *state, uint64_t seq) {
    RtPathsState *a = static_cast<RtPathsState *>(state);
    if (!a || a->clock.seq != seq || a->clock.n_events == 0 || collect(a) != RT_OK) return -1.0;
    return a->info.raygen_ms + a->info.trace_ms + a->info.query_ms + a->info.step_ms + a->info.resolve_ms;
}

RtPathsState *state_of(rt_scene *s) { return unit_state<RtPathsState>(s, RT_INTERNAL_UNIT_PATHS, paths_free, paths_ms); }

template <bool FIRST, bool LAST>
void launch_step(uint32_t total, uint32_t S, const rt_paths_params &pr, uint32_t seed, uint32_t key, const void *hits,
                 const RtPathsState *a, bool queried, const float *d_kd, int n_objects, unsigned long long *alive, hipStream_t stream) {
    hipLaunchKernelGGL((rt_paths_step_kernel<FIRST, LAST>), dim3(blocks_of(total)), dim3(kBlock), 0, stream, total, S, pr.emitters,
                       pr.gain, seed, key, static_cast<const int32_t *>(hits), static_cast<const float *>(a->colours.p),
                       queried ? static_cast<const float4 *>(a->gather.p) : nullptr, d_kd, n_objects, static_cast<float *>(a->T.p),
                       static_cast<float *>(a->acc.p), static_cast<float *>(a->rays.p), alive);
}

/* the call, every argument checked, the handle locked, n > 0: device memory, on stream.  The events of the call before are
 * recorded anew without being waited for: its stage times, if nobody asked for them, are lost. */
int run(rt_scene *s, const rt_paths_params &pr, int n, const void *d_hits, const void *d_base, void *d_out, hipStream_t stream) {
    RtPathsState *a = state_of(s);
    const int S = pr.samples * pr.samples, B = pr.bounces;
    const int chunk = chunk_records(pr, n);
    const size_t most = (size_t)chunk * (size_t)S;                        /* paths of the largest chunk, the first */
    const bool any_query = !pr.emitters || B > 1;
    const float *d_kd = nullptr;
    int n_objects = 0;
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    int rc = rt_internal_object_diffuse(s, &d_kd, &n_objects);
    if (rc == RT_OK) rc = a->rays.grow(most * 24);
    if (rc == RT_OK) rc = a->colours.grow(most * 12);
    if (rc == RT_OK && any_query) rc = a->gather.grow(most * 48);
    if (rc == RT_OK) rc = a->T.grow(most * 12);
    if (rc == RT_OK) rc = a->acc.grow(most * 12);
    if (rc == RT_OK) rc = a->counters.grow(sizeof(unsigned long long) * kCountWords);
    /* everything below writes scratch that the call before, on another stream, may not have finished with */
    if (rc == RT_OK) rc = rt_internal_order_stream(s, stream);
    if (rc) return rc;
    a->clock.n_events = 0;
    a->clock.collected = true;
    a->stage_of.clear();
    a->info = rt_paths_info{};
    a->info.records = n;
    unsigned long long *counters = static_cast<unsigned long long *>(a->counters.p);
    HIP_TRY(hipMemsetAsync(counters, 0, sizeof(unsigned long long) * kCountWords, stream));
    if ((rc = a->clock.mark(stream))) return rc;
    auto stage = [&](Stage which) {
        a->stage_of.push_back((uint8_t)which);
        return a->clock.mark(stream);
    };
    const unsigned group = (unsigned)(kResolveSamples / S);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - i0);
        const uint32_t total = m * (uint32_t)S;                           /* <= kPathsMaxBatchRays */
        const int n_rays = (int)total;
        const char *hits = static_cast<const char *>(d_hits) + (size_t)i0 * 48;
        const uint32_t key = pr.key0 + (uint32_t)i0;                      /* the chunk's first record's; its first path's: */
        const uint32_t path_key = key * (uint32_t)S;
        rc = rt_internal_indirect_raygen(pr.samples, pr.seed, key, m, hits, a->rays.p, stream);
        if (rc == RT_OK) rc = stage(kRaygen);
        for (int b = 0; b < B && rc == RT_OK; ++b) {
            const bool last = b == B - 1, queried = !(last && pr.emitters);
            rc = rt_internal_launch_rays(s, n_rays, n_rays, a->rays.p, pr.gather_depth, a->colours.p, stream);
            if (rc == RT_OK) rc = stage(kTrace);
            if (rc == RT_OK && queried) {
                rc = rt_internal_launch_hits(s, n_rays, n_rays, a->rays.p, a->gather.p, stream);
                if (rc == RT_OK) rc = stage(kQuery);
            }
            if (rc) break;
            const uint32_t next_seed = pr.seed + (uint32_t)(b + 1) * kGolden;
            if (b == 0 && last) launch_step<true, true>(total, S, pr, next_seed, path_key, hits, a, queried, d_kd, n_objects, counters + (size_t)b * kCountSlots * kCountStride, stream);
            else if (b == 0) launch_step<true, false>(total, S, pr, next_seed, path_key, hits, a, queried, d_kd, n_objects, counters + (size_t)b * kCountSlots * kCountStride, stream);
            else if (last) launch_step<false, true>(total, S, pr, next_seed, path_key, hits, a, queried, d_kd, n_objects, counters + (size_t)b * kCountSlots * kCountStride, stream);
            else launch_step<false, false>(total, S, pr, next_seed, path_key, hits, a, queried, d_kd, n_objects, counters + (size_t)b * kCountSlots * kCountStride, stream);
            HIP_TRY(hipGetLastError());
            rc = stage(kStep);
            a->info.rays += (int64_t)n_rays;
        }
        if (rc) return rc;
        hipLaunchKernelGGL(rt_paths_resolve_kernel, dim3((m + group - 1) / group), dim3(kBlock), 0, stream, m, S, pr.gain,
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

int rt_paths_version(void) { return RT_PATHS_VERSION; }

int rt_indirect_paths_device(rt_scene *s, const rt_paths_params *pr, int n, const void *d_hits, const void *d_base_rgb, void *d_out_rgb,
                             void *hip_stream) {
    const int rc = rt_paths_check_args(s, pr, n, d_hits, d_base_rgb, d_out_rgb, true);
    if (rc || n == 0) return rc;
    const rt_paths_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    return run(s, p, n, d_hits, d_base_rgb, d_out_rgb, static_cast<hipStream_t>(hip_stream));
}

int rt_indirect_paths(rt_scene *s, const rt_paths_params *pr, int n, const rt_hit *hits, const float *base_rgb, float *out_rgb) {
    int rc = rt_paths_check_args(s, pr, n, hits, base_rgb, out_rgb, false);
    if (rc || n == 0) return rc;
    const rt_paths_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    RtPathsState *a = state_of(s);
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    rc = a->hits.grow((size_t)n * 48);
    if (rc == RT_OK) rc = a->out_rgb.grow((size_t)n * 12);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(a->hits.p, hits, (size_t)n * 48, hipMemcpyHostToDevice));
    if (base_rgb) HIP_TRY(hipMemcpy(a->out_rgb.p, base_rgb, (size_t)n * 12, hipMemcpyHostToDevice));
    /* (the base, if any, is gathered onto in place) */
    if ((rc = run(s, p, n, a->hits.p, base_rgb ? a->out_rgb.p : nullptr, a->out_rgb.p, nullptr))) return rc;
    HIP_TRY(hipMemcpy(out_rgb, a->out_rgb.p, (size_t)n * 12, hipMemcpyDeviceToHost));
    HIP_TRY(hipDeviceSynchronize());
    return RT_OK;
}

int rt_get_paths_info(const rt_scene *cs, rt_paths_info *out) {
    if (!cs || !out) return fail(RT_ERR_INVALID, "scene/out is NULL");
    rt_scene *s = const_cast<rt_scene *>(cs);
    rt_internal_lock(s);
    Unlock unlock{s};
    RtPathsState *a = static_cast<RtPathsState *>(rt_internal_unit_slot(s, RT_INTERNAL_UNIT_PATHS)->state);
    if (!a) {
        *out = rt_paths_info{};
        return RT_OK;
    }
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    const int rc = collect(a);
    if (rc) return rc;
    *out = a->info;
    return RT_OK;
}

} // extern "C"
