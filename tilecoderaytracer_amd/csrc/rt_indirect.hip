/*
 * rt_indirect.hip -- implementation of include/rt_capi_indirect.h: one diffuse bounce from hit records.  The header is the
 * definition; these kernels are bit-exact to it (the library's arithmetic flags: no contraction, correctly rounded divide and
 * square root, denormals kept).
 *
 * SHAPE, modelled on rt_lens.hip.  The render and query kernels are rt_capi.hip's: every gather ray is
 * traced by its ray-batch launch and, with emitters == 0, asked for its first hit by its hit query, through rt_internal.h --
 * every launch decision stays there.  Around them, here, per chunk of records:
 *   raygen   one lane per sample: the record's frame and hash once per record through LDS, the sample's direction
 *            (include/rt_capi_ao.h) -> {P, P + D}, 24 bytes a lane, consecutive lanes consecutive rays; a dead record's lanes
 *            write zeros;
 *   trace    rt_internal_launch_rays, one flat list (rows = the chunk's rays: the layout profiles/lens_experiments.txt kept);
 *   query    emitters == 0 only: rt_internal_launch_hits of the same rays;
 *   resolve  per record the sequential sum of its S colours -- those whose gather record is a light as zeros -- the divide,
 *            the weight, the base, stored once at the record's place.
 * Nothing is read back: the launches depend on the arguments alone, and the call never waits for the device.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_capi_indirect.h"
#include "rt_host.h"

#pragma clang fp contract(off)

static_assert(sizeof(rt_indirect_params) == 28 && sizeof(rt_indirect_info) == 56, "rt_capi_indirect.h layouts");
static_assert(sizeof(rt_hit) == 48, "rt_capi_query.h layout");

namespace {

constexpr int kBlock = 256;                            /* raygen: rays a workgroup; resolve: lanes a workgroup */
constexpr int kResolveSamples = 1024;                  /* resolve: samples a workgroup -- 1024 / S records */
constexpr int kMaxSamples = RT_INDIRECT_MAX_SAMPLES;   /* n */
constexpr size_t kChunkBytes = (size_t)256 << 20;      /* the default chunk: its scratch within 256 MiB */
constexpr long long kMaxBatchRays = 0x7fffffffLL - 64; /* rt_trace_rays' grid limit for a flat list (include/rt_capi_rays.h) */
constexpr double kMaxRayFloats = 2.0e9 * 4.0;          /* rt_render's limit for one output, in floats */
constexpr int kMaxRecords = 533333333;                 /* rt_render_gbuffer's record limit */
constexpr int kHitWords = 12, kHitFlagsWord = 11;      /* an rt_hit in 4-byte words; its flags (byte 44) */
constexpr int kFrameStride = 15;                       /* raygen: a record's 14 words in LDS (P, N, U, V, hash, live), odd stride */

/* resolve: a record's 3 S floats in LDS, padded to an odd stride so that the sums' reads spread over the banks */
constexpr int lds_stride(int S) { return (3 * S) | 1; }
constexpr int lds_floats() {
    int most = 0;
    for (int n = 1; n <= kMaxSamples; ++n) most = std::max(most, (kResolveSamples / (n * n)) * lds_stride(n * n));
    return most;
}
static_assert(lds_floats() * 4 <= 16384, "resolve: LDS");

} // namespace

/* the 32-bit integer hash "lowbias32" (include/rt_capi_soft.h) */
__device__ __forceinline__ uint32_t rt_indirect_hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

/* Ray r = p S + s of a chunk of m records (m S rays, r < 2^31): {P, T} of the header at rays[6 r ..]; record p of the chunk
 * samples with key + p.  One lane per sample, consecutive lanes consecutive rays.  What the S samples of a record share -- its 48
 * bytes, P, N, the tangent frame U, V (a square root and three divides) and the record's hash -- is made once per record: the
 * workgroup's 256 rays belong to at most 256 / S + 2 records (S is no power of two for n = 3, 5, 6, 7: a record's lanes straddle
 * wavefronts and workgroups), one lane each reads its record as three 16-byte loads and leaves the 14 words in LDS, on an odd
 * stride; after the barrier every lane reads its record's words from there and computes its own sample alone.  (One lane per
 * sample computing all of it measured 1.44 - 1.72 times rt_lens_raygen_kernel at n = 4, where the traffic is 1.125 times:
 * profiles/indirect_experiments.txt.)  The arithmetic is ao_tile()'s (rt_kernel.hip), operation for operation. */
__global__ __launch_bounds__(kBlock) void rt_indirect_raygen_kernel(uint32_t m, int n, uint32_t seed, uint32_t key,
                                                                    const float4 *__restrict__ hits, float *__restrict__ rays) {
    __shared__ uint32_t frames[kBlock * kFrameStride];
    const uint32_t S = (uint32_t)(n * n), total = m * S;
    const uint32_t r0 = blockIdx.x * (uint32_t)kBlock;                    /* (r0 < total: the grid is ceil(total / kBlock)) */
    const uint32_t p0 = r0 / S, p1 = (min(r0 + (uint32_t)kBlock, total) - 1u) / S;       /* the workgroup's records, p1 < m */
    if (threadIdx.x <= p1 - p0) {                                         /* (p1 - p0 < kBlock: no more records than rays) */
        const float4 *src = hits + (size_t)(p0 + threadIdx.x) * 3;
        const float4 q0 = src[0], q1 = src[1], q2 = src[2];
        const bool live = __float_as_int(q0.x) >= 0 && (__float_as_int(q2.w) & RT_HIT_LIGHT) == 0;
        const bool flip = (__float_as_int(q2.w) & RT_HIT_INSIDE) != 0;
        const float Nx = flip ? -q1.y : q1.y, Ny = flip ? -q1.z : q1.z, Nz = flip ? -q1.w : q1.w;
        /* A = |N.x| < 0.5 ? (1, 0, 0) : (0, 1, 0);  U = normalize(cross(A, N));  V = cross(N, U) */
        const bool ax = fabsf(Nx) < 0.5f;
        const float Ax = ax ? 1.0f : 0.0f, Ay = ax ? 0.0f : 1.0f, Az = 0.0f;
        const float cx = Ay * Nz - Az * Ny, cy = Az * Nx - Ax * Nz, cz = Ax * Ny - Ay * Nx;
        const float len = sqrtf(cx * cx + cy * cy + cz * cz);
        const float Ux = cx / len, Uy = cy / len, Uz = cz / len;
        const float Vx = Ny * Uz - Nz * Uy, Vy = Nz * Ux - Nx * Uz, Vz = Nx * Uy - Ny * Ux;
        uint32_t *f = frames + threadIdx.x * kFrameStride;
        f[0] = __float_as_uint(q0.z), f[1] = __float_as_uint(q0.w), f[2] = __float_as_uint(q1.x);
        f[3] = __float_as_uint(Nx), f[4] = __float_as_uint(Ny), f[5] = __float_as_uint(Nz);
        f[6] = __float_as_uint(Ux), f[7] = __float_as_uint(Uy), f[8] = __float_as_uint(Uz);
        f[9] = __float_as_uint(Vx), f[10] = __float_as_uint(Vy), f[11] = __float_as_uint(Vz);
        f[12] = rt_indirect_hash(rt_indirect_hash(seed ^ 0x9e3779b9u) ^ (key + p0 + threadIdx.x));
        f[13] = live ? 1u : 0u;
    }
    __syncthreads();
    const uint32_t r = r0 + threadIdx.x;
    if (r >= total) return;
    const uint32_t p = r / S, s = r - p * S;
    const uint32_t *f = frames + (p - p0) * kFrameStride;
    float *o = rays + 6 * (size_t)r;
    if (f[13] == 0u) {                                                    /* dead */
#pragma unroll
        for (int c = 0; c < 6; ++c) o[c] = 0.0f;
        return;
    }
    const float Px = __uint_as_float(f[0]), Py = __uint_as_float(f[1]), Pz = __uint_as_float(f[2]);
    const float Nx = __uint_as_float(f[3]), Ny = __uint_as_float(f[4]), Nz = __uint_as_float(f[5]);
    const float Ux = __uint_as_float(f[6]), Uy = __uint_as_float(f[7]), Uz = __uint_as_float(f[8]);
    const float Vx = __uint_as_float(f[9]), Vy = __uint_as_float(f[10]), Vz = __uint_as_float(f[11]);
    /* the sample's point of the disc, lifted to the hemisphere */
    const uint32_t i = s / (uint32_t)n, j = s - i * (uint32_t)n;
    const uint32_t hs = rt_indirect_hash(f[12] ^ s);
    const float xi1 = (float)(hs >> 8) * 0x1p-24f;
    const float xi2 = (float)(rt_indirect_hash(hs ^ 0x9e3779b9u) >> 8) * 0x1p-24f;
    const float step = 2.0f / (float)n;
    const float a = ((float)i + xi1) * step - 1.0f, b = ((float)j + xi2) * step - 1.0f;
    const float dx = a * sqrtf(1.0f - (b * b) * 0.5f), dy = b * sqrtf(1.0f - (a * a) * 0.5f);
    const float w = (1.0f - dx * dx) - dy * dy;
    const float dz = w > 0.0f ? sqrtf(w) : 0.0f;
    const float Dx = (Ux * dx + Vx * dy) + Nx * dz, Dy = (Uy * dx + Vy * dy) + Ny * dz, Dz = (Uz * dx + Vz * dy) + Nz * dz;
    o[0] = Px, o[1] = Py, o[2] = Pz;
    o[3] = Px + Dx, o[4] = Py + Dy, o[5] = Pz + Dz;
}

/* out[3 p + c] = base[3 p + c] + term.c of the header for the m records of a chunk.  Sample s of record p is
 * samples[3 (p S + s) ..] and, with gather != NULL, its gather record's flags word gather[12 (p S + s) + 11].  A workgroup
 * takes kResolveSamples / S records: it reads their samples' floats as the consecutive words they are into LDS (lds_stride(S)
 * floats a record); then, one lane a sample, the flags word alone of each gather record, zeroing in LDS the three floats of a
 * sample whose first hit is a light; then one lane per record and channel sums its S values in order, divides, multiplies by
 * the weight, adds the base and stores -- a record's three lanes store its 12 bytes.  A word of the output is read (base) and
 * stored by the same lane, once: out == base is allowed. */
__global__ __launch_bounds__(kBlock) void rt_indirect_resolve_kernel(uint32_t m, int S, float gain, const float *__restrict__ samples,
                                                                     const int32_t *__restrict__ gather,
                                                                     const int32_t *__restrict__ hits, const float *__restrict__ kd,
                                                                     int n_objects, const float *base, float *out) {
    __shared__ float lds[lds_floats()];
    const uint32_t group = (uint32_t)kResolveSamples / (uint32_t)S;
    const uint32_t g0 = blockIdx.x * group;
    const uint32_t records = min(group, m - g0);                         /* (g0 < m: the grid is ceil(m / group)) */
    const uint32_t per = 3u * (uint32_t)S, stride = (uint32_t)lds_stride(S), words = records * per;
    const float *src = samples + (size_t)per * (size_t)g0;
    for (uint32_t i = threadIdx.x; i < words; i += (uint32_t)kBlock) {
        const uint32_t px = i / per;
        lds[px * stride + (i - px * per)] = src[i];
    }
    if (gather) {
        __syncthreads();
        const int32_t *flags = gather + ((size_t)g0 * (size_t)S) * kHitWords + kHitFlagsWord;
        for (uint32_t i = threadIdx.x; i < records * (uint32_t)S; i += (uint32_t)kBlock) {
            if ((flags[(size_t)i * kHitWords] & RT_HIT_LIGHT) == 0) continue;
            const uint32_t px = i / (uint32_t)S;
            float *v = lds + px * stride + 3u * (i - px * (uint32_t)S);
            v[0] = 0.0f, v[1] = 0.0f, v[2] = 0.0f;
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < 3u * records; t += (uint32_t)kBlock) {
        const uint32_t px = t / 3u, c = t - 3u * px;
        const float *v = lds + px * stride + c;
        float acc = v[0];
        for (int s = 1; s < S; ++s) acc = acc + v[3 * s];
        const float mean = acc / (float)S;
        const int32_t *h = hits + (size_t)(g0 + px) * kHitWords;
        const int32_t object = h[0];
        float term = 0.0f;
        if (object >= 0 && (h[kHitFlagsWord] & RT_HIT_LIGHT) == 0) {
            const float k = object < n_objects ? kd[object] : 0.0f;
            term = ((__int_as_float(h[8 + c]) * k) * gain) * mean;
        }
        const size_t at = 3 * (size_t)(g0 + px) + c;
        out[at] = base ? base[at] + term : term;
    }
}

namespace {

/* the handle's scratch, which only grows, and the last call's bookkeeping */
struct RtIndirectState {
    Buffer rays, samples, gather;                          /* a chunk's rays, their colours, their records (emitters == 0) */
    Buffer hits, out_rgb;                                  /* the host variant's records and its base / output */
    /* the last call's start, then per chunk rays generated, traced, (emitters == 0: queried,) resolved */
    StageClock clock;
    int stages = 3;
    rt_indirect_info info{};
    ~RtIndirectState() { clock.release(); }
};

unsigned blocks_of(size_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

/* the header's checks (2) .. (9) */
int check_params(const rt_indirect_params *pr, int n, const void *hits, const void *out) {
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->samples < 1 || pr->samples > kMaxSamples)
        return fail(RT_ERR_INVALID, "samples must be 1.." + std::to_string(kMaxSamples) + " (got " + std::to_string(pr->samples) + ")");
    if (pr->gather_depth < 0) return fail(RT_ERR_INVALID, "gather_depth must not be negative");
    if (pr->chunk_records < 0) return fail(RT_ERR_INVALID, "chunk_records must not be negative");
    if (pr->emitters != 0 && pr->emitters != 1)
        return fail(RT_ERR_INVALID, "emitters must be 0 or 1 (got " + std::to_string(pr->emitters) + ")");
    if (!std::isfinite(pr->gain)) return fail(RT_ERR_INVALID, "gain must be finite");
    if (n < 0) return fail(RT_ERR_INVALID, "n < 0");
    if (n > 0 && !hits) return fail(RT_ERR_INVALID, "hits pointer is NULL");
    if (n > 0 && !out) return fail(RT_ERR_INVALID, "output pointer is NULL");
    return RT_OK;
}

/* rt_indirect_rays*: the header's checks up to the device */
int check_rays_args(const rt_indirect_params *pr, int n, const void *hits, const void *out, bool device) {
    const int rc = check_params(pr, n, hits, out);
    if (rc) return rc;
    if ((double)n * (double)(pr->samples * pr->samples) * 6.0 > kMaxRayFloats)
        return fail(RT_ERR_INVALID, "batch too large for its rays");
    if (device && ((uintptr_t)hits & 15u) != 0) return fail(RT_ERR_INVALID, "d_hits must be 16-byte aligned");
    if (device && ((uintptr_t)out & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_rays must be 4-byte aligned");
    return RT_OK;
}

/* rt_indirect_diffuse*'s checks in the header's order (device: the device variant's alignments as well) */
int check_diffuse_args(const rt_scene *s, const rt_indirect_params *pr, int n, const void *hits, const void *base, const void *out,
                       bool device) {
    if (!s) return fail(RT_ERR_INVALID, "scene is NULL");
    const int rc = check_params(pr, n, hits, out);
    if (rc) return rc;
    if (n > kMaxRecords) return fail(RT_ERR_INVALID, "more than " + std::to_string(kMaxRecords) + " records");
    if (device && ((uintptr_t)hits & 15u) != 0) return fail(RT_ERR_INVALID, "d_hits must be 16-byte aligned");
    if (device && ((uintptr_t)out & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_rgb must be 4-byte aligned");
    if (device && base && ((uintptr_t)base & 3u) != 0) return fail(RT_ERR_INVALID, "d_base_rgb must be 4-byte aligned");
    if (rt_internal_scene_soft(s))
        return fail(RT_ERR_INVALID, "the indirect term refuses a scene with area lights: a ray batch keys their shadow samples by "
                                    "the ray index (include/rt_capi_soft.h), so the result would change with chunk_records");
    return RT_OK;
}

/* a record's scratch: its rays and their colours, and with emitters == 0 the gather rays' records */
size_t record_bytes(const rt_indirect_params &pr) {
    return (size_t)(pr.samples * pr.samples) * (pr.emitters ? 36u : 84u);
}

/* the records a launch gathers for: the caller's chunk_records, or the default -- as many as keep the scratch within
 * kChunkBytes, at least one -- never more than kMaxBatchRays rays' worth, nor than the batch has */
int chunk_records(const rt_indirect_params &pr, int n) {
    const long long S = (long long)pr.samples * pr.samples;                          /* rays a record; <= 64 */
    long long c = pr.chunk_records > 0 ? pr.chunk_records : std::max<long long>(1, (long long)(kChunkBytes / record_bytes(pr)));
    c = std::min(c, kMaxBatchRays / S);
    return (int)std::min<long long>(c, n);
}

/* the last call's stage times from its events, once: interval i is stage i % stages of chunk i / stages, the stages being
 * raygen, trace, (stages == 4: query,) resolve */
int collect(RtIndirectState *a) {
    if (a->clock.collected) return RT_OK;
    std::vector<float> t;
    const int rc = a->clock.intervals(&t);
    if (rc) return rc;
    double ms[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = 0; i < t.size(); ++i) ms[i % (size_t)a->stages] += t[i];
    a->info.raygen_ms = ms[0], a->info.trace_ms = ms[1];
    a->info.query_ms = a->stages == 4 ? ms[2] : 0.0;
    a->info.resolve_ms = ms[a->stages - 1];
    return RT_OK;
}

void indirect_free(void *state) { delete static_cast<RtIndirectState *>(state); }

double indirect_ms(void *state, uint64_t seq) {
    RtIndirectState *a = static_cast<RtIndirectState *>(state);
    if (!a || a->clock.seq != seq || a->clock.n_events == 0 || collect(a) != RT_OK) return -1.0;
    return a->info.raygen_ms + a->info.trace_ms + a->info.query_ms + a->info.resolve_ms;
}

RtIndirectState *state_of(rt_scene *s) {
    return unit_state<RtIndirectState>(s, RT_INTERNAL_UNIT_INDIRECT, indirect_free, indirect_ms);
}

/* the rays of m records at d_hits, the first of which samples with key, into d_rays, on stream */
int enqueue_raygen(const rt_indirect_params &pr, uint32_t key, uint32_t m, const void *d_hits, void *d_rays, hipStream_t stream) {
    const size_t n_rays = (size_t)m * (size_t)(pr.samples * pr.samples);
    hipLaunchKernelGGL(rt_indirect_raygen_kernel, dim3(blocks_of(n_rays)), dim3(kBlock), 0, stream, m, pr.samples, pr.seed, key,
                       static_cast<const float4 *>(d_hits), static_cast<float *>(d_rays));
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

/* rt_indirect_rays*'s launches: at most kMaxBatchRays rays each, so that a ray's number fits the kernel's 32 bits */
int enqueue_all_rays(const rt_indirect_params &pr, int n, const void *d_hits, void *d_rays, hipStream_t stream) {
    const int S = pr.samples * pr.samples;
    const int chunk = (int)std::min<long long>(kMaxBatchRays / S, n);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        const int rc = enqueue_raygen(pr, pr.key0 + (uint32_t)i0, (uint32_t)m, static_cast<const char *>(d_hits) + (size_t)i0 * 48,
                                      static_cast<char *>(d_rays) + (size_t)i0 * (size_t)S * 24, stream);
        if (rc) return rc;
    }
    return RT_OK;
}

/* the call, every argument checked, the handle locked, n > 0: device memory, on stream.  The events of the call before are
 * recorded anew without being waited for: its stage times, if nobody asked for them, are lost. */
int run(rt_scene *s, const rt_indirect_params &pr, int n, const void *d_hits, const void *d_base, void *d_out, hipStream_t stream) {
    RtIndirectState *a = state_of(s);
    const int S = pr.samples * pr.samples;
    const int chunk = chunk_records(pr, n);
    const size_t most = (size_t)chunk * (size_t)S;                        /* rays of the largest chunk, the first */
    const float *d_kd = nullptr;
    int n_objects = 0;
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    int rc = rt_internal_object_diffuse(s, &d_kd, &n_objects);
    if (rc == RT_OK) rc = a->rays.grow(most * 24);
    if (rc == RT_OK) rc = a->samples.grow(most * 12);
    if (rc == RT_OK && !pr.emitters) rc = a->gather.grow(most * 48);
    /* the ray generation below writes the rays that the call before, on another stream, may not have traced yet */
    if (rc == RT_OK) rc = rt_internal_order_stream(s, stream);
    if (rc) return rc;
    a->clock.n_events = 0;
    a->stages = pr.emitters ? 3 : 4;
    a->clock.collected = true;
    a->info = rt_indirect_info{};
    a->info.records = n;
    if ((rc = a->clock.mark(stream))) return rc;
    const unsigned group = (unsigned)(kResolveSamples / S);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, n - i0);
        const int n_rays = (int)(m * (uint32_t)S);                        /* <= kMaxBatchRays */
        const char *hits = static_cast<const char *>(d_hits) + (size_t)i0 * 48;
        rc = enqueue_raygen(pr, pr.key0 + (uint32_t)i0, m, hits, a->rays.p, stream);
        if (rc == RT_OK) rc = a->clock.mark(stream);
        if (rc == RT_OK) rc = rt_internal_launch_rays(s, n_rays, n_rays, a->rays.p, pr.gather_depth, a->samples.p, stream);
        if (rc == RT_OK) rc = a->clock.mark(stream);
        if (rc == RT_OK && !pr.emitters) {
            rc = rt_internal_launch_hits(s, n_rays, n_rays, a->rays.p, a->gather.p, stream);
            if (rc == RT_OK) rc = a->clock.mark(stream);
        }
        if (rc) return rc;
        hipLaunchKernelGGL(rt_indirect_resolve_kernel, dim3((m + group - 1) / group), dim3(kBlock), 0, stream, m, S, pr.gain,
                           static_cast<const float *>(a->samples.p), pr.emitters ? nullptr : static_cast<const int32_t *>(a->gather.p),
                           reinterpret_cast<const int32_t *>(hits), d_kd, n_objects,
                           d_base ? static_cast<const float *>(d_base) + 3 * (size_t)i0 : nullptr,
                           static_cast<float *>(d_out) + 3 * (size_t)i0);
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

int rt_capi_indirect_version(void) { return RT_CAPI_INDIRECT_VERSION; }

/* rt_internal.h: the chunk's ray generation, for rt_paths.hip's bounce 0 */
int rt_internal_indirect_raygen(int samples, uint32_t seed, uint32_t key, uint32_t m, const void *d_hits, void *d_rays,
                                void *hip_stream) {
    rt_indirect_params pr{};
    pr.samples = samples, pr.seed = seed;
    return enqueue_raygen(pr, key, m, d_hits, d_rays, static_cast<hipStream_t>(hip_stream));
}

int rt_indirect_rays_device(const rt_indirect_params *pr, int n, const void *d_hits, int device, void *d_out_rays, void *hip_stream) {
    int rc = check_rays_args(pr, n, d_hits, d_out_rays, true);
    if (rc == RT_OK) rc = rt_internal_check_device(device);
    if (rc || n == 0) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue_all_rays(*pr, n, d_hits, d_out_rays, static_cast<hipStream_t>(hip_stream));
}

int rt_indirect_rays(const rt_indirect_params *pr, int n, const rt_hit *hits, int device, float *out_rays) {
    int rc = check_rays_args(pr, n, hits, out_rays, false);
    if (rc == RT_OK) rc = rt_internal_check_device(device);
    if (rc || n == 0) return rc;
    const HostIn in[1] = {{hits, (size_t)n * 48}};
    const HostOut out[1] = {{out_rays, (size_t)n * (size_t)(pr->samples * pr->samples) * 24}};
    return staged_call(device, in, 1, out, 1, 0, nullptr, [&](void *const *d_in, void *const *d_out, void *) {
        return enqueue_all_rays(*pr, n, d_in[0], d_out[0], nullptr);
    });
}

int rt_indirect_diffuse_device(rt_scene *s, const rt_indirect_params *pr, int n, const void *d_hits, const void *d_base_rgb,
                               void *d_out_rgb, void *hip_stream) {
    const int rc = check_diffuse_args(s, pr, n, d_hits, d_base_rgb, d_out_rgb, true);
    if (rc || n == 0) return rc;
    const rt_indirect_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    return run(s, p, n, d_hits, d_base_rgb, d_out_rgb, static_cast<hipStream_t>(hip_stream));
}

int rt_indirect_diffuse(rt_scene *s, const rt_indirect_params *pr, int n, const rt_hit *hits, const float *base_rgb, float *out_rgb) {
    int rc = check_diffuse_args(s, pr, n, hits, base_rgb, out_rgb, false);
    if (rc || n == 0) return rc;
    const rt_indirect_params p = *pr;
    rt_internal_lock(s);
    Unlock unlock{s};
    RtIndirectState *a = state_of(s);
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

int rt_get_indirect_info(const rt_scene *cs, rt_indirect_info *out) {
    if (!cs || !out) return fail(RT_ERR_INVALID, "scene/out is NULL");
    rt_scene *s = const_cast<rt_scene *>(cs);
    rt_internal_lock(s);
    Unlock unlock{s};
    RtIndirectState *a = static_cast<RtIndirectState *>(rt_internal_unit_slot(s, RT_INTERNAL_UNIT_INDIRECT)->state);
    if (!a) {
        *out = rt_indirect_info{};
        return RT_OK;
    }
    HIP_TRY(hipSetDevice(rt_internal_scene_device(s)));
    const int rc = collect(a);
    if (rc) return rc;
    *out = a->info;
    return RT_OK;
}

} // extern "C"
