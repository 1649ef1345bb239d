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

#pragma clang fp contract(off)

/* -DRT_MIRROR_VARIANTS=1 (scripts/mirror_experiments.py) builds both ways of reading the records and exports the switch
 * between them, rt_internal_mirror_variant(); the library proper has the kept one alone. */
#ifndef RT_MIRROR_VARIANTS
#define RT_MIRROR_VARIANTS 0
#endif

static_assert(sizeof(rt_mirror_params) == 12 && sizeof(rt_mirror_info) == 32, "rt_mirror.h layouts");
static_assert(sizeof(rt_hit) == 48, "rt_capi_query.h layout");

namespace {

constexpr int kBlock = 256;                            /* rays a workgroup */
constexpr size_t kChunkBytes = (size_t)256 << 20;      /* the default chunk: its scratch within 256 MiB */
constexpr double kMaxRayFloats = 2.0e9 * 4.0;          /* rt_render's limit for one output, in floats */
constexpr long long kMaxCells = 0x7fffffffLL - 64;     /* rt_trace_rays' grid limit (include/rt_capi_rays.h) */
constexpr int kStateWords = 14;                        /* a ray's state: the word, w, L, A -- each a plane of the chunk */
constexpr int kStateWordsNoGuide = 4;                  /* without a guide: the word and w */
constexpr size_t kRayBytes = 48 + 24 + 4 * kStateWords;   /* a ray's scratch: its record, its next ray, its state */
constexpr uint32_t kDone = 1u << 9;                    /* the state word is out_path's (k | cut << 8 | tag << 12) and this */
constexpr int kLdsStride = 13;                         /* STAGE: a record's 12 words in LDS, odd stride */
/* How the step kernel reads its 48-byte-strided records.  false: three 16-byte loads a lane.  true: the workgroup's records as
 * the consecutive words they are through LDS (rt_accumulate_body.h's and rt_upsample.hip's way).  Both were measured
 * (profiles/mirror_experiments.txt); this is the one kept. */
constexpr bool kStageLds = false;

} // namespace

/* the 32-bit integer hash "lowbias32" (include/rt_capi_ao.h) */
__device__ __forceinline__ uint32_t rt_mirror_hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float rt_mirror_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

/* normalize(T - E) of the ray at r[0..5], createEyeRay's arithmetic */
__device__ __forceinline__ void rt_mirror_direction(const float *r, float *dx, float *dy, float *dz) {
    const float x = r[3] - r[0], y = r[4] - r[1], z = r[5] - r[2];
    const float len = sqrtf((x * x + y * y) + z * z);
    *dx = x / len, *dy = y / len, *dz = z / len;
}

/* Bounce s of the m rays of a chunk, one lane a ray (i < m < 2^31).  records[3 i ..] is the record of ray_s, rays_k[6 i ..] is
 * ray_s itself (FIRST: the caller's rays; later the chunk's scratch, which rays_next then is as well: a lane reads its own
 * ray before it writes it), rays0 the caller's rays, state the chunk's planes of `stride` words (kStateWords of them with
 * GUIDE, else kStateWordsNoGuide).  FIRST: s == 0, the starting state is the header's and no state is read.  last: s ==
 * max_bounces, every ray still alive ends here.  GUIDE: out_guide is given, so L and A are carried.  STAGE: kStageLds.  Every
 * address is i's own (STAGE: or one of the workgroup's records, below records[3 m]): nothing is read or written past ray m - 1. */
template <bool FIRST, bool GUIDE, bool STAGE>
__global__ __launch_bounds__(kBlock) void rt_mirror_step_kernel(uint32_t m, uint32_t stride, int last, float min_reflective,
                                                                const float *__restrict__ rf, int n_objects,
                                                                const float4 *__restrict__ records, const float *rays_k,
                                                                const float *__restrict__ rays0, float *rays_next, uint32_t *state,
                                                                float4 *__restrict__ out_hits, float4 *__restrict__ out_guide,
                                                                float *__restrict__ out_weight, uint32_t *__restrict__ out_path) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    __shared__ float lds[STAGE ? kBlock * kLdsStride : 1];
    if (STAGE) {
        const uint32_t base = blockIdx.x * (uint32_t)kBlock;                 /* (base < m: the grid is ceil(m / kBlock)) */
        const uint32_t words = min((uint32_t)kBlock, m - base) * 12u;
        const float *src = reinterpret_cast<const float *>(records) + (size_t)base * 12;
        for (uint32_t t = threadIdx.x; t < words; t += (uint32_t)kBlock) {
            const uint32_t rec = t / 12u;
            lds[rec * kLdsStride + (t - rec * 12u)] = src[t];
        }
        __syncthreads();
    }
    if (i >= m) return;
    const uint32_t word = FIRST ? 0u : state[i];
    if (word & kDone) return;
    float4 q0, q1, q2;
    if (STAGE) {
        const float *q = lds + threadIdx.x * kLdsStride;
        q0 = make_float4(q[0], q[1], q[2], q[3]), q1 = make_float4(q[4], q[5], q[6], q[7]), q2 = make_float4(q[8], q[9], q[10], q[11]);
    } else {
        q0 = records[3 * (size_t)i], q1 = records[3 * (size_t)i + 1], q2 = records[3 * (size_t)i + 2];
    }
    const int32_t object = __float_as_int(q0.x), flags = __float_as_int(q2.w);
    const uint32_t k = word & 0xffu, tag = word >> 12;
    float wx = 1.0f, wy = 1.0f, wz = 1.0f, L = 0.0f;
    float A[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    if (!FIRST) {
        wx = __uint_as_float(state[(size_t)stride + i]);
        wy = __uint_as_float(state[2 * (size_t)stride + i]);
        wz = __uint_as_float(state[3 * (size_t)stride + i]);
        if (GUIDE) {
            L = __uint_as_float(state[4 * (size_t)stride + i]);
#pragma unroll
            for (int c = 0; c < 9; ++c) A[c] = __uint_as_float(state[(size_t)(5 + c) * stride + i]);
        }
    }
    if (GUIDE && object >= 0) L = L + q0.y;
    const float refl = (object >= 0 && object < n_objects) ? rf[object] : 0.0f;
    const bool mirror = object >= 0 && object < n_objects && (flags & RT_HIT_LIGHT) == 0 && refl >= min_reflective;
    const float Px = q0.z, Py = q0.w, Pz = q1.x, nx = q1.y, ny = q1.z, nz = q1.w;

    if (!mirror || last) {                                                    /* the terminal record */
        out_hits[3 * (size_t)i] = q0, out_hits[3 * (size_t)i + 1] = q1, out_hits[3 * (size_t)i + 2] = q2;
        if (out_weight) {
            float *o = out_weight + 3 * (size_t)i;
            o[0] = wx, o[1] = wy, o[2] = wz;
        }
        if (out_path) out_path[i] = k | (mirror ? 1u << 8 : 0u) | tag << 12;
        if (GUIDE) {
            float4 g0 = q0, g1 = q1;
            if (!FIRST && object >= 0 && k != 0u) {
                const float *e = rays0 + 6 * (size_t)i;
                float dx, dy, dz;
                rt_mirror_direction(e, &dx, &dy, &dz);
                g0.x = __int_as_float((int32_t)(tag << 12 | (uint32_t)object));
                g0.y = L;
                g0.z = e[0] + dx * L, g0.w = e[1] + dy * L, g1.x = e[2] + dz * L;
                g1.y = rt_mirror_dot(A[0], A[1], A[2], nx, ny, nz);
                g1.z = rt_mirror_dot(A[3], A[4], A[5], nx, ny, nz);
                g1.w = rt_mirror_dot(A[6], A[7], A[8], nx, ny, nz);
            }
            out_guide[3 * (size_t)i] = g0, out_guide[3 * (size_t)i + 1] = g1, out_guide[3 * (size_t)i + 2] = q2;
        }
        if (!last) {                                                          /* retired: a degenerate ray from here on */
            float *o = rays_next + 6 * (size_t)i;
#pragma unroll
            for (int c = 0; c < 6; ++c) o[c] = 0.0f;
            state[i] = kDone;
        }
        return;
    }

    float dx, dy, dz;
    rt_mirror_direction(rays_k + 6 * (size_t)i, &dx, &dy, &dz);
    const float c = rt_mirror_dot(nx, ny, nz, dx, dy, dz);
    const float rx = ((-2.0f * nx) * c) + dx, ry = ((-2.0f * ny) * c) + dy, rz = ((-2.0f * nz) * c) + dz;
    float *o = rays_next + 6 * (size_t)i;
    o[0] = Px, o[1] = Py, o[2] = Pz;
    o[3] = Px + rx, o[4] = Py + ry, o[5] = Pz + rz;
    state[i] = (k + 1u) | (1u + rt_mirror_hash(tag << 12 | (uint32_t)object) % 0x7fffeu) << 12;
    state[(size_t)stride + i] = __float_as_uint(wx * (refl * q2.x));
    state[2 * (size_t)stride + i] = __float_as_uint(wy * (refl * q2.y));
    state[3 * (size_t)stride + i] = __float_as_uint(wz * (refl * q2.z));
    if (GUIDE) {
        state[4 * (size_t)stride + i] = __float_as_uint(L);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float an = rt_mirror_dot(A[3 * r], A[3 * r + 1], A[3 * r + 2], nx, ny, nz);
            const float two = 2.0f * an;
            state[(size_t)(5 + 3 * r) * stride + i] = __float_as_uint(A[3 * r] - two * nx);
            state[(size_t)(6 + 3 * r) * stride + i] = __float_as_uint(A[3 * r + 1] - two * ny);
            state[(size_t)(7 + 3 * r) * stride + i] = __float_as_uint(A[3 * r + 2] - two * nz);
        }
    }
}

namespace {

/* the handle's scratch, which only grows, and the last call's bookkeeping */
struct RtMirrorState {
    Buffer records, rays, state;                           /* a chunk's records, its next rays, its state planes */
    StageClock clock;                                      /* the last call's start, then per chunk and bounce query, step */
    rt_mirror_info info{};
    ~RtMirrorState() { clock.release(); }
};

/* the header's checks (1) .. (10) */
int check_args(const rt_scene *s, const rt_mirror_params *pr, int n, int rows, const void *rays, const void *out_hits,
               const void *out_guide, const void *out_weight, const void *out_path, bool device) {
    if (!s) return fail(RT_ERR_INVALID, "scene is NULL");
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->max_bounces < 0 || pr->max_bounces > RT_MIRROR_MAX_BOUNCES)
        return fail(RT_ERR_INVALID, "max_bounces must be 0.." + std::to_string(RT_MIRROR_MAX_BOUNCES) + " (got " +
                                        std::to_string(pr->max_bounces) + ")");
    if (pr->chunk_rays < 0) return fail(RT_ERR_INVALID, "chunk_rays must not be negative");
    if (std::isnan(pr->min_reflective)) return fail(RT_ERR_INVALID, "min_reflective must not be NaN");
    if (n < 0) return fail(RT_ERR_INVALID, "n < 0");
    if (rows < 1) return fail(RT_ERR_INVALID, "rows must be positive");
    if (n > 0 && !rays) return fail(RT_ERR_INVALID, "rays pointer is NULL");
    if (n > 0 && !out_hits) return fail(RT_ERR_INVALID, "out_hits pointer is NULL");
    /* rt_trace_rays' limit (rays_args() of rt_capi.hip): the batch's floats, and the cells of its grid of rows */
    const int r = std::min(rows, std::max(n, 1));
    if ((double)n * 3.0 > kMaxRayFloats || (((long long)n + r - 1) / r) * r > kMaxCells)
        return fail(RT_ERR_INVALID, "ray batch too large for its rows");
    if (!device) return RT_OK;
    if (((uintptr_t)rays & 3u) != 0) return fail(RT_ERR_INVALID, "d_rays must be 4-byte aligned");
    if (((uintptr_t)out_hits & 15u) != 0) return fail(RT_ERR_INVALID, "d_out_hits must be 16-byte aligned");
    if (((uintptr_t)out_guide & 15u) != 0) return fail(RT_ERR_INVALID, "d_out_guide must be 16-byte aligned");
    if (((uintptr_t)out_weight & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_weight must be 4-byte aligned");
    if (((uintptr_t)out_path & 3u) != 0) return fail(RT_ERR_INVALID, "d_out_path must be 4-byte aligned");
    return RT_OK;
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
    hipLaunchKernelGGL((rt_mirror_step_kernel<FIRST, GUIDE, STAGE>), dim3((m + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, m, stride,
                       last, min_reflective, rf, n_objects, static_cast<const float4 *>(records), static_cast<const float *>(rays_k),
                       static_cast<const float *>(rays0), static_cast<float *>(rays_next), static_cast<uint32_t *>(state),
                       static_cast<float4 *>(out_hits), static_cast<float4 *>(out_guide), static_cast<float *>(out_weight),
                       static_cast<uint32_t *>(out_path));
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
