/*
 * rt_upsample.hip -- implementation of include/rt_capi_upsample.h: the records of every s-th pixel picked out of a frame's, and
 * values gathered for them carried back to every pixel by a joint-bilateral tent filter guided by the full-resolution records.
 * The header is the definition; these kernels are bit-exact to it (the library's arithmetic flags: no contraction, correctly
 * rounded divide, denormals kept).
 *
 * SHAPE.  Both passes are memory-bound.  One lane a pixel (a cell, for the subsample), the 64 lanes of a
 * wavefront along z, the contiguous axis: a pixel's own 48-byte record is three 16-byte loads a lane, 3 KiB contiguous a
 * wavefront.  The four tap records of a pixel are shared by the s x s pixels of its cell, so a workgroup's 4 x 64 pixels need at
 * most 3 x 33 of them.  Two ways of fetching them were built and measured (profiles/upsample_experiments.txt): kLds stages the
 * tile's tap records in LDS once, as three planes of 16-byte slots so that neighbouring lanes read neighbouring slots; the other
 * loads the four taps per lane from global memory, where s lanes in a row read the same address and the caches serve the rest.
 * At 4096 x 4096 the staged variant takes 0.27 ms at s = 2 and 0.26 ms at s = 4, the other 0.34 and 0.28 ms, a device copy of
 * the same traffic 0.23 ms.  The staged variant is the one the library has; the other is compiled, with an entry point that names
 * the variant (rt_internal_upsample_variant), only into a build with -DRT_UPSAMPLE_VARIANTS=1 (`make variant`), which is what
 * scripts/upsample_experiments.py needs to repeat the comparison.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/rt_capi_upsample.h"
#include "rt_host.h"

static_assert(sizeof(rt_hit) == 48, "rt_hit layout");
static_assert(sizeof(rt_upsample_params) == 28, "rt_upsample_params layout");

#ifndef RT_UPSAMPLE_VARIANTS
#define RT_UPSAMPLE_VARIANTS 0         /* 1: also the variant that was measured and not kept, and the entry point that names it */
#endif

namespace {

constexpr int kTileZ = 64, kTileX = 4;                 /* a workgroup: 4 wavefronts, each 64 consecutive z of one column */
constexpr int kCellsX = 3, kCellsZ = 33;               /* the most tap cells a tile touches, at s = 2: 4/2 + 1 and 64/2 + 1 */
constexpr double kMaxPixels = 2.0e9 * 4.0 * 4.0 / 60.0; /* rt_render_gbuffer's limit: 3.2e10 bytes of colours and records */

} // namespace

struct rt_upsample_args {    /* the upsample kernel's arguments beside its buffers */
    int Wn, H, Wl, Hl, s, squarings, match_color, modulate, plane;
    float inv, dead_value;
    uint32_t tiles_z;
};
using Args = rt_upsample_args;

/* a record's three 16-byte words: {object, distance, point.xy}, {point.z, normal.xyz}, {color.rgb, flags} */
struct Rec {
    uint4 a, b, c;
};

__device__ __forceinline__ Rec load_rec(const uint4 *__restrict__ hits, int64_t index) {
    const uint4 *r = hits + 3 * index;                  /* (64-bit: 48 index passes 2^32 in a large frame) */
    return Rec{r[0], r[1], r[2]};
}

/* cell (i, j) of the low-resolution frame <- pixel (i s, j s); white: a live record's colour words become 1.0f */
__global__ __launch_bounds__(256) void rt_subsample_kernel(const uint4 *__restrict__ hits, uint4 *__restrict__ out, int H, int Wl,
                                                          int Hl, int s, int white, uint32_t tiles_z) {
    const uint32_t tz = blockIdx.x % tiles_z, tx = blockIdx.x / tiles_z;
    const int64_t i = (int64_t)tx * kTileX + threadIdx.y, j = (int64_t)tz * kTileZ + threadIdx.x;
    if (i >= Wl || j >= Hl) return;
    Rec r = load_rec(hits, (i * s) * (int64_t)H + j * s);
    const bool dead = (int32_t)r.a.x < 0 || (r.c.w & (uint32_t)RT_HIT_LIGHT) != 0u;
    if (white && !dead) r.c.x = r.c.y = r.c.z = 0x3F800000u;
    uint4 *o = out + 3 * (i * Hl + j);
    o[0] = r.a, o[1] = r.b, o[2] = r.c;
}

/* the header's definition, one lane a pixel.  kC: channels; kLds: the tile's tap records come from LDS (staged below) instead
 * of from global memory.  A lane without a pixel stays for the barrier and leaves after it. */
template <int kC, bool kLds>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_upsample_kernel(const uint4 *__restrict__ hits, const float *__restrict__ lo,
                                                                     const float *base, float *out, uint8_t *__restrict__ flags,
                                                                     Args A) {
    __shared__ uint4 taps[kLds ? 3 : 1][kLds ? kCellsX * kCellsZ : 1];
    const int s = A.s;
    const uint32_t tz = blockIdx.x % A.tiles_z, tx = blockIdx.x / A.tiles_z;
    const int64_t x64 = (int64_t)tx * kTileX + threadIdx.y, z64 = (int64_t)tz * kTileZ + threadIdx.x;
    const int ci = (int)(((int64_t)tx * kTileX) / s), cj = (int)(((int64_t)tz * kTileZ) / s);      /* the tile's first cell */
    if (kLds) {
        /* cells [ci, ci + ni) x [cj, cj + nj): those of the tile's pixels and one more each way, as far as they exist */
        const int64_t xe = (int64_t)tx * kTileX + kTileX - 1, ze = (int64_t)tz * kTileZ + kTileZ - 1;
        const int ni = (int)(xe / s) - ci + 2, nj = (int)(ze / s) - cj + 2;       /* <= kCellsX, kCellsZ */
        const int t = (int)(threadIdx.y * kTileZ + threadIdx.x);
        for (int k = t; k < ni * nj * 3; k += kTileZ * kTileX) {
            const int cell = k / 3, word = k - 3 * cell;
            const int i = ci + cell / nj, j = cj + cell % nj;
            if (i < A.Wl && j < A.Hl) taps[word][(i - ci) * kCellsZ + (j - cj)] = hits[3 * (((int64_t)i * s) * A.H + (int64_t)j * s) + word];
        }
        __syncthreads();
    }
    if (x64 >= A.Wn || z64 >= A.H) return;
    const int x = (int)x64, z = (int)z64;
    const int64_t p = (int64_t)x * A.H + z;
    const Rec h = load_rec(hits, p);
    const bool dead = (int32_t)h.a.x < 0 || (h.c.w & (uint32_t)RT_HIT_LIGHT) != 0u;
    const int i0 = x / s, j0 = z / s, fx = x - i0 * s, fz = z - j0 * s;
    float v[kC];
    uint8_t flag = 0;
    if (dead) {
#pragma unroll
        for (int c = 0; c < kC; ++c) v[c] = A.dead_value;
    } else if (fx == 0 && fz == 0) {
        const float *l = lo + ((int64_t)i0 * A.Hl + j0) * kC;
#pragma unroll
        for (int c = 0; c < kC; ++c) v[c] = l[c];
    } else {
        const float npx = __uint_as_float(h.b.y), npy = __uint_as_float(h.b.z), npz = __uint_as_float(h.b.w);
        const float ppx = __uint_as_float(h.a.z), ppy = __uint_as_float(h.a.w), ppz = __uint_as_float(h.b.x);
        float acc[kC], all[kC], wsum = 0.0f, tsum = 0.0f;
#pragma unroll
        for (int c = 0; c < kC; ++c) acc[c] = all[c] = 0.0f;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int i = i0 + a, j = j0 + b;
                const int ti = (a ? fx : s - fx) * (b ? fz : s - fz);
                if (i >= A.Wl || j >= A.Hl || ti == 0) continue;
                const float tent = (float)ti;
                Rec g;
                if (kLds) {
                    const int slot = (i - ci) * kCellsZ + (j - cj);
                    g = Rec{taps[0][slot], taps[1][slot], taps[2][slot]};
                } else {
                    g = load_rec(hits, ((int64_t)i * s) * A.H + (int64_t)j * s);
                }
                const float *l = lo + ((int64_t)i * A.Hl + j) * kC;
                float lv[kC];
#pragma unroll
                for (int c = 0; c < kC; ++c) lv[c] = l[c];
                /* the hole's fallback: every cell that exists, by its tent alone */
#pragma unroll
                for (int c = 0; c < kC; ++c) all[c] = all[c] + tent * lv[c];
                tsum = tsum + tent;
                bool take = g.a.x == h.a.x && ((g.c.w ^ h.c.w) & 3u) == 0u;
                if (A.match_color) take = take && g.c.x == h.c.x && g.c.y == h.c.y && g.c.z == h.c.z;
                const float t = (npx * __uint_as_float(g.b.y) + npy * __uint_as_float(g.b.z)) + npz * __uint_as_float(g.b.w);
                float wn = t > 0.0f ? t : 0.0f;
                for (int k = 0; k < A.squarings; ++k) wn = wn * wn;
                float w = tent * wn;
                if (A.plane) {
                    const float ex = __uint_as_float(g.a.z) - ppx, ey = __uint_as_float(g.a.w) - ppy, ez = __uint_as_float(g.b.x) - ppz;
                    const float d = (ex * npx + ey * npy) + ez * npz;
                    const float u = 1.0f - (d * d) * A.inv;
                    w = w * (u > 0.0f ? u : 0.0f);
                }
                take = take && w > 0.0f;
                if (take) {
#pragma unroll
                    for (int c = 0; c < kC; ++c) acc[c] = acc[c] + w * lv[c];
                    wsum = wsum + w;
                }
            }
        }
        const bool any = wsum > 0.0f;
        flag = any ? 0 : 1;
#pragma unroll
        for (int c = 0; c < kC; ++c) v[c] = any ? acc[c] / wsum : all[c] / tsum;
    }
    if constexpr (kC == 3) {
        if (A.modulate && !dead) {
            v[0] = v[0] * __uint_as_float(h.c.x);
            v[1] = v[1] * __uint_as_float(h.c.y);
            v[2] = v[2] * __uint_as_float(h.c.z);
        }
    }
    float *o = out + p * kC;
    if (base) {
        const float *bs = base + p * kC;                /* (may be o: read before the stores below) */
        float bv[kC];
#pragma unroll
        for (int c = 0; c < kC; ++c) bv[c] = bs[c];
#pragma unroll
        for (int c = 0; c < kC; ++c) v[c] = bv[c] + v[c];
    }
#pragma unroll
    for (int c = 0; c < kC; ++c) o[c] = v[c];
    if (flags) flags[p] = flag;
}

namespace {

/* the header's checks that the two calls share, in its order: scale, then the 0 / 1 switches */
int check_scale(int scale) {
    if (scale < 2 || scale > 8) return fail(RT_ERR_INVALID, "scale must be 2..8");
    return RT_OK;
}

int check_rectangle(int Wn, int H) {
    if (Wn <= 0 || H <= 0) return fail(RT_ERR_INVALID, "need Wn, H > 0");
    if ((double)Wn * (double)H > kMaxPixels) return fail(RT_ERR_INVALID, "rectangle too large for its colours and records");
    /* a launch has fewer than 2^32 work-items: a workgroup is 256 of them whatever part of its 4 x 64 pixels exists */
    const uint64_t tiles = (((uint64_t)Wn + kTileX - 1) / kTileX) * (((uint64_t)H + kTileZ - 1) / kTileZ);
    if (tiles >= (1ull << 24)) return fail(RT_ERR_INVALID, "rectangle too thin: 2^24 or more tiles of 4 x 64 pixels");
    return RT_OK;
}

int check_params(const rt_upsample_params *pr, int Wn, int H) {
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    int rc = check_scale(pr->scale);
    if (rc) return rc;
    if (pr->channels != 1 && pr->channels != 3) return fail(RT_ERR_INVALID, "channels must be 1 or 3");
    if (pr->normal_squarings < 0 || pr->normal_squarings > 6) return fail(RT_ERR_INVALID, "normal_squarings must be 0..6");
    if ((pr->match_color | 1) != 1) return fail(RT_ERR_INVALID, "match_color must be 0 or 1");
    if ((pr->modulate | 1) != 1) return fail(RT_ERR_INVALID, "modulate must be 0 or 1");
    if (pr->modulate && pr->channels != 3) return fail(RT_ERR_INVALID, "modulate needs channels 3");
    if (!(pr->sigma_plane >= 0.0f) || std::isinf(pr->sigma_plane))
        return fail(RT_ERR_INVALID, "sigma_plane must be finite and >= 0");
    if (!std::isfinite(pr->dead_value)) return fail(RT_ERR_INVALID, "dead_value must be finite");
    return check_rectangle(Wn, H);
}

size_t cells_of(int n, int s) { return (size_t)((n + s - 1) / s); }

dim3 grid_of(size_t columns, size_t rows, uint32_t *tiles_z) {
    *tiles_z = (uint32_t)((rows + kTileZ - 1) / kTileZ);
    return dim3((unsigned)(*tiles_z * ((columns + kTileX - 1) / kTileX)));
}

int enqueue_subsample(int scale, int white, int Wn, int H, const void *d_hits, void *d_out, hipStream_t stream) {
    const size_t Wl = cells_of(Wn, scale), Hl = cells_of(H, scale);
    uint32_t tiles_z;
    const dim3 grid = grid_of(Wl, Hl, &tiles_z);
    hipLaunchKernelGGL(rt_subsample_kernel, grid, dim3(kTileZ, kTileX), 0, stream, static_cast<const uint4 *>(d_hits),
                       static_cast<uint4 *>(d_out), H, (int)Wl, (int)Hl, scale, white, tiles_z);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

template <int kC, bool kLds>
void launch(dim3 grid, hipStream_t stream, const void *d_hits, const void *d_lo, const void *d_base, void *d_out, void *d_flags,
            const Args &A) {
    hipLaunchKernelGGL((rt_upsample_kernel<kC, kLds>), grid, dim3(kTileZ, kTileX), 0, stream, static_cast<const uint4 *>(d_hits),
                       static_cast<const float *>(d_lo), static_cast<const float *>(d_base), static_cast<float *>(d_out),
                       static_cast<uint8_t *>(d_flags), A);
}

/* the kernel, enqueued on stream; every argument already checked, the device current.  lds: which tap-loading variant */
int enqueue_upsample(const rt_upsample_params *pr, int Wn, int H, const void *d_hits, const void *d_lo, const void *d_base,
                     void *d_out, void *d_flags, hipStream_t stream, bool lds) {
    Args A;
    A.Wn = Wn, A.H = H, A.s = pr->scale, A.Wl = (int)cells_of(Wn, pr->scale), A.Hl = (int)cells_of(H, pr->scale);
    A.squarings = pr->normal_squarings, A.match_color = pr->match_color, A.modulate = pr->modulate;
    A.plane = pr->sigma_plane > 0.0f;
    A.inv = A.plane ? 1.0f / (pr->sigma_plane * pr->sigma_plane) : 0.0f;
    A.dead_value = pr->dead_value;
    const dim3 grid = grid_of((size_t)Wn, (size_t)H, &A.tiles_z);
#if RT_UPSAMPLE_VARIANTS
    if (!lds) {
        pr->channels == 3 ? launch<3, false>(grid, stream, d_hits, d_lo, d_base, d_out, d_flags, A)
                          : launch<1, false>(grid, stream, d_hits, d_lo, d_base, d_out, d_flags, A);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
#endif
    (void)lds;
    pr->channels == 3 ? launch<3, true>(grid, stream, d_hits, d_lo, d_base, d_out, d_flags, A)
                      : launch<1, true>(grid, stream, d_hits, d_lo, d_base, d_out, d_flags, A);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

} // namespace

extern "C" {

int rt_capi_upsample_version(void) { return RT_CAPI_UPSAMPLE_VERSION; }

static int check_subsample(int scale, int white, int Wn, int H, const void *hits, const void *out_lo) {
    int rc = check_scale(scale);
    if (rc) return rc;
    if ((white | 1) != 1) return fail(RT_ERR_INVALID, "white must be 0 or 1");
    if ((rc = check_rectangle(Wn, H))) return rc;
    if (!hits || !out_lo) return fail(RT_ERR_INVALID, "hits / out_lo is NULL");
    return RT_OK;
}

int rt_subsample_hits(int device, int scale, int white, int Wn, int H, const rt_hit *hits, rt_hit *out_lo) {
    int rc = check_subsample(scale, white, Wn, H, hits, out_lo);
    if (rc) return rc;
    if ((rc = rt_internal_check_device(device))) return rc;
    const size_t pixels = (size_t)Wn * (size_t)H, cells = cells_of(Wn, scale) * cells_of(H, scale);
    const HostIn in[1] = {{hits, pixels * sizeof(rt_hit)}};
    const HostOut out[1] = {{out_lo, cells * sizeof(rt_hit)}};
    return staged_call(device, in, 1, out, 1, 0, nullptr, [&](void *const *d_in, void *const *d_out, void *) {
        return enqueue_subsample(scale, white, Wn, H, d_in[0], d_out[0], nullptr);
    });
}

int rt_subsample_hits_device(int device, int scale, int white, int Wn, int H, const void *d_hits, void *d_out_lo,
                             void *hip_stream) {
    int rc = check_subsample(scale, white, Wn, H, d_hits, d_out_lo);
    if (rc) return rc;
    if (((uintptr_t)d_hits & 15u) != 0 || ((uintptr_t)d_out_lo & 15u) != 0)
        return fail(RT_ERR_INVALID, "d_hits and d_out_lo must be 16-byte aligned");
    if ((rc = rt_internal_check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue_subsample(scale, white, Wn, H, d_hits, d_out_lo, static_cast<hipStream_t>(hip_stream));
}

int rt_upsample_guided(int device, const rt_upsample_params *pr, int Wn, int H, const rt_hit *hits, const float *lo,
                       const float *base, float *out, uint8_t *out_flags, double *kernel_ms) {
    int rc = check_params(pr, Wn, H);
    if (rc) return rc;
    if (!hits || !lo || !out) return fail(RT_ERR_INVALID, "hits / lo / out is NULL");
    if ((rc = rt_internal_check_device(device))) return rc;
    const size_t pixels = (size_t)Wn * (size_t)H, cells = cells_of(Wn, pr->scale) * cells_of(H, pr->scale);
    const size_t cb = (size_t)pr->channels * sizeof(float);
    const HostIn in[3] = {{hits, pixels * sizeof(rt_hit)}, {lo, cells * cb}, {base, pixels * cb}};
    const HostOut outs[2] = {{out, pixels * cb}, {out_flags, pixels}};
    return staged_call(device, in, 3, outs, 2, 0, kernel_ms, [&](void *const *d_in, void *const *d_out, void *) {
        return enqueue_upsample(pr, Wn, H, d_in[0], d_in[1], d_in[2], d_out[0], d_out[1], nullptr, true);
    });
}

/* rt_upsample_guided_device's checks and launch; lds: the tap-loading variant (true in a build that has one) */
static int upsample_device(int device, const rt_upsample_params *pr, int Wn, int H, const void *d_hits, const void *d_lo,
                           const void *d_base, void *d_out, void *d_flags, void *hip_stream, bool lds) {
    int rc = check_params(pr, Wn, H);
    if (rc) return rc;
    if (!d_hits || !d_lo || !d_out) return fail(RT_ERR_INVALID, "d_hits / d_lo / d_out is NULL");
    if (((uintptr_t)d_hits & 15u) != 0) return fail(RT_ERR_INVALID, "d_hits must be 16-byte aligned");
    if ((((uintptr_t)d_lo | (uintptr_t)d_base | (uintptr_t)d_out) & 3u) != 0)
        return fail(RT_ERR_INVALID, "d_lo, d_base and d_out must be 4-byte aligned");
    const size_t cb = (size_t)pr->channels * sizeof(float);
    if (overlap(d_out, (size_t)Wn * (size_t)H * cb, d_lo, cells_of(Wn, pr->scale) * cells_of(H, pr->scale) * cb))
        return fail(RT_ERR_INVALID, "d_out overlaps d_lo");
    if ((rc = rt_internal_check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue_upsample(pr, Wn, H, d_hits, d_lo, d_base, d_out, d_flags, static_cast<hipStream_t>(hip_stream), lds);
}

int rt_upsample_guided_device(int device, const rt_upsample_params *pr, int Wn, int H, const void *d_hits, const void *d_lo,
                              const void *d_base, void *d_out, void *d_out_flags, void *hip_stream) {
    return upsample_device(device, pr, Wn, H, d_hits, d_lo, d_base, d_out, d_out_flags, hip_stream, true);
}

#if RT_UPSAMPLE_VARIANTS
/* development aid, not in the header: rt_upsample_guided_device with the tap-loading variant named (lds 0 / 1), for the
 * comparison recorded in profiles/upsample_experiments.txt */
int rt_internal_upsample_variant(int device, const rt_upsample_params *pr, int Wn, int H, const void *d_hits, const void *d_lo,
                                 const void *d_base, void *d_out, void *d_flags, void *hip_stream, int lds) {
    return upsample_device(device, pr, Wn, H, d_hits, d_lo, d_base, d_out, d_flags, hip_stream, lds != 0);
}
#endif

} // extern "C"
