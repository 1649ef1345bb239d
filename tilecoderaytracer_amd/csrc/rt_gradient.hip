/*
 * rt_gradient.hip -- implementation of include/rt_gradient.h: temporal-gradient weights for an accumulated history.  The header is
 * the definition; the kernel is bit-exact to it (the library's arithmetic flags: no contraction, correctly rounded divide,
 * denormals kept).
 *
 * SHAPE.  One launch a call, one lane a pixel, a workgroup of four wavefronts: 64 consecutive z of four
 * columns, rt_clamp.hip's and rt_upsample.hip's tile.  A lane reads its own record, value, moments and length; only a lane that
 * is alive with a history longer than one walks the (2r+2)^2 cells of its window, behind a branch a wavefront without such a lane
 * skips -- a first frame costs its own words.  The kernels are specialised on channels and on then_hits given or NULL; scale and
 * radius are kernel arguments (the window is a pair of loops over at most 36 cells, none of them indexing a private array).  Two
 * forms of the window's reads:
 *   direct   each lane loads its cells' words from global memory -- the object word, the two 16-byte thirds of the record that
 *            hold the normal and colour | flags, the cell's words of now_lo and then_lo and, with then_hits, that record's object
 *            and flag words -- and computes the cell's d and m itself; a cell that does not exist reads cell (i0, j0), which
 *            always does, and is dropped by a select.
 *   LDS      the workgroup stages the cells its pixels can reach, at most 7 x 37 of them (s = 2, r = 2: 2 + 5 by 32 + 5) --
 *            key {object, colour bits (zeros without match_color)}, aux {normal, side | dead << 2} and {d, m} computed ONCE a
 *            cell, 40 bytes a cell, 10 360 bytes (10 624 with the barrier's reduction) -- and the lanes walk the window there; a
 *            cell outside the cell grid is staged dead, so the walk has no bounds.  A workgroup none of whose lanes walks
 *            stages nothing.
 * The library has the LDS form: at 4096 x 4096 it takes 0.48 ms against the direct form's 1.25 at s = 2, r = 1 with three
 * channels, a device copy of the call's bytes taking 0.37, and it is ahead in every setting and with one channel too.
 * RT_GRADIENT_LDS picks the form the library has; -DRT_GRADIENT_VARIANTS=1 (scripts/gradient_experiments.py) builds both and
 * exports the switch between them, rt_internal_gradient_variant().  profiles/gradient_experiments.txt has the numbers.
 *
 * IN PLACE.  out_value, out_moments and out_len may be value, moments and len: a lane reads those at its own pixel alone, before
 * it writes them, and cur, hits and the cell buffers are never written.  Every output cell of the rectangle is written exactly
 * once, dead pixels too, with plain vector stores.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/rt_gradient.h"
#include "rt_host.h"

static_assert(sizeof(rt_hit) == 48, "rt_hit layout");
static_assert(sizeof(rt_gradient_params) == 32, "rt_gradient_params layout");

#ifndef RT_GRADIENT_LDS
#define RT_GRADIENT_LDS 1              /* the window's reads in the library: 0 direct loads, 1 (kept) cells staged in LDS */
#endif
#ifndef RT_GRADIENT_VARIANTS
#define RT_GRADIENT_VARIANTS 0         /* 1: both forms, and the entry point that names one */
#endif

namespace {

constexpr int kTileZ = 64, kTileX = 4;                 /* a workgroup: 4 wavefronts, each 64 consecutive z of one column */
constexpr double kMaxPixels = 2.0e9 * 4.0 * 4.0 / 60.0; /* rt_render_gbuffer's limit: 3.2e10 bytes of colours and records */
constexpr uint32_t kDead = 4u;                         /* aux.w: flags & 3, and this bit for a miss or a light */
constexpr int kMaxRadius = 2, kMinScale = 2;
/* the cells a tile's pixels reach: those under the tile, at most 2 along x (a tile starts on a multiple of 4) and 32 along z,
 * and 2r + 1 more */
constexpr int kCellsX = 2 + 2 * kMaxRadius + 1, kCellsZ = kTileZ / kMinScale + 2 * kMaxRadius + 1;

/* the kernels' arguments.  The history's inputs and outputs carry no __restrict__: they may be the same buffers. */
struct GradientArgs {
    const float *cur;
    const uint4 *hits;
    const float *value, *moments, *len;
    const float *now_lo, *then_lo;
    const uint4 *lo_hits, *then_hits;
    float *out_value, *out_moments, *out_len, *out_variance, *out_lambda;
    uint8_t *out_flags;
    int Wn, H, Wl, Hl, scale, radius;
    uint32_t tiles_z;
    uint32_t color_mask;                               /* ~0 with match_color, else 0 */
    float normal_cos, gain, lambda_min, den_floor;
};

template <int kC>
__device__ __forceinline__ float gradient_lum(const float *c) {
    return kC == 3 ? (0.25f * c[0] + 0.5f * c[1]) + 0.25f * c[2] : c[0];
}

/* the header's per-cell lines: d and m of cell q, whose record's object and flag words are oq and fq */
template <int kC, bool kThen>
__device__ __forceinline__ void gradient_cell(const GradientArgs &a, int64_t q, uint32_t oq, uint32_t fq, float *d, float *m) {
    float cn[kC], ct[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) cn[k] = a.now_lo[q * kC + k], ct[k] = a.then_lo[q * kC + k];
    const float ln = gradient_lum<kC>(cn), lt = gradient_lum<kC>(ct);
    float dd = ln - lt;
    dd = dd < 0.0f ? -dd : dd;
    const float mm = lt > ln ? lt : ln;
    if (kThen) {
        const uint32_t ot = a.then_hits[3 * q].x, ft = a.then_hits[3 * q + 2].w;
        dd = ((ot ^ oq) | ((ft ^ fq) & 3u)) != 0u ? mm : dd;
    }
    *d = dd, *m = mm;
}

/* what the window gives a pixel */
struct Cells {
    int cnt;
    float num, den;
    /* header step 2's line for a cell, taken only if `counts` (selects: the caller's loads stay unconditional) */
    __device__ __forceinline__ void add(bool counts, float d, float m) {
        cnt = counts ? cnt + 1 : cnt;
        num = counts ? num + d : num;
        den = counts ? den + m : den;
    }
};

/* header steps 2's end to 6 and the stores of pixel p; walked: the pixel is alive with a history longer than one, and w is its
 * window; c: the pixel's sample, read only if walked */
template <int kC>
__device__ __forceinline__ void gradient_finish(const GradientArgs &a, int64_t p, bool walked, const Cells &w, const float *c,
                                                const float *v, float m1, float m2, float L) {
    float vo[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) vo[k] = v[k];
    float m1o = m1, m2o = m2, Lo = L, lambda_out = 0.0f;
    uint8_t flag = 0;
    if (walked) {
        if (w.cnt == 0) {
            flag = 2;
        } else {
            const float t = w.den > a.den_floor ? w.num / w.den : 0.0f;
            float lambda = a.gain * t;
            lambda = lambda > 1.0f ? 1.0f : lambda;
            lambda_out = lambda > 0.0f ? lambda : 0.0f;
            if (lambda > a.lambda_min) {
                const float l = gradient_lum<kC>(c), ll = l * l;
                if (lambda == 1.0f) {
                    flag = 3;
#pragma unroll
                    for (int k = 0; k < kC; ++k) vo[k] = c[k];
                    m1o = l, m2o = ll, Lo = 1.0f;
                } else {
                    flag = 1;
#pragma unroll
                    for (int k = 0; k < kC; ++k) vo[k] = v[k] + lambda * (c[k] - v[k]);
                    m1o = m1 + lambda * (l - m1);
                    m2o = m2 + lambda * (ll - m2);
                    const float al = 1.0f / L;
                    const float a2 = al + lambda * (1.0f - al);
                    Lo = 1.0f / a2;
                    if (!(Lo >= 1.0f)) Lo = 1.0f;
                    if (!(Lo <= L)) Lo = L;
                }
            }
        }
    }
    const float t = m2o - m1o * m1o;
#pragma unroll
    for (int k = 0; k < kC; ++k) a.out_value[p * kC + k] = vo[k];
    a.out_moments[p * 2] = m1o, a.out_moments[p * 2 + 1] = m2o;
    a.out_len[p] = Lo;
    if (a.out_variance) a.out_variance[p] = t > 0.0f ? t : 0.0f;
    if (a.out_lambda) a.out_lambda[p] = lambda_out;
    if (a.out_flags) a.out_flags[p] = flag;
}

} // namespace

#if !RT_GRADIENT_LDS || RT_GRADIENT_VARIANTS
/* the window read with direct loads */
template <int kC, bool kThen>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_gradient_direct_kernel(const GradientArgs a) {
    const uint32_t tz = blockIdx.x % a.tiles_z, tx = blockIdx.x / a.tiles_z;
    const int64_t x64 = (int64_t)tx * kTileX + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    const int64_t z64 = (int64_t)tz * kTileZ + threadIdx.x;
    if (x64 >= a.Wn || z64 >= a.H) return;              /* (no barrier below: a thread without a pixel leaves) */
    const int x = (int)x64, z = (int)z64;
    const int64_t p = x64 * (int64_t)a.H + z;
    const uint32_t op = a.hits[3 * p].x;
    const uint4 p2 = a.hits[3 * p + 2];
    const float m1 = a.moments[p * 2], m2 = a.moments[p * 2 + 1], L = a.len[p];
    float v[kC], c[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) v[k] = a.value[p * kC + k], c[k] = 0.0f;
    const bool dead = (int32_t)op < 0 || (p2.w & (uint32_t)RT_HIT_LIGHT) != 0u;
    const bool walked = !dead && L > 1.0f;
    Cells w{0, 0.0f, 0.0f};
    if (walked) {
        const uint4 p1 = a.hits[3 * p + 1];
        const float npx = __uint_as_float(p1.y), npy = __uint_as_float(p1.z), npz = __uint_as_float(p1.w);
#pragma unroll
        for (int k = 0; k < kC; ++k) c[k] = a.cur[p * kC + k];
        const int i0 = x / a.scale, j0 = z / a.scale, n = 2 * a.radius + 2;
        for (int da = 0; da < n; ++da) {
            const int i = i0 - a.radius + da;
            if (i < 0 || i >= a.Wl) continue;           /* (wave-uniform) */
            const int64_t row = (int64_t)i * (int64_t)a.Hl;
            for (int db = 0; db < n; ++db) {
                const int j = j0 - a.radius + db;
                const bool inside = j >= 0 && j < a.Hl;
                const int64_t q = row + (inside ? j : j0);          /* a cell that does not exist reads this row's own j0 */
                const uint32_t oq = a.lo_hits[3 * q].x;
                const uint4 q1 = a.lo_hits[3 * q + 1], q2 = a.lo_hits[3 * q + 2];
                float d, m;
                gradient_cell<kC, kThen>(a, q, oq, q2.w, &d, &m);
                const bool dead_q = (int32_t)oq < 0 || (q2.w & (uint32_t)RT_HIT_LIGHT) != 0u;
                const uint32_t differ = (oq ^ op) | ((q2.w ^ p2.w) & 3u) |
                                        (((q2.x ^ p2.x) | (q2.y ^ p2.y) | (q2.z ^ p2.z)) & a.color_mask);
                const float t = (npx * __uint_as_float(q1.y) + npy * __uint_as_float(q1.z)) + npz * __uint_as_float(q1.w);
                w.add(inside & !dead_q & (differ == 0u) & (t >= a.normal_cos), d, m);
            }
        }
    }
    gradient_finish<kC>(a, p, walked, w, c, v, m1, m2, L);
}
#endif

#if RT_GRADIENT_LDS || RT_GRADIENT_VARIANTS
/* the window read from cells staged in LDS: the same arithmetic in the same order */
template <int kC, bool kThen>
__global__ __launch_bounds__(kTileZ *kTileX) void rt_gradient_lds_kernel(const GradientArgs a) {
    __shared__ uint4 s_key[kCellsX * kCellsZ], s_aux[kCellsX * kCellsZ];
    __shared__ float2 s_dm[kCellsX * kCellsZ];
    const uint32_t tz = blockIdx.x % a.tiles_z, tx = blockIdx.x / a.tiles_z;
    const int64_t x0 = (int64_t)tx * kTileX, z0 = (int64_t)tz * kTileZ;
    const int64_t x64 = x0 + threadIdx.y, z64 = z0 + threadIdx.x;
    const bool mine = x64 < a.Wn && z64 < a.H;          /* (a thread without a pixel stays for the barriers) */
    const int64_t p = mine ? x64 * (int64_t)a.H + z64 : 0;
    float m1 = 0.0f, m2 = 0.0f, L = 0.0f;
    float v[kC], c[kC];
#pragma unroll
    for (int k = 0; k < kC; ++k) v[k] = c[k] = 0.0f;
    uint32_t op = 0u;
    uint4 p2 = make_uint4(0u, 0u, 0u, 0u);
    bool walked = false;
    if (mine) {
        op = a.hits[3 * p].x, p2 = a.hits[3 * p + 2];
        m1 = a.moments[p * 2], m2 = a.moments[p * 2 + 1], L = a.len[p];
#pragma unroll
        for (int k = 0; k < kC; ++k) v[k] = a.value[p * kC + k];
        walked = !((int32_t)op < 0 || (p2.w & (uint32_t)RT_HIT_LIGHT) != 0u) && L > 1.0f;
    }
    Cells w{0, 0.0f, 0.0f};
    if (__syncthreads_or(walked)) {
        /* the staged cells: columns ia .. ia + ni - 1 and rows ja .. ja + nj - 1 of the cell grid (uniform over the workgroup).
         * The tile's last pixels may not exist; the cells under them are staged all the same, dead where the grid ends. */
        const int s = a.scale, r = a.radius;
        const int ia = (int)(x0 / s) - r, ja = (int)(z0 / s) - r;
        const int ni = (int)((x0 + kTileX - 1) / s) + r + 1 - ia + 1, nj = (int)((z0 + kTileZ - 1) / s) + r + 1 - ja + 1;
        for (int cell = (int)(threadIdx.y * kTileZ + threadIdx.x); cell < ni * nj; cell += kTileX * kTileZ) {
            const int ci = cell / nj, cj = cell - ci * nj;
            const int i = ia + ci, j = ja + cj;
            uint4 key = make_uint4(0u, 0u, 0u, 0u), aux = make_uint4(0u, 0u, 0u, kDead);     /* outside the grid: dead */
            float d = 0.0f, m = 0.0f;
            if (i >= 0 && i < a.Wl && j >= 0 && j < a.Hl) {
                const int64_t q = (int64_t)i * (int64_t)a.Hl + j;
                const uint32_t oq = a.lo_hits[3 * q].x;
                const uint4 q1 = a.lo_hits[3 * q + 1], q2 = a.lo_hits[3 * q + 2];
                const bool dead_q = (int32_t)oq < 0 || (q2.w & (uint32_t)RT_HIT_LIGHT) != 0u;
                key = make_uint4(oq, q2.x & a.color_mask, q2.y & a.color_mask, q2.z & a.color_mask);
                aux = make_uint4(q1.y, q1.z, q1.w, (q2.w & 3u) | (dead_q ? kDead : 0u));
                gradient_cell<kC, kThen>(a, q, oq, q2.w, &d, &m);
            }
            s_key[cell] = key, s_aux[cell] = aux, s_dm[cell] = make_float2(d, m);
        }
        __syncthreads();
        if (walked) {
            const uint4 p1 = a.hits[3 * p + 1];
            const float npx = __uint_as_float(p1.y), npy = __uint_as_float(p1.z), npz = __uint_as_float(p1.w);
            const uint4 kp = make_uint4(op, p2.x & a.color_mask, p2.y & a.color_mask, p2.z & a.color_mask);
#pragma unroll
            for (int k = 0; k < kC; ++k) c[k] = a.cur[p * kC + k];
            /* the window's first cell, in staged coordinates: (i0 - r) - ia and (j0 - r) - ja */
            const int ci0 = (int)(x64 / s) - r - ia, cj0 = (int)(z64 / s) - r - ja, n = 2 * r + 2;
            for (int da = 0; da < n; ++da) {
                const int row = (ci0 + da) * nj + cj0;
                for (int db = 0; db < n; ++db) {
                    const uint4 kq = s_key[row + db], aq = s_aux[row + db];
                    const float2 dm = s_dm[row + db];
                    const uint32_t differ = (kq.x ^ kp.x) | (kq.y ^ kp.y) | (kq.z ^ kp.z) | (kq.w ^ kp.w) | ((aq.w ^ p2.w) & 3u);
                    const float t = (npx * __uint_as_float(aq.x) + npy * __uint_as_float(aq.y)) + npz * __uint_as_float(aq.z);
                    w.add(((aq.w & kDead) == 0u) & (differ == 0u) & (t >= a.normal_cos), dm.x, dm.y);
                }
            }
        }
    }
    if (!mine) return;
    gradient_finish<kC>(a, p, walked, w, c, v, m1, m2, L);
}
#endif

namespace {

/* the header's checks up to the buffers, in its order */
int check_shape(const rt_gradient_params *pr, int Wn, int H) {
    if (!pr) return fail(RT_ERR_INVALID, "params is NULL");
    if (pr->channels != 1 && pr->channels != 3) return fail(RT_ERR_INVALID, "channels must be 1 or 3");
    if (pr->scale < kMinScale || pr->scale > 8) return fail(RT_ERR_INVALID, "scale must be 2..8");
    if (pr->radius < 0 || pr->radius > kMaxRadius) return fail(RT_ERR_INVALID, "radius must be 0..2");
    if ((pr->match_color | 1) != 1) return fail(RT_ERR_INVALID, "match_color must be 0 or 1");
    if (!(pr->normal_cos >= -1.0f && pr->normal_cos <= 1.0f)) return fail(RT_ERR_INVALID, "normal_cos must be in -1..1");
    if (!(pr->gain >= 0.0f) || std::isinf(pr->gain)) return fail(RT_ERR_INVALID, "gain must be finite and >= 0");
    if (!(pr->lambda_min >= 0.0f && pr->lambda_min <= 1.0f)) return fail(RT_ERR_INVALID, "lambda_min must be in 0..1");
    if (!(pr->den_floor >= 0.0f) || std::isinf(pr->den_floor)) return fail(RT_ERR_INVALID, "den_floor must be finite and >= 0");
    if (Wn <= 0 || H <= 0) return fail(RT_ERR_INVALID, "need Wn, H > 0");
    if ((double)Wn * (double)H > kMaxPixels) return fail(RT_ERR_INVALID, "rectangle too large for its values and records");
    /* a launch has fewer than 2^32 work-items: a workgroup is 256 of them whatever part of its 4 x 64 pixels exists */
    const uint64_t tiles = (((uint64_t)Wn + kTileX - 1) / kTileX) * (((uint64_t)H + kTileZ - 1) / kTileZ);
    if (tiles >= (1ull << 24)) return fail(RT_ERR_INVALID, "rectangle too thin: 2^24 or more tiles of 4 x 64 pixels");
    return RT_OK;
}

constexpr int kIn = 9, kOut = 6;

struct Buffers {             /* the call's buffers, in device memory */
    const void *in[kIn];     /* cur, hits, value, moments, len, now_lo, then_lo, lo_hits, then_hits */
    void *out[kOut];         /* out_value, out_moments, out_len, out_variance, out_lambda, out_flags */
};

/* the bytes of every buffer of a call */
void sizes(const rt_gradient_params *pr, int Wn, int H, size_t *in_bytes, size_t *out_bytes) {
    const size_t pixels = (size_t)Wn * (size_t)H, cb = (size_t)pr->channels * sizeof(float);
    const size_t s = (size_t)pr->scale, cells = (((size_t)Wn + s - 1) / s) * (((size_t)H + s - 1) / s);
    const size_t in[kIn] = {pixels * cb, pixels * sizeof(rt_hit), pixels * cb,           pixels * 8,            pixels * 4,
                            cells * cb,  cells * cb,              cells * sizeof(rt_hit), cells * sizeof(rt_hit)};
    const size_t out[kOut] = {pixels * cb, pixels * 8, pixels * 4, pixels * 4, pixels * 4, pixels};
    for (int k = 0; k < kIn; ++k) in_bytes[k] = in[k];
    for (int k = 0; k < kOut; ++k) out_bytes[k] = out[k];
}

using Launch = void (*)(dim3, hipStream_t, const GradientArgs &);

#if !RT_GRADIENT_LDS || RT_GRADIENT_VARIANTS
template <int kC, bool kThen>
void launch_direct(dim3 grid, hipStream_t stream, const GradientArgs &a) {
    hipLaunchKernelGGL((rt_gradient_direct_kernel<kC, kThen>), grid, dim3(kTileZ, kTileX), 0, stream, a);
}
const Launch kDirect[2][2] = {{launch_direct<1, false>, launch_direct<1, true>}, {launch_direct<3, false>, launch_direct<3, true>}};
#endif
#if RT_GRADIENT_LDS || RT_GRADIENT_VARIANTS
template <int kC, bool kThen>
void launch_lds(dim3 grid, hipStream_t stream, const GradientArgs &a) {
    hipLaunchKernelGGL((rt_gradient_lds_kernel<kC, kThen>), grid, dim3(kTileZ, kTileX), 0, stream, a);
}
const Launch kLds[2][2] = {{launch_lds<1, false>, launch_lds<1, true>}, {launch_lds<3, false>, launch_lds<3, true>}};
#endif

#if RT_GRADIENT_VARIANTS
bool g_lds = RT_GRADIENT_LDS != 0;
#endif

/* the one launch, enqueued on stream; every argument already checked, the device current */
int enqueue(const rt_gradient_params *pr, int Wn, int H, const Buffers &b, hipStream_t stream) {
    const uint32_t tiles_z = (uint32_t)((H + kTileZ - 1) / kTileZ);
    const dim3 grid(tiles_z * (uint32_t)(((int64_t)Wn + kTileX - 1) / kTileX));
    const int s = pr->scale;
    const auto f = [](const void *p) { return static_cast<const float *>(p); };
    const auto g = [](void *p) { return static_cast<float *>(p); };
    const GradientArgs a{f(b.in[0]), static_cast<const uint4 *>(b.in[1]), f(b.in[2]), f(b.in[3]), f(b.in[4]), f(b.in[5]), f(b.in[6]),
                         static_cast<const uint4 *>(b.in[7]), static_cast<const uint4 *>(b.in[8]), g(b.out[0]), g(b.out[1]),
                         g(b.out[2]), g(b.out[3]), g(b.out[4]), static_cast<uint8_t *>(b.out[5]), Wn, H, (Wn + s - 1) / s,
                         (H + s - 1) / s, s, pr->radius, tiles_z, pr->match_color ? ~0u : 0u, pr->normal_cos, pr->gain,
                         pr->lambda_min, pr->den_floor};
    const int c = pr->channels == 3, t = b.in[8] != nullptr;
#if RT_GRADIENT_VARIANTS
    (g_lds ? kLds : kDirect)[c][t](grid, stream, a);
#elif RT_GRADIENT_LDS
    kLds[c][t](grid, stream, a);
#else
    kDirect[c][t](grid, stream, a);
#endif
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

const char *const kNull = "cur / hits / value / moments / len / now_lo / then_lo / lo_hits / out_value / out_moments / out_len is NULL";

} // namespace

extern "C" {

int rt_capi_gradient_version(void) { return RT_CAPI_GRADIENT_VERSION; }

#if RT_GRADIENT_VARIANTS
/* 0: direct loads; 1: through LDS; returns what was set before */
int rt_internal_gradient_variant(int lds) {
    const int before = g_lds;
    g_lds = lds != 0;
    return before;
}
#endif

int rt_gradient_reweight(int device, const rt_gradient_params *pr, int Wn, int H, const float *cur, const rt_hit *hits,
                         const float *value, const float *moments, const float *len, const float *now_lo, const float *then_lo,
                         const rt_hit *lo_hits, const rt_hit *then_hits, float *out_value, float *out_moments, float *out_len,
                         float *out_variance, float *out_lambda, uint8_t *out_flags, double *kernel_ms) {
    int rc = check_shape(pr, Wn, H);
    if (rc) return rc;
    if (!cur || !hits || !value || !moments || !len || !now_lo || !then_lo || !lo_hits || !out_value || !out_moments || !out_len)
        return fail(RT_ERR_INVALID, kNull);
    if ((rc = rt_internal_check_device(device))) return rc;
    size_t in_bytes[kIn], out_bytes[kOut];
    sizes(pr, Wn, H, in_bytes, out_bytes);
    const void *ins[kIn] = {cur, hits, value, moments, len, now_lo, then_lo, lo_hits, then_hits};
    void *outs[kOut] = {out_value, out_moments, out_len, out_variance, out_lambda, out_flags};
    HostIn in[kIn];
    HostOut out[kOut];
    for (int k = 0; k < kIn; ++k) in[k] = HostIn{ins[k], in_bytes[k]};
    for (int k = 0; k < kOut; ++k) out[k] = HostOut{outs[k], out_bytes[k]};
    return staged_call(device, in, kIn, out, kOut, 0, kernel_ms, [&](void *const *d_in, void *const *d_out, void *) {
        Buffers b;
        for (int k = 0; k < kIn; ++k) b.in[k] = d_in[k];
        for (int k = 0; k < kOut; ++k) b.out[k] = d_out[k];
        return enqueue(pr, Wn, H, b, nullptr);
    });
}

int rt_gradient_reweight_device(int device, const rt_gradient_params *pr, int Wn, int H, const void *d_cur, const void *d_hits,
                                const void *d_value, const void *d_moments, const void *d_len, const void *d_now_lo,
                                const void *d_then_lo, const void *d_lo_hits, const void *d_then_hits, void *d_out_value,
                                void *d_out_moments, void *d_out_len, void *d_out_variance, void *d_out_lambda, void *d_out_flags,
                                void *hip_stream) {
    int rc = check_shape(pr, Wn, H);
    if (rc) return rc;
    if (!d_cur || !d_hits || !d_value || !d_moments || !d_len || !d_now_lo || !d_then_lo || !d_lo_hits || !d_out_value ||
        !d_out_moments || !d_out_len)
        return fail(RT_ERR_INVALID, kNull);
    if ((((uintptr_t)d_hits | (uintptr_t)d_lo_hits | (uintptr_t)d_then_hits) & 15u) != 0)
        return fail(RT_ERR_INVALID, "d_hits, d_lo_hits and d_then_hits must be 16-byte aligned");
    if ((((uintptr_t)d_cur | (uintptr_t)d_value | (uintptr_t)d_moments | (uintptr_t)d_len | (uintptr_t)d_now_lo |
          (uintptr_t)d_then_lo | (uintptr_t)d_out_value | (uintptr_t)d_out_moments | (uintptr_t)d_out_len |
          (uintptr_t)d_out_variance | (uintptr_t)d_out_lambda) & 3u) != 0)
        return fail(RT_ERR_INVALID, "the float buffers must be 4-byte aligned");
    size_t in_bytes[kIn], out_bytes[kOut];
    sizes(pr, Wn, H, in_bytes, out_bytes);
    const Buffers b{{d_cur, d_hits, d_value, d_moments, d_len, d_now_lo, d_then_lo, d_lo_hits, d_then_hits},
                    {d_out_value, d_out_moments, d_out_len, d_out_variance, d_out_lambda, d_out_flags}};
    /* outputs 0..2 may be inputs 2..4 exactly (in place), and nothing else may share a byte */
    for (int o = 0; o < kOut; ++o) {
        for (int q = o + 1; q < kOut; ++q)
            if (overlap(b.out[o], out_bytes[o], b.out[q], out_bytes[q])) return fail(RT_ERR_INVALID, "an output overlaps another output");
        for (int q = 0; q < kIn; ++q) {
            if (o < 3 && q == o + 2 && b.out[o] == b.in[q]) continue;   /* in place: the same buffer, the same bytes */
            if (overlap(b.out[o], out_bytes[o], b.in[q], in_bytes[q]))
                return fail(RT_ERR_INVALID, q < 2    ? "an output overlaps d_cur or d_hits"
                                            : q >= 5 ? "an output overlaps a cell buffer"
                                                     : "an output overlaps an input that is not its own, or its own input partially");
        }
    }
    if ((rc = rt_internal_check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue(pr, Wn, H, b, static_cast<hipStream_t>(hip_stream));
}

} // extern "C"
