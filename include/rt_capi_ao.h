/*
 * rt_capi_ao.h -- ambient occlusion from hit records: for every rt_hit of a batch (a G-buffer's records, rt_intersect_rays'
 * output, or the caller's own), the fraction of n x n stratified directions of the hemisphere around the record's normal that
 * are free for a distance R.  The records stay on the GPU, every sample is the occlusion query's scan, and the result is a
 * grey value per record that rt_denoise and rt_encode_image take as it is.  Plain C99, versioned on its own
 * (RT_CAPI_AO_VERSION / rt_capi_ao_version()); rt_capi_query.h, which this header includes for rt_hit, and every other header
 * are unchanged, and no existing call changes a bit.
 *
 * THE DEFINITION.  All arithmetic is IEEE fp32, one rounding per operation, no contraction.  add, sub, scale, normalize and
 * length are the reference's vector3d operations in the order written (normalize: sqrtf of the left-to-right sum of squares,
 * then three divides); H() is the 32-bit hash lowbias32 and cross() the cross product, both as in rt_capi_soft.h:
 *   H(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
 *   cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)
 * For record h = hits[i], with n = samples, R = radius and key = key0 + (uint32_t)i (wrapping):
 *
 *   h.object < 0 or (h.flags & RT_HIT_LIGHT):   ao = 1.0f  (nothing is read from the scene)
 *   P = h.point;  N = h.normal;  if (h.flags & RT_HIT_INSIDE) N = (-N.x, -N.y, -N.z)
 *   A = fabsf(N.x) < 0.5f ? (1,0,0) : (0,1,0);   U = normalize(cross(A, N));   V = cross(N, U)
 *   g = H(H(seed ^ 0x9e3779b9u) ^ key);          step = 2.0f / (float)n
 *   for i, j in [0, n), s = i*n + j:
 *       hs  = H(g ^ s)
 *       xi1 = (float)(hs >> 8) * 0x1p-24f;       xi2 = (float)(H(hs ^ 0x9e3779b9u) >> 8) * 0x1p-24f
 *       a   = ((float)i + xi1) * step - 1.0f;    b   = ((float)j + xi2) * step - 1.0f
 *       dx  = a * sqrtf(1.0f - (b*b) * 0.5f);    dy  = b * sqrtf(1.0f - (a*a) * 0.5f)
 *       w   = (1.0f - dx*dx) - dy*dy;            dz  = w > 0 ? sqrtf(w) : 0.0f
 *       D   = add(add(scale(U, dx), scale(V, dy)), scale(N, dz))
 *       Q   = add(P, scale(D, R))
 *       open <=> !inShadeCollisionDetection(Ray(P, sub(Q, P)), length(sub(Q, P)))
 *   ao = (float)(number of open samples) / (float)(n*n)
 *
 * (a, b) is the jittered point of stratum (i, j) of the square [-1, 1]^2, (dx, dy) its image on the unit disc (the soft
 * shadows' square-to-disc map) and D the disc point lifted to the hemisphere.
 *
 * THE SAME VERDICT AS THE OCCLUSION QUERY.  Sample s of record i has exactly the verdict rt_occluded_rays gives the segment
 * {P, Q}: the same scan over [shadow_begin, shadow_end) of the scene with lights skipped, blocking on distance < |Q - P|, and
 * the same treatment of NaN and infinite coordinates (whatever the record holds, the sample is open or not as that segment is).
 *
 * THE KEY.  Record i samples with key0 + i, so a strip of a frame launched with key0 = x0 * H is bit-identical to the same
 * columns of the whole frame.  rows is a layout hint only and never changes a result, as for the ray queries: record i is
 * cell (i / rows, i % rows) of an n_cols x rows grid tiled like an image; for a frame's records rows is H, record i being
 * pixel (i / H, i % H).  rows > n is read as rows = n.
 *
 * THE OUTPUT.  channels 1: out_ao[i].  channels 3: out_ao[3i .. 3i+2], all three equal -- a grey frame in rt_render's layout,
 * which rt_denoise (with the same records) and rt_encode_image take directly.
 *
 * LIMITS.  The directions are cosine-distributed through the disc lift and carry no further weighting: ao is the plain
 * fraction of open ones.  An inside hit (RT_HIT_INSIDE) looks into the sphere that contains it.  Glass blocks fully: the scan
 * knows no transmission.  A plane's record already carries the reference's 1e-3 offset along its normal; a sphere's record
 * lies on the sphere and relies on the sphere test's `v < 0` rejection for its own sphere.  Not provided: distance falloff,
 * bent normals, importance weights, applying the value to colours (the reference's shading has no ambient term to scale;
 * callers multiply what they like), supersampled frames, the counting build (rt_render_stats), several GPUs.
 *
 * SHADING.  AO is geometry: on any scene (image textures, refraction, area lights) the call runs the same kernels and gives
 * the same bits as on the plain geometry, as rt_occluded_rays does.  The scene's shadow seed is not used; the call has its own.
 *
 * n = 0 is RT_OK and launches nothing.  These are RT_ERR_INVALID, checked in this order before any device work: the scene is
 * NULL; params is NULL; samples outside 1..RT_AO_MAX_SAMPLES; radius not finite or not > 0; channels neither 1 nor 3; n < 0;
 * rows < 1; the records or the output NULL while n > 0; n > 533 333 333 (rt_render_gbuffer's record limit); for the device
 * call, d_hits not 16-byte aligned, then d_out_ao not 4-byte aligned.  Host and device behaviour, error texts,
 * rt_last_error(), rt_get_timing() (kernel ms, download ms), the handle's lock and thread safety are as for rt_occluded_rays
 * and rt_occluded_rays_device; rt_get_launch_info() and rt_get_launch_kernel() name the rt_ao_kernel* that ran (rt_ao_kernel,
 * _items, _large, _clusters, _clusters_wide: the scene's table mode, chosen as for any batch) and its tile shape in cells.
 *
 * Speed-only options (rt_capi_tuning.h) apply as for a query launch ("first_row", "tile_z", "cull", "fast", "tables", "wide",
 * "tile_prio"); "help" does not apply and there is no bounce stack.
 */
#ifndef RT_CAPI_AO_H_
#define RT_CAPI_AO_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_AO_VERSION 1
#define RT_AO_MAX_SAMPLES 8

typedef struct rt_ao_params {
    int32_t samples;    /* n: n x n stratified directions per record, 1..RT_AO_MAX_SAMPLES */
    float radius;       /* R: how far a direction is followed, finite, > 0 */
    uint32_t seed;
    uint32_t key0;      /* record i samples with key = key0 + (uint32_t)i (wraps) */
    int32_t channels;   /* 1: out[i]; 3: out[3i .. 3i+2], all equal */
} rt_ao_params;         /* 20 bytes */

int rt_capi_ao_version(void);

/* host memory, synchronous (as rt_occluded_rays): n records in, n * channels floats out */
int rt_ambient_occlusion(rt_scene *scene, const rt_ao_params *params, int n, int rows, const rt_hit *hits, float *out_ao);

/* device memory on the scene's device, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising
 * (as rt_occluded_rays_device); params is read before the call returns, the records must stay alive until the stream has
 * drained.  d_hits is 48 n bytes, 16-byte aligned; d_out_ao is 4 n channels bytes, 4-byte aligned. */
int rt_ambient_occlusion_device(rt_scene *scene, const rt_ao_params *params, int n, int rows, const void *d_hits, void *d_out_ao,
                                void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_AO_H_ */
