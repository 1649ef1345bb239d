/*
 * rt_capi_indirect.h -- one diffuse bounce from hit records: for every rt_hit of a batch (a G-buffer's records,
 * rt_intersect_rays' output, or the caller's own), the light that n x n stratified directions of the hemisphere around the
 * record's normal bring in, weighted by the record's colour and its object's diffuse coefficient, added to a base colour if
 * there is one.  The records stay on the GPU, the gather rays are generated there, traced as ray batches (rt_capi_rays.h) and
 * averaged there; nothing but the result crosses the bus.  Plain C99, versioned on its own (RT_CAPI_INDIRECT_VERSION /
 * rt_capi_indirect_version()); rt_capi_query.h, which this header includes for rt_hit, and every other header are unchanged,
 * and no existing call changes a bit.
 *
 * THE DEFINITION, which the GPU meets bit for bit.  All arithmetic is IEEE fp32, one rounding per operation, no contraction.
 * For record h = hits[i], with n = samples, S = n*n and key = key0 + (uint32_t)i (wrapping):
 *
 *   dead <=> h.object < 0 or (h.flags & RT_HIT_LIGHT).  A dead record's S rays are six +0.0f each (what rt_trace_rays makes
 *       of a ray with E == T is its own matter, rt_capi_rays.h), and its term is (0, 0, 0) whatever those rays return.
 *   P, N, U, V and the direction D of sample s = i*n + j are EXACTLY rt_capi_ao.h's: P = h.point, N = h.normal negated for
 *       RT_HIT_INSIDE, the tangent frame U, V, the hash g = H(H(seed ^ 0x9e3779b9u) ^ key), the stratum jitter hs, xi1, xi2,
 *       the point (a, b) of the square, its image (dx, dy) on the disc, the lift dz and
 *       D = add(add(scale(U, dx), scale(V, dy)), scale(N, dz)) -- that header's formulae, which are not repeated here.  So
 *       rt_indirect_rays and rt_ambient_occlusion at the same seed, key0 and samples look in the same directions (AO's segment
 *       end Q at radius 1 is T below, bit for bit).
 *   T = add(P, D);  ray s of record i is {P, T}, written at out_rays[6*(i*S + s) .. +5] = {P.x, P.y, P.z, T.x, T.y, T.z}.
 *   colour_s = the colour rt_trace_rays gives that ray at max_depth = gather_depth.
 *   emitters == 0:  hit_s = the record rt_intersect_rays gives the same ray; where hit_s.flags & RT_HIT_LIGHT, colour_s is
 *       replaced by (0, 0, 0).  (The reference shades lights as point lights, which the record's own direct shading has
 *       counted already; a gather ray that meets the visible light sphere would count that light a second time.)
 *   emitters == 1:  nothing is replaced and no query is launched.
 *   mean.c = (((colour_0.c + colour_1.c) + ...) + colour_{S-1}.c) / (float)S        strictly in order of s
 *   kd     = the `diffuse` of objects[h.object] as given to rt_scene_create*; 0.0f if h.object >= n_objects (records the
 *            caller made up)
 *   w.c    = (h.color.c * kd) * gain
 *   term.c = w.c * mean.c                                                            ((0, 0, 0) for a dead record)
 *   out_rgb[3i + c] = base_rgb[3i + c] + term.c;  with base_rgb == NULL it is term.c itself (it is not evaluated as
 *            0 + term, which could flip the sign of a zero).  A dead record's output is therefore base + 0.0f: the base word
 *            for word, except that a base of -0.0 comes out as +0.0; without a base it is +0.0.
 * out_rgb == base_rgb is allowed: each word is read and written by one lane.  Any other overlap of the arguments is the
 * caller's error and is not checked.
 *
 * WHAT FOLLOWS.
 *   - Record i samples with key0 + i: a strip of a W x H frame launched with key0 = x0*H equals the same columns of the whole
 *     frame bit for bit.  chunk_records never changes a bit.
 *   - The directions are cosine-distributed (the disc lift), so mean estimates irradiance / pi and albedo * mean is the
 *     Lambertian bounce with no further weight.  A mirror (diffuse 0) gains nothing.
 *   - A gather ray that misses returns the scene's null_color: an open scene is lit by its sky.
 *   - Only the first hit gathers: what the camera ray sees in a mirror or through glass is not given a bounce of its own
 *     (for mirrors, include/rt_mirror.h gives the records to gather at).
 *   - An inside hit (RT_HIT_INSIDE) gathers inside the sphere that contains it, as AO looks there.
 *
 * SOFT-SHADOW SCENES (rt_scene_create_soft with at least one area light) are refused with RT_ERR_INVALID, for the reason
 * rt_capi_lens.h gives: a ray batch keys its shadow samples by the ray index (rt_capi_soft.h), so the result would change with
 * chunk_records.  Image textures and refraction work unchanged.
 *
 * rt_indirect_rays* are the ray generation alone: no scene, a device index (the conventions of rt_lens_rays).  out_rays holds
 * 6 n S floats.
 *
 * Argument checks, all before any device work, all RT_ERR_INVALID, in this order: (1) the scene is NULL
 * (rt_indirect_diffuse* only); (2) params is NULL; (3) samples outside 1..RT_INDIRECT_MAX_SAMPLES; (4) gather_depth < 0;
 * (5) chunk_records < 0; (6) emitters neither 0 nor 1; (7) gain NaN or infinite; (8) n < 0; (9) hits, then the output, NULL
 * while n > 0; (10) n > 533 333 333 (rt_render_gbuffer's record limit) -- for rt_indirect_rays* in its place: 6 n S floats
 * beyond rt_render's limit of 8e9; (11) for the device calls: d_hits not 16-byte aligned, then the output not 4-byte aligned,
 * then a non-NULL d_base_rgb not 4-byte aligned; (12) last, the scene has area lights.  rt_indirect_rays* then return
 * RT_ERR_NO_DEVICE without a device, or RT_ERR_INVALID for a device index out of range, as rt_lens_rays does.  n == 0 is
 * RT_OK and launches nothing.
 *
 * NO HOST SYNCHRONISATION.  rt_indirect_diffuse_device and rt_indirect_rays_device are enqueued on hip_stream and return;
 * nothing is read back, the launches depend on the arguments alone.  (Scratch that has to grow is reallocated first, which
 * waits for the device as any allocation does; a call that fits the handle's scratch, on the stream of the handle's previous
 * call, waits for nothing.  On another stream it first waits on the host for that previous stream, as every call of a handle
 * does: INTEGRATION.md section 4, "Streams".)
 *
 * SCRATCH lives in the scene handle and only grows: per record of a chunk the rays and their colours, 36 S bytes, and with
 * emitters == 0 the gather rays' records as well, 84 S bytes in all.  chunk_records = 0 is the library's default: the most
 * records whose scratch stays within 256 MiB, and at least one; no chunk_records gives a launch more than 2^31 - 65 rays.  The
 * host variant adds the records, the base and the output of the whole batch.  All offsets are 64-bit.
 *
 * Timing, lock and options are as rt_capi_lens.h says for rt_render_lens: rt_indirect_info's four stage times are HIP-event
 * times on the call's stream, summed over the chunks (query_ms is 0 with emitters == 1); rt_get_timing().last_kernel_ms is
 * their sum for as long as the call is the handle's last launch; launches and sum_kernel_ms count the ray-batch and query
 * launches as for any other call, and rt_get_launch_info() describes the call's last one (a *_hits kernel with emitters == 0,
 * else a *_rays kernel).  The handle's lock is held for the whole call.  Speed-only options (rt_capi_tuning.h) apply as for
 * rt_trace_rays and rt_intersect_rays.
 *
 * Not provided: several GPUs; the counting build; soft-shadow scenes; compaction of dead records (a sky pixel still traces its
 * S degenerate rays: a compacting variant needs a host read-back); gathers at refracted hits (mirrors: include/rt_mirror.h);
 * more than one diffuse bounce beyond what gather_depth gives the gather rays' own direct shading; importance by BRDF.
 *
 * rt_indirect_params is 28 bytes; rt_indirect_info is 56 bytes: records at 0, rays at 8, chunks at 16, raygen_ms at 24,
 * trace_ms at 32, query_ms at 40, resolve_ms at 48.
 */
#ifndef RT_CAPI_INDIRECT_H_
#define RT_CAPI_INDIRECT_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_INDIRECT_VERSION 1
#define RT_INDIRECT_MAX_SAMPLES 8

typedef struct rt_indirect_params {
    int32_t  samples;        /* n, 1..8: n x n gather rays per record                                     */
    int32_t  gather_depth;   /* >= 0: max_depth of the gather rays                                        */
    int32_t  chunk_records;  /* >= 0; most records gathered per launch, 0: library default; never changes */
                             /* a result                                                                  */
    int32_t  emitters;       /* 0: gather rays whose first hit is a light count black; 1: as traced       */
    uint32_t seed;
    uint32_t key0;           /* record i samples with key = key0 + (uint32_t)i (wraps)                    */
    float    gain;           /* finite                                                                    */
} rt_indirect_params;        /* 28 bytes */

typedef struct rt_indirect_info {       /* of the scene's last rt_indirect_diffuse* call */
    int64_t records, rays;              /* records of the batch; gather rays traced (records * S) */
    int32_t chunks;                     /* chunks of records the batch was gathered in */
    double  raygen_ms, trace_ms, query_ms, resolve_ms;   /* HIP events, summed over the chunks; query_ms 0 with emitters 1 */
} rt_indirect_info;                     /* 56 bytes */

int rt_capi_indirect_version(void);

/* the gather rays alone; host memory, synchronous */
int rt_indirect_rays(const rt_indirect_params *params, int n, const rt_hit *hits, int device, float *out_rays);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising; d_hits
 * 48 n bytes, 16-byte aligned; d_out_rays 24 n S bytes, 4-byte aligned */
int rt_indirect_rays_device(const rt_indirect_params *params, int n, const void *d_hits, int device, void *d_out_rays,
                            void *hip_stream);

/* host memory, synchronous: n records in, base_rgb (3 n floats) or NULL, 3 n floats out */
int rt_indirect_diffuse(rt_scene *scene, const rt_indirect_params *params, int n, const rt_hit *hits, const float *base_rgb,
                        float *out_rgb);

/* device memory on the scene's device, enqueued on hip_stream without synchronising (above); params is read before the call
 * returns, the records and the base must stay alive until the stream has drained */
int rt_indirect_diffuse_device(rt_scene *scene, const rt_indirect_params *params, int n, const void *d_hits,
                               const void *d_base_rgb, void *d_out_rgb, void *hip_stream);

/* the last rt_indirect_diffuse* call of the scene (all zero before the first); waits for that call's events */
int rt_get_indirect_info(const rt_scene *scene, rt_indirect_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_INDIRECT_H_ */
