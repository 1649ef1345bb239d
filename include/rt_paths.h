/*
 * rt_paths.h -- diffuse light paths of more than one bounce from hit records: rt_indirect_diffuse (rt_capi_indirect.h) ends
 * every gather path at its first hit; rt_indirect_paths follows each of a record's n x n gather rays for up to B bounces, one
 * new cosine-distributed direction at every diffuse hit, and adds what every bounce's ray brings in, weighted by the surfaces
 * the path has left.  The records, the paths' state and every ray stay on the GPU; each bounce is one ray batch
 * (rt_capi_rays.h), one hit query (rt_capi_query.h) and one step kernel over all paths of a chunk; nothing but the result
 * crosses the bus.  Plain C99, versioned on its own (RT_PATHS_VERSION / rt_paths_version()); rt_capi_indirect.h, which this
 * header includes for rt_hit and the first seven parameters' meaning, and every other header are unchanged, and no existing
 * call changes a bit.
 *
 * THE DEFINITION, which the GPU meets bit for bit.  All arithmetic is IEEE fp32, one rounding per operation, no contraction.
 * For record h = hits[i], with n = samples, S = n*n, B = bounces, sample s, path q = i*S + s and the path's key
 * kq = (key0 + (uint32_t)i)*S + s (wrapping in uint32):
 *
 *   Bounce 0.  ray_0 is EXACTLY rt_indirect_rays' ray s of record i: the same seed, the same key key0 + i.  A dead record
 *       (rt_capi_indirect.h: a miss or a light) has rays of six +0.0f and the term (0, 0, 0).  T_0 = (1, 1, 1).  The path is
 *       alive exactly when the record is live.
 *   For b = 0 .. B-1, while the path is alive:
 *       colour_b = the colour rt_trace_rays gives ray_b at max_depth = gather_depth;
 *       g_b      = the record rt_intersect_rays gives ray_b;
 *       emitters == 0:  where g_b.flags & RT_HIT_LIGHT, colour_b is replaced by (0, 0, 0) -- at every bounce;
 *       acc = colour_0 at b = 0, else acc.c = acc.c + T_b.c * colour_b.c;
 *       if b == B-1, stop;
 *       w.c = (g_b.color.c * kd(g_b.object)) * gain  (kd as in rt_capi_indirect.h: 0.0f for an object the scene does not
 *           have),  T_{b+1}.c = T_b.c * w.c;
 *       the path ENDS if g_b is a miss (object < 0) or a light, or if all three channels of T_{b+1} compare equal to 0: its
 *           later rays are six +0.0f and acc is not touched again;
 *       otherwise ray_{b+1} is rt_indirect_rays' single ray (samples = 1) of the record g_b with the seed
 *           seed + (b+1) * 0x9e3779b9u (wrapping) and the key kq -- rt_capi_ao.h's arithmetic for n = 1, s = 0, the frame made
 *           from g_b's normal, negated for RT_HIT_INSIDE; that header's formulae are not repeated here.
 *   Resolve.  mean.c = (((acc_0.c + acc_1.c) + ...) + acc_{S-1}.c) / (float)S over the record's S paths, strictly in order of
 *       s;  out_rgb[3i + c] = base_rgb[3i + c] + ((h.color.c * kd) * gain) * mean.c.  The dead-record rule, the NULL-base rule
 *       and the in-place rule (out_rgb == base_rgb) are exactly rt_indirect_diffuse's.
 *
 * WHAT FOLLOWS.
 *   - With bounces == 1 every word is rt_indirect_diffuse's.
 *   - Strips (key0 = x0*H) and chunk_records never change a bit: a path's key depends on its record's key and its sample alone.
 *   - With gain >= 0 (and colours and coefficients that are not negative) the term never falls as B grows: every bounce adds
 *     T * colour >= 0 to acc, and fp32 addition and the in-order sum are monotonic.
 *   - The zero-throughput stop changes no output word -- a path whose T is (0, 0, 0) adds T * colour = 0 from then on; on
 *     the oracle's frames both rules gave equal words, with gain -0.75 as well -- but it changes alive[]: on the two-mirror
 *     frame 798 paths reach bounce 1 with it and 1703 without.  alive[] is what tells the rule apart.
 *   - A path that has ended is still traced as a degenerate ray at every later bounce (no compaction: that needs a host
 *     read-back); what the ray returns is not read.
 *
 * alive[b] is the number of paths alive at bounce b (b < B, the rest 0), summed over the chunks, counted on the device;
 * alive[0] = S times the live records.  rt_get_paths_info reads the counts after waiting for the call's events.
 *
 * SOFT-SHADOW SCENES are refused with RT_ERR_INVALID, for rt_capi_indirect.h's reason.  Image textures and refraction work
 * unchanged.
 *
 * Argument checks, all before any device work, all RT_ERR_INVALID, in rt_indirect_diffuse's order: (1) the scene is NULL;
 * (2) params is NULL; (3) samples outside 1..RT_INDIRECT_MAX_SAMPLES; (3b) bounces outside 1..RT_PATHS_MAX_BOUNCES;
 * (4) gather_depth < 0; (5) chunk_records < 0; (6) emitters neither 0 nor 1; (7) gain NaN or infinite; (8) n < 0; (9) hits,
 * then the output, NULL while n > 0; (10) n > 533 333 333; (11) for the device call: d_hits not 16-byte aligned, then the
 * output not 4-byte aligned, then a non-NULL d_base_rgb not 4-byte aligned; (12) last, the scene has area lights.  n == 0 is
 * RT_OK and launches nothing.
 *
 * NO HOST SYNCHRONISATION.  rt_indirect_paths_device is enqueued on hip_stream and returns; nothing is read back, the launches
 * depend on the arguments alone: per chunk one ray generation, per bounce a ray batch, a hit query (left out at the last
 * bounce with emitters == 1, the one place it is not needed) and a step, and one resolve.  Scratch that has to grow is
 * reallocated first, and a change of stream waits for the handle's previous stream, as for every call of a handle
 * ("Streams").
 *
 * SCRATCH lives in the scene handle and only grows: 108 bytes a path -- its ray 24, the ray's colour 12, the ray's record 48,
 * T 12, acc 12 -- and 128 KiB of counters (alive[] is counted in 128 partial counts a bounce, a cache line each).
 * chunk_records = 0 is the library's default: the most records whose scratch stays within 256 MiB, and at least one; no
 * chunk_records gives a launch more than 2^31 - 65 rays.  The host variant adds the records, the base and the output of the
 * whole batch.  All offsets are 64-bit.
 *
 * Timing, lock and options are as rt_capi_indirect.h says: the five stage times are HIP-event times on the call's stream,
 * summed over the chunks and bounces (step_ms: the step kernels; resolve_ms: the resolve); rt_get_timing().last_kernel_ms is
 * their sum for as long as the call is the handle's last launch.  The handle's lock is held for the whole call.
 *
 * Not provided: compaction of finished paths (a host read-back; a later call of its own, as rt_mirror_compact.h was for the
 * mirror unit); Russian roulette and importance by BRDF; several GPUs; the counting build; soft-shadow scenes; graph capture
 * (not claimed, not tested); buffers past 2^32 bytes (untested).
 *
 * rt_paths_params is 32 bytes: samples at 0, gather_depth at 4, chunk_records at 8, emitters at 12, seed at 16, key0 at 20,
 * gain at 24, bounces at 28 -- rt_indirect_params' seven fields in their order, then bounces.  rt_paths_info is 128 bytes:
 * records at 0, rays at 8, chunks at 16, raygen_ms at 24, trace_ms at 32, query_ms at 40, step_ms at 48, resolve_ms at 56,
 * alive at 64 (rt_paths.hip asserts both layouts).
 */
#ifndef RT_PATHS_H_
#define RT_PATHS_H_

#include "rt_capi_indirect.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_PATHS_VERSION 1
#define RT_PATHS_MAX_BOUNCES 8

typedef struct rt_paths_params {
    int32_t  samples;        /* n, 1..8: n x n paths per record                                            */
    int32_t  gather_depth;   /* >= 0: max_depth of every bounce's rays                                     */
    int32_t  chunk_records;  /* >= 0; most records gathered per launch, 0: library default; never changes  */
                             /* a result                                                                   */
    int32_t  emitters;       /* 0: a ray whose first hit is a light counts black, at every bounce; 1: as   */
                             /* traced                                                                     */
    uint32_t seed;           /* bounce b draws with seed + b * 0x9e3779b9u (wraps)                         */
    uint32_t key0;           /* record i samples with key0 + (uint32_t)i, its path s with (that) * S + s   */
    float    gain;           /* finite                                                                     */
    int32_t  bounces;        /* B, 1..8: rays a path traces at most                                        */
} rt_paths_params;           /* 32 bytes */

typedef struct rt_paths_info {          /* of the scene's last rt_indirect_paths* call */
    int64_t records, rays;              /* records of the batch; rays traced (records * S * B) */
    int32_t chunks;                     /* chunks of records the batch was gathered in */
    double  raygen_ms, trace_ms, query_ms, step_ms, resolve_ms;   /* HIP events, summed over the chunks and bounces */
    int64_t alive[RT_PATHS_MAX_BOUNCES];                          /* paths alive at bounce b; 0 for b >= bounces */
} rt_paths_info;                        /* 128 bytes */

int rt_paths_version(void);

/* host memory, synchronous: n records in, base_rgb (3 n floats) or NULL, 3 n floats out */
int rt_indirect_paths(rt_scene *scene, const rt_paths_params *params, int n, const rt_hit *hits, const float *base_rgb,
                      float *out_rgb);

/* device memory on the scene's device, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising
 * (above); d_hits 48 n bytes, 16-byte aligned; params is read before the call returns, the records and the base must stay
 * alive until the stream has drained */
int rt_indirect_paths_device(rt_scene *scene, const rt_paths_params *params, int n, const void *d_hits, const void *d_base_rgb,
                             void *d_out_rgb, void *hip_stream);

/* the last rt_indirect_paths* call of the scene (all zero before the first); waits for that call's events */
int rt_get_paths_info(const rt_scene *scene, rt_paths_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RT_PATHS_H_ */
