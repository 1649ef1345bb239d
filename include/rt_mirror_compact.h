/*
 * rt_mirror_compact.h -- rt_mirror_records over the rays still alive.  rt_mirror_records (rt_mirror.h) never waits for the
 * device, so it cannot know which chains have ended: it asks max_bounces + 1 hit queries of ALL the rays of a chunk, and a
 * finished ray is queried again as six zeros on every later bounce.  The calls of this header read back, after each bounce, how
 * many chains go on, keep those rays in a dense list in ray order, and query that list alone: the queries cover
 * sum(alive[b]) rays instead of (max_bounces + 1) n, and a chunk stops at the first bounce that leaves no ray alive.  Plain
 * C99, versioned on its own (RT_MIRROR_COMPACT_VERSION / rt_mirror_compact_version()); rt_mirror.h, which this header includes
 * for its structs and rt_hit, and every other header are unchanged, and no existing call changes a bit.
 *
 * THE DEFINITION: this header adds none.  Every output word is rt_mirror_records' for the same arguments, bit for bit: for every
 * max_bounces, min_reflective, chunk_rays, rows and strip, for every combination of NULL optional outputs, for misses, E == T
 * rays and lights.  Each output word is written exactly once, by the step that ends its ray.
 *
 * Argument checks: rt_mirror.h's (1) .. (10), in its order, with its messages, all before any device work and all
 * RT_ERR_INVALID.  n == 0 is RT_OK and launches nothing.
 *
 * SYNCHRONISATION -- the one difference.  Per chunk and bounce the call enqueues the hit query of the live rays, a pass that
 * counts the chains that go on, and the step; whenever another bounce could follow (every bounce but max_bounces) it then
 * WAITS FOR ITS STREAM, once, and reads the 4-byte count through pinned host memory: at most max_bounces waits a chunk, fewer
 * when the chunk's chains end sooner.  The stream must therefore not be capturing (the call refuses one that is, RT_ERR_INVALID:
 * it cannot be recorded into a graph), and work the caller enqueued on the stream before the call is waited for as well.  The
 * device call returns with its last step possibly still running: the outputs are valid once the stream has drained.  The wait
 * costs host time that the two stage times below do not show; choose rt_mirror_records where the call must stay asynchronous
 * or be captured, or where nearly every chain runs to max_bounces.
 *
 * EARLY END.  A chunk stops at the first bounce after which no ray is alive.  Per chunk: queries = the number of
 * b <= max_bounces for which the chunk has a live ray; syncs = that number, minus 1 if the chunk ran all max_bounces + 1
 * queries.  The query of bounce 0 is over the caller's rays with the caller's rows; that of bounce b >= 1 is over exactly the
 * chunk's alive[b] rays as a flat list (rows = their number), in ray order: neighbouring pixels' rays stay neighbours, and
 * the list, the launches and the times' meaning are the same from run to run.
 *
 * SCRATCH lives in the scene handle, apart from rt_mirror_records', and only grows: per ray of a chunk its record (48 bytes),
 * two lists -- the one a bounce reads and the one it writes -- of a next ray (24), a state (56 with out_guide: w, L, A and a
 * word; else 16) and the ray's index in the chunk (4) each, and 8 bytes per 256 rays of counts: 216 bytes a ray and the counts,
 * reckoned as 217.  chunk_rays = 0 is the library's default: the most rays whose scratch stays within 256 MiB, 1 237 029.  The
 * host variant adds the rays and the outputs of the whole batch.  All offsets are 64-bit.
 *
 * rt_get_mirror_compact_info describes the scene's last call of THIS header (all zero before the first) and waits for that
 * call's events; rt_get_mirror_info is not touched by these calls, nor this one by rt_mirror_records*.  alive[b] is the number
 * of rays whose chain reached query b, summed over the chunks: |{i : (out_path[i] & 0xff) >= b}|, 0 beyond max_bounces;
 * rays_queried is their sum.  query_ms and step_ms are HIP-event times on the call's stream, summed over the chunks and
 * bounces: the queries, and the count, scan and step kernels; the time the device stands idle while the host reads a count is in
 * neither.  rt_get_timing() and rt_get_launch_info() behave as rt_mirror.h says for rt_mirror_records, with these two times.
 * The handle's lock is held for the whole call.  Speed-only options (rt_capi_tuning.h) apply as for rt_intersect_rays.
 *
 * Not provided: a graph-capturable form; compaction across chunks; several GPUs; the counting build; a command-line flag.
 * Glass is rt_glass_compact.h's rt_glass_records_compact, the same loop over rt_glass.h's chains.
 *
 * Buffers past 2^32 bytes: the device call is tested on 100 000 007 rays (tests/test_mirror_large_gpu.py), every output word
 * and the info's counts compared: with the default chunk, and with one chunk of 90 000 001 rays -- 19.5 GB of scratch, lists
 * of 43.9 million entries whose ray indices address output bytes past 2^32 -- with and without out_guide and out_weight.  The
 * scan is tested on its own up to 2^21 + 1537 counts, three trips of its second level (tests/test_mirror_compact_gpu.py).  Not
 * tested, because no batch that fits a test's 48 GB of device memory reaches them: a list of more than 2^28 entries through
 * the call (a chunk of 56 GB with its rays and records; the scan alone is covered); out_weight and out_path past 2^32 bytes
 * (n > 357.9 million and n > 2^30); the element index 6 * ray of the rays past 2^32 (n > 715 827 882); the host variant past
 * 2^32 bytes (it stages the batch and runs the device call's code).
 *
 * rt_mirror_compact_info is 568 bytes: rays at 0, rays_queried at 8, chunks at 16, queries at 20, syncs at 24, reserved at 28,
 * query_ms at 32, step_ms at 40, alive at 48.
 */
#ifndef RT_MIRROR_COMPACT_H_
#define RT_MIRROR_COMPACT_H_

#include "rt_mirror.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_MIRROR_COMPACT_VERSION 1

typedef struct rt_mirror_compact_info {             /* of the scene's last rt_mirror_records_compact* call */
    int64_t rays;                                   /* rays of the batch */
    int64_t rays_queried;                           /* the sum of alive[]: rays the hit queries were asked */
    int32_t chunks;                                 /* chunks of rays the batch was walked in */
    int32_t queries;                                /* hit queries actually launched */
    int32_t syncs;                                  /* stream waits made */
    int32_t reserved;                               /* 0 */
    double  query_ms, step_ms;                      /* HIP events, summed over the chunks and bounces */
    int64_t alive[RT_MIRROR_MAX_BOUNCES + 1];       /* rays whose chain reached query b, summed over the chunks */
} rt_mirror_compact_info;                           /* 568 bytes */

int rt_mirror_compact_version(void);

/* host memory, synchronous: rt_mirror_records' arguments and outputs */
int rt_mirror_records_compact(rt_scene *scene, const rt_mirror_params *params, int n, int rows, const float *rays,
                              rt_hit *out_hits, rt_hit *out_guide, float *out_weight, uint32_t *out_path);

/* device memory on the scene's device, on hip_stream (a hipStream_t; NULL = the null stream), which the call waits for (above)
 * and which must not be capturing; the rays must stay alive, and the outputs are valid, once the stream has drained */
int rt_mirror_records_compact_device(rt_scene *scene, const rt_mirror_params *params, int n, int rows, const void *d_rays,
                                     void *d_out_hits, void *d_out_guide, void *d_out_weight, void *d_out_path,
                                     void *hip_stream);

/* the last rt_mirror_records_compact* call of the scene (all zero before the first); waits for that call's events */
int rt_get_mirror_compact_info(const rt_scene *scene, rt_mirror_compact_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RT_MIRROR_COMPACT_H_ */
