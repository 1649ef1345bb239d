/*
 * rt_glass_compact.h -- rt_glass_records over the rays still alive.  rt_glass_records (rt_glass.h) never waits for the device, so
 * it cannot know which chains have ended: it asks max_bounces + 1 hit queries of ALL the rays of a chunk, and a finished ray is
 * queried again as six zeros on every later bounce.  Behind glass most chains are short -- the glass room's pixel rays at 61 x 37
 * have 2257, 1223, 454, 124, 81, 31, 22, 20, 12 rays alive at query 0 .. 8 -- and the queries are most of the call's time.  The
 * calls of this header are to rt_glass_records what rt_mirror_compact.h's are to rt_mirror_records: after each bounce they read
 * back how many chains go on, keep those rays in a dense list in ray order, and query that list alone.  Plain C99, versioned on
 * its own (RT_GLASS_COMPACT_VERSION / rt_glass_compact_version()); rt_glass.h, which this header includes for its structs and
 * rt_hit, and every other header are unchanged, and no existing call changes a bit.
 *
 * THE DEFINITION: this header adds none.  Every output word is rt_glass_records' for the same arguments, bit for bit: for every
 * max_bounces, min_reflective, min_transmissive, chunk_rays, rows and strip, for every combination of NULL optional outputs.
 * Each output word is written exactly once, by the step that ends its ray.  With min_transmissive = +INFINITY, or on a scene
 * without refractive objects, the words are rt_mirror_records_compact's as well, and so are the info's alive[], rays_queried,
 * queries, syncs and chunks.
 *
 * Argument checks: rt_glass.h's (1) .. (10), in its order, with its messages, all before any device work and all
 * RT_ERR_INVALID; after them the device call refuses a capturing stream (below).  n == 0 is RT_OK and launches nothing.
 *
 * SYNCHRONISATION -- the one difference.  Per chunk and bounce the call enqueues the hit query of the live rays, a pass that
 * counts the chains that go on, and the step; whenever another bounce could follow (every bounce but max_bounces) it then
 * WAITS FOR ITS STREAM, once, and reads the 4-byte count through pinned host memory: at most max_bounces waits a chunk, fewer
 * when the chunk's chains end sooner.  The stream must therefore not be capturing (the call refuses one that is, RT_ERR_INVALID:
 * it cannot be recorded into a graph), and work the caller enqueued on the stream before the call is waited for as well.  The
 * device call returns with its last step possibly still running: the outputs are valid once the stream has drained.  The wait
 * costs host time that the two stage times below do not show; choose rt_glass_records where the call must stay asynchronous or
 * be captured, or where nearly every chain runs to max_bounces.
 *
 * WHETHER A CHAIN GOES ON is rt_glass.h's `follow` (steps 3 to 8), which depends on the transmitted child's geometry: the
 * counting pass evaluates it from the entry's record, its ray and its object's 48 table bytes before the step does, by the same
 * function, so the places the step writes are those that were counted.  A hit that is no candidate costs the pass two words of
 * its record and at most two table words.
 *
 * EARLY END.  A chunk stops at the first bounce after which no ray is alive.  Per chunk: queries = the number of
 * b <= max_bounces for which the chunk has a live ray; syncs = that number, minus 1 if the chunk ran all max_bounces + 1
 * queries.  The query of bounce 0 is over the caller's rays with the caller's rows; that of bounce b >= 1 is over exactly the
 * chunk's alive[b] rays as a flat list (rows = their number), in ray order.
 *
 * SCRATCH lives in the scene handle, apart from every other call's, and only grows: per ray of a chunk its record (48 bytes),
 * two lists -- the one a bounce reads and the one it writes -- of a next ray (24), a state (56 with out_guide: w, L, A and a
 * word, which carries g; else 16) and the ray's index in the chunk (4) each, and 8 bytes per 256 rays of counts: 216 bytes a ray
 * and the counts, reckoned as 217 -- rt_mirror_compact.h's figure.  chunk_rays = 0 is the library's default: the most rays whose
 * scratch stays within 256 MiB, 1 237 029.  The host variant adds the rays and the outputs of the whole batch.  All offsets are
 * 64-bit.
 *
 * rt_get_glass_compact_info describes the scene's last call of THIS header (all zero before the first) and waits for that
 * call's events; rt_get_glass_info and rt_get_mirror_compact_info are not touched by these calls, nor this one by theirs.
 * alive[b] is the number of rays whose chain reached query b, summed over the chunks: |{i : (out_path[i] & 0xff) >= b}|, 0
 * beyond max_bounces; rays_queried is their sum.  query_ms and step_ms are HIP-event times on the call's stream, summed over the
 * chunks and bounces: the queries, and the count, scan and step kernels; the time the device stands idle while the host reads a
 * count is in neither.  rt_get_timing() and rt_get_launch_info() behave as rt_mirror.h says for rt_mirror_records, with these two
 * times.  The handle's lock is held for the whole call.  Speed-only options (rt_capi_tuning.h) apply as for rt_intersect_rays.
 *
 * Not provided: a graph-capturable form; compaction across chunks; several GPUs; the counting build; a command-line flag.
 *
 * Buffers past 2^32 bytes: every offset is 64-bit.  Tested (tests/test_glass_compact_large_gpu.py, the device call, 100 000 007
 * rays): records and guide records past 2^32 bytes and rays past 2^31, with the default chunk and with one chunk of 90 000 001
 * rays, whose records and state planes pass 2^32 bytes themselves; a dense list of 62.3 million entries; and a dense list of
 * 90 000 001 entries, whose own records pass 2^32 bytes and whose rays 2^31.  NOT tested: weights past 2^32 bytes (n > 357.9
 * million), path words past 2^32 bytes (n > 2^30), the rays' element index 6 * ray past 2^32, lists of more than 2^28 entries
 * through the call, and the host variant at any of these sizes.
 *
 * rt_glass_compact_info is 568 bytes: rays at 0, rays_queried at 8, chunks at 16, queries at 20, syncs at 24, reserved at 28,
 * query_ms at 32, step_ms at 40, alive at 48 -- rt_mirror_compact_info's fields and layout.
 */
#ifndef RT_GLASS_COMPACT_H_
#define RT_GLASS_COMPACT_H_

#include "rt_glass.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_GLASS_COMPACT_VERSION 1

typedef struct rt_glass_compact_info {              /* of the scene's last rt_glass_records_compact* call */
    int64_t rays;                                   /* rays of the batch */
    int64_t rays_queried;                           /* the sum of alive[]: rays the hit queries were asked */
    int32_t chunks;                                 /* chunks of rays the batch was walked in */
    int32_t queries;                                /* hit queries actually launched */
    int32_t syncs;                                  /* stream waits made */
    int32_t reserved;                               /* 0 */
    double  query_ms, step_ms;                      /* HIP events, summed over the chunks and bounces */
    int64_t alive[RT_MIRROR_MAX_BOUNCES + 1];       /* rays whose chain reached query b, summed over the chunks */
} rt_glass_compact_info;                            /* 568 bytes */

int rt_glass_compact_version(void);

/* host memory, synchronous: rt_glass_records' arguments and outputs */
int rt_glass_records_compact(rt_scene *scene, const rt_glass_params *params, int n, int rows, const float *rays,
                             rt_hit *out_hits, rt_hit *out_guide, float *out_weight, uint32_t *out_path);

/* device memory on the scene's device, on hip_stream (a hipStream_t; NULL = the null stream), which the call waits for (above)
 * and which must not be capturing; the rays must stay alive, and the outputs are valid, once the stream has drained */
int rt_glass_records_compact_device(rt_scene *scene, const rt_glass_params *params, int n, int rows, const void *d_rays,
                                    void *d_out_hits, void *d_out_guide, void *d_out_weight, void *d_out_path,
                                    void *hip_stream);

/* the last rt_glass_records_compact* call of the scene (all zero before the first); waits for that call's events */
int rt_get_glass_compact_info(const rt_scene *scene, rt_glass_compact_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RT_GLASS_COMPACT_H_ */
