/*
 * rt_paths_compact.h -- rt_indirect_paths over the paths still alive.  rt_indirect_paths (rt_paths.h) never waits for the device,
 * so it cannot know which paths have ended: it traces and queries ALL records * S rays of a chunk at every one of its B bounces,
 * and an ended path is traced again as a ray of six zeros each time.  The calls of this header read back, after each bounce, how
 * many paths go on, keep those paths' rays in a dense list in path order, and trace and query that list alone: the ray batches
 * cover records * S + sum(alive[b >= 1]) rays instead of records * S * B, and a chunk stops at the first bounce that leaves no
 * path alive.  Plain C99, versioned on its own (RT_PATHS_COMPACT_VERSION / rt_paths_compact_version()); rt_paths.h, which this
 * header includes for its params, rt_hit and RT_PATHS_MAX_BOUNCES, and every other header are unchanged, and no existing call
 * changes a bit.
 *
 * THE DEFINITION: this header adds none.  Every word of out_rgb is rt_indirect_paths' for the same arguments, bit for bit: for
 * every bounces, samples, emitters, gain, key0, chunk_records, base (NULL, out of place, in place: out_rgb == base_rgb) and
 * strip.  alive[] equals rt_paths_info.alive[] of that call.
 *
 * Argument checks: rt_paths.h's (1) .. (12), in its order, with its messages, all before any device work and all
 * RT_ERR_INVALID.  n == 0 is RT_OK and launches nothing.
 *
 * SYNCHRONISATION -- the one difference.  Per chunk the call makes one ray generation, exactly rt_indirect_paths'.  Bounce 0
 * goes over all m * S rays of the chunk, the dead records' rays of six zeros included: nothing is known before the first trace.
 * For every bounce b < B-1 the call enqueues the ray batch, the hit query, a pass that counts the paths that go on, a scan of
 * the counts and the step; then it WAITS FOR ITS STREAM, once, and reads the 4-byte total through pinned host memory: at most
 * B-1 waits a chunk, fewer when the chunk's paths end sooner.  Bounce b >= 1 traces and queries exactly the chunk's alive[b]
 * rays as a flat list (rows = their number), in path order: the list, the launches and the times' meaning are the same from run
 * to run.  A chunk stops at the first bounce that leaves no path alive; the resolve follows.  With bounces == 1 there is no
 * count, no list and no wait: only the chunk size may then differ from rt_indirect_paths_device.
 *     The stream must therefore not be capturing: the call refuses one that is with RT_ERR_INVALID, before any device work (it
 * cannot be recorded into a graph; rt_indirect_paths_device can), and work the caller enqueued on the stream before the call is
 * waited for as well.  The device call returns with its last step and its resolve possibly still running: out_rgb is valid once
 * the stream has drained.  The waits cost host time that the five stage times do not show; choose rt_indirect_paths where the
 * call must stay asynchronous or be captured, or where nearly every path runs all B bounces.
 *
 * COUNTS.  Bounces run, per chunk: 1 + |{b in 1 .. B-1 : the chunk's alive[b] > 0}|.  traces is the sum of the bounces run over
 * the chunks; queries the same sum, minus one for every chunk that ran bounce B-1 with emitters == 1 (the one place a query is
 * not needed); syncs, per chunk, the bounces run, minus 1 if the chunk ran all B bounces; rays the rays actually traced:
 * records * S plus the sum of alive[b] over b >= 1 -- never records * S * B.  alive[0] is counted on the device, as
 * rt_indirect_paths counts it; alive[b >= 1] are the totals the host read, summed over the chunks.
 *
 * SCRATCH lives in the scene handle, apart from rt_indirect_paths', and only grows.  Per path of a chunk 140 bytes: two lists
 * -- the one a bounce reads and the one it writes -- of a ray (24) and the path's slot in the chunk (4) each; the ray's colour
 * (12) and the ray's record (48), both dense, one per list entry; the path's throughput T (12) and its sum acc (12), both at the
 * path's SLOT; and 8 bytes per 256 paths of counts and their scan: reckoned together as 141 bytes a path, and 16 KiB of
 * alive[0]'s partial counters.  With bounces == 1 the second list and the slots are not grown.  chunk_records = 0 is the
 * library's default: the most records whose scratch stays within 256 MiB, and at least one (rt_indirect_paths' default chunk is
 * larger: 108 bytes a path); no chunk_records gives a launch more than 2^31 - 65 rays.  The host variant adds the records, the
 * base and the output of the whole batch.  All offsets are 64-bit.
 *
 * rt_get_paths_compact_info describes the scene's last call of THIS header (all zero before the first) and waits for that
 * call's events; rt_get_paths_info is not touched by these calls, nor this one by rt_indirect_paths*.  The five stage times are
 * HIP-event times on the call's stream, summed over the chunks and bounces: step_ms covers the count, scan and step kernels;
 * the time the device stands idle while the host reads a total is in no stage.  rt_get_timing().last_kernel_ms is their sum for
 * as long as the call is the handle's last launch.  The handle's lock is held for the whole call.  Speed-only options
 * (rt_capi_tuning.h) apply as for rt_trace_rays and rt_intersect_rays.
 *
 * Not provided: compaction before bounce 0 (dead records, an open scene's sky: it needs a wait before the first trace);
 * compaction across chunks; a graph-capturable form; Russian roulette and importance by BRDF; several GPUs; the counting build;
 * soft-shadow scenes (refused, rt_paths.h's check (12)); buffers past 2^32 bytes (untested, as for rt_paths.h).
 *
 * rt_paths_compact_info is 136 bytes: records at 0, rays at 8, chunks at 16, traces at 20, queries at 24, syncs at 28,
 * raygen_ms at 32, trace_ms at 40, query_ms at 48, step_ms at 56, resolve_ms at 64, alive at 72 (rt_paths_compact.hip asserts
 * the layout).
 */
#ifndef RT_PATHS_COMPACT_H_
#define RT_PATHS_COMPACT_H_

#include "rt_paths.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_PATHS_COMPACT_VERSION 1

typedef struct rt_paths_compact_info {  /* of the scene's last rt_indirect_paths_compact* call */
    int64_t records, rays;              /* records of the batch; rays traced: records * S + the sum of alive[b >= 1] */
    int32_t chunks;                     /* chunks of records the batch was gathered in */
    int32_t traces;                     /* ray batches launched: the bounces run, summed over the chunks */
    int32_t queries;                    /* hit queries launched */
    int32_t syncs;                      /* stream waits made */
    double  raygen_ms, trace_ms, query_ms, step_ms, resolve_ms;   /* HIP events, summed over the chunks and bounces */
    int64_t alive[RT_PATHS_MAX_BOUNCES];                          /* paths alive at bounce b; 0 for b >= bounces */
} rt_paths_compact_info;                /* 136 bytes */

int rt_paths_compact_version(void);

/* host memory, synchronous: rt_indirect_paths' arguments and output */
int rt_indirect_paths_compact(rt_scene *scene, const rt_paths_params *params, int n, const rt_hit *hits, const float *base_rgb,
                              float *out_rgb);

/* device memory on the scene's device, on hip_stream (a hipStream_t; NULL = the null stream), which the call waits for (above)
 * and which must not be capturing; d_hits 48 n bytes, 16-byte aligned; the records and the base must stay alive, and the output
 * is valid, once the stream has drained */
int rt_indirect_paths_compact_device(rt_scene *scene, const rt_paths_params *params, int n, const void *d_hits,
                                     const void *d_base_rgb, void *d_out_rgb, void *hip_stream);

/* the last rt_indirect_paths_compact* call of the scene (all zero before the first); waits for that call's events */
int rt_get_paths_compact_info(const rt_scene *scene, rt_paths_compact_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RT_PATHS_COMPACT_H_ */
