/*
 * rt_mirror.h -- hit records of what a pixel sees in a mirror.  Every stage after the G-buffer (rt_ambient_occlusion,
 * rt_indirect_diffuse, rt_denoise, rt_upsample_guided, rt_temporal_accumulate, rt_motion_accumulate, rt_svgf_filter) works from
 * one rt_hit per pixel, the camera ray's first hit; where that hit is a mirror the record describes the mirror's surface and not
 * what the pixel shows.  This call walks the mirror chain of every ray of a batch on the GPU and returns, per ray: the TERMINAL
 * record (the first hit that is not a followed mirror: AO and the bounce gather there), the path's THROUGHPUT (to weight what
 * was gathered), a GUIDE record (the terminal surface unfolded through the mirrors to where the camera sees it, with an object id
 * that tells the mirror image from the thing itself: the filters and the temporal pass are steered by it) and a PATH word.
 * Plain C99, versioned on its own (RT_MIRROR_VERSION / rt_mirror_version()); rt_capi_query.h, which this header includes for
 * rt_hit, and every other header are unchanged, and no existing call changes a bit.
 *
 * THE DEFINITION, which the GPU meets bit for bit: IEEE fp32, one rounding per operation, no contraction, in the order written.
 * rays and rows are rt_intersect_rays': ray i is {E, T} at rays[6i .. 6i+5].  For ray i the starting state is
 *     ray_0 = the input ray;  d = d0 = normalize(T - E) in createEyeRay's arithmetic (what rt_intersect_rays traces: the three
 *     differences, sqrtf of the left-to-right sum of their squares, three divides);  w = (1, 1, 1);  L = +0.0f;  A = the 3 x 3
 *     identity;  tag = 0;  k = 0.
 * dot(a, b) is (a.x*b.x + a.y*b.y) + a.z*b.z.  H is rt_capi_ao.h's lowbias32.  rf[o] is the `reflective` of object o as given
 * to rt_scene_create*.  Repeat:
 *     h = the record rt_intersect_rays gives ray_k.
 *     If h.object >= 0:  L = L + h.distance.
 *     mirror <=> h.object >= 0 and !(h.flags & RT_HIT_LIGHT) and rf[h.object] >= min_reflective.
 *     If !mirror or k == max_bounces: the terminal record is h, cut = mirror ? 1 : 0, and the loop stops.
 *     Otherwise, with n = h.normal (as it stands in the record, inside hits included) and P = h.point:
 *         c    = dot(n, d)
 *         r.j  = ((-2.0f * n.j) * c) + d.j                     (the reference's CollisionObject expression)
 *         Tn.j = P.j + r.j
 *         ray_{k+1} = {P, Tn}
 *         d    = normalize(Tn - P), the same arithmetic as d0
 *         w.j  = w.j * (rf[h.object] * h.color.j)
 *         an.r = dot(A[r], n), then A[r][j] = A[r][j] - (2.0f * an.r) * n.j          (rows r = 0, 1, 2)
 *         tag  = 1u + H((tag << 12) | (uint32_t)h.object) % 0x7fffeu     (1 .. 0x7fffe, 19 bits; objects take 12: 4 096 a scene)
 *         k    = k + 1
 * The outputs:
 *     out_hits[i]        = the terminal record word for word.
 *     out_weight[3i + j] = w.j
 *     out_path[i]        = k | cut << 8 | tag << 12
 *     out_guide[i]       = the terminal record word for word if its object < 0 or k == 0; otherwise
 *         object   = (int32_t)((tag << 12) | object)
 *         distance = L
 *         point.j  = E.j + d0.j * L
 *         normal.r = dot(A[r], terminal.normal)
 *         color and flags verbatim.
 * out_hits is required; out_guide, out_weight and out_path may each be NULL, and what is given does not depend on which are.
 *
 * WHAT FOLLOWS.
 *   - With max_bounces 0, or no object at or above min_reflective, out_hits is rt_intersect_rays' output, the guide equals it,
 *     the weight is 1 and the path is 0 -- but for the cut bit (0x100), which max_bounces 0 sets where the first hit is a
 *     mirror it was not allowed to follow.
 *   - For planar mirrors the guide's point and normal are the terminal surface reflected back through the mirrors, up to the
 *     planes' 1e-3 point offsets: reprojecting them by an earlier camera finds where the reflected image was.  For a curved
 *     mirror they are a definition, not a geometry.
 *   - The tagged object is >= 0, differs from every true index once a mirror was followed, and differs between chains (up to
 *     hash collisions).  The guide's object MUST NOT be used to index object tables: rt_indirect_diffuse gets out_hits, the
 *     filters and the accumulation get out_guide.  rt_motion_accumulate reads a tagged id as "beyond the table": static.
 *   - The chain is this header's, not calculatePixel's bit for bit.  The reference traces Ray(P, r), whose direction is
 *     normalize(r); a ray batch can only say {P, P + r}, and normalize((P + r) - P) may differ from normalize(r) in the last
 *     bits.  At a silhouette inside a mirror image the terminal object can therefore differ from the one the rendered colour's
 *     recursion met (measured: DESIGN.md section 27).
 *   - A strip or any sub-batch equals the same rays of the whole batch: a ray's result depends on that ray alone.  rows and
 *     chunk_rays never change a bit.
 *   - Soft-shadow, textured and refractive scenes are accepted: a hit query casts no shadow rays.  Glass is not looked
 *     through; a refractive object whose `reflective` qualifies is followed as a mirror.
 *
 * Argument checks, all before any device work, all RT_ERR_INVALID, in this order: (1) the scene is NULL; (2) params is NULL;
 * (3) max_bounces outside 0..RT_MIRROR_MAX_BOUNCES; (4) chunk_rays < 0; (5) min_reflective NaN; (6) n < 0; (7) rows < 1;
 * (8) rays, then out_hits, NULL while n > 0; (9) the batch is beyond rt_trace_rays' limit (rt_capi_rays.h); (10) the device
 * call only: d_rays not 4-byte aligned; then d_out_hits or a non-NULL d_out_guide not 16-byte aligned; then a non-NULL weight or
 * path not 4-byte aligned.  n == 0 is RT_OK and launches nothing.
 *
 * NO HOST SYNCHRONISATION in the device call.  The host cannot know when every chain has ended, so each chunk enqueues
 * max_bounces + 1 hit queries with a step kernel after each; a ray whose chain has ended is given six +0.0f as its next ray, as
 * a dead record's rays are in rt_indirect_diffuse, and its later records are ignored.  Nothing is read back.  (Scratch that has
 * to grow is reallocated first, which waits for the device as any allocation does; and a call on another stream than the
 * handle's previous call first waits on the host for that previous stream, as every call of a handle does: INTEGRATION.md
 * section 4, "Streams".)
 *
 * SCRATCH lives in the scene handle and only grows: per ray of a chunk its record (48 bytes), its next ray (24) and its state
 * (56: w, L, A and a word).  chunk_rays = 0 is the library's default: the most rays whose scratch stays within 256 MiB.  The
 * host variant adds the rays and the outputs of the whole batch.  All offsets are 64-bit.
 *
 * Timing, lock and options are as rt_capi_indirect.h says for rt_indirect_diffuse: rt_mirror_info's two stage times are
 * HIP-event times on the call's stream, summed over the chunks and bounces; rt_get_timing().last_kernel_ms is their sum for as
 * long as the call is the handle's last launch; launches and sum_kernel_ms count the query launches as for any other call, and
 * rt_get_launch_info() describes the call's last one (a *_hits kernel).  The handle's lock is held for the whole call.
 * Speed-only options (rt_capi_tuning.h) apply as for rt_intersect_rays.
 *
 * Not provided: compaction of finished rays (it needs a read-back: rt_mirror_compact.h has it, as calls of its own); glass; more than one terminal per pixel (a half-mirror is
 * either followed or not: that is min_reflective's job); several GPUs; the counting build; a command-line flag.  (Glass has since got
 * a header of its own: rt_glass.h, this chain with the transmitted child as one more way to go on.)
 *
 * Buffers past 2^32 bytes: the device call is tested on 100 000 007 rays (tests/test_mirror_large_gpu.py) -- terminal and guide
 * records of 4.8 GB each, every word compared; the default chunk, whose offsets into the outputs pass 2^32 bytes, and one
 * chunk of 90 000 001 rays, whose records and state planes in the scratch pass 2^32 bytes.  Not tested, because no batch that
 * fits a test's 48 GB of device memory reaches them: out_weight and out_path past 2^32 bytes (n > 357.9 million and n > 2^30);
 * the element index 6 * ray of the rays past 2^32 (n > 715 827 882); the host variant past 2^32 bytes (it stages the batch and
 * runs the device call's code).
 *
 * rt_mirror_params is 12 bytes; rt_mirror_info is 32 bytes: rays at 0, chunks at 8, queries at 12, query_ms at 16, step_ms
 * at 24.
 */
#ifndef RT_MIRROR_H_
#define RT_MIRROR_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_MIRROR_VERSION 1
#define RT_MIRROR_MAX_BOUNCES 64

typedef struct rt_mirror_params {
    int32_t max_bounces;      /* 0..RT_MIRROR_MAX_BOUNCES: the most mirrors followed                       */
    int32_t chunk_rays;       /* >= 0; most rays walked per launch, 0: library default; never changes a    */
                              /* result                                                                    */
    float   min_reflective;   /* a hit is followed when its object's `reflective` >= this; not NaN         */
} rt_mirror_params;           /* 12 bytes */

typedef struct rt_mirror_info {         /* of the scene's last rt_mirror_records* call */
    int64_t rays;                       /* rays of the batch */
    int32_t chunks;                     /* chunks of rays the batch was walked in */
    int32_t queries;                    /* hit queries launched: chunks * (max_bounces + 1) */
    double  query_ms, step_ms;          /* HIP events, summed over the chunks and bounces */
} rt_mirror_info;                       /* 32 bytes */

int rt_mirror_version(void);

/* host memory, synchronous: n rays in; n records, n records, 3 n floats and n words out, the last three each or NULL */
int rt_mirror_records(rt_scene *scene, const rt_mirror_params *params, int n, int rows, const float *rays, rt_hit *out_hits,
                      rt_hit *out_guide, float *out_weight, uint32_t *out_path);

/* device memory on the scene's device, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising
 * (above); params is read before the call returns, the rays must stay alive until the stream has drained */
int rt_mirror_records_device(rt_scene *scene, const rt_mirror_params *params, int n, int rows, const void *d_rays,
                             void *d_out_hits, void *d_out_guide, void *d_out_weight, void *d_out_path, void *hip_stream);

/* the last rt_mirror_records* call of the scene (all zero before the first); waits for that call's events */
int rt_get_mirror_info(const rt_scene *scene, rt_mirror_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RT_MIRROR_H_ */
