/*
 * rt_glass.h -- hit records of what a pixel sees through glass.  rt_mirror.h gave every stage after the G-buffer the record of
 * what a pixel shows where its first hit is a mirror; on a scene made by rt_scene_create_refractive (rt_capi_refract.h) the same
 * defect remains behind a window or a glass ball: AO and the bounce are gathered on the pane, the filters see one flat object,
 * and under a moving camera the history reprojects the pane's plane and not the room behind it.  This call is rt_mirror_records
 * with one more way for a chain to go on: through a transmissive object, along the transmitted child rt_capi_refract.h defines.
 * Its outputs are rt_mirror.h's -- TERMINAL record, THROUGHPUT, GUIDE record, PATH word -- and are used the same way.
 * Plain C99, versioned on its own (RT_GLASS_VERSION / rt_glass_version()); it includes rt_mirror.h alone, and no existing call
 * changes a bit.
 *
 * THE DEFINITION, which the GPU meets bit for bit: IEEE fp32, one rounding per operation, no contraction, in the order written.
 * It is rt_mirror.h's chain; what is not said here is said there.  The state is rt_mirror.h's (ray_k = {E_k, T_k}, d, w, L, A,
 * tag, k) and a bit g = 0.  tf[o] and ior[o] are object o's rt_refraction_desc (tf = 0 where it has none); centre_o is a
 * sphere's origin; normal_o and reverse_normal_o are a plane's two stored normals as given to rt_scene_create* (what the render
 * kernels' refraction path reads).  dot and normalize are rt_mirror.h's.  Repeat:
 *      1. h = the record rt_intersect_rays gives ray_k.
 *      2. If h.object >= 0:  L = L + h.distance.
 *      3. eligible  <=> h.object >= 0 and !(h.flags & RT_HIT_LIGHT).                       o = h.object from here on
 *      4. candidate <=> eligible and tf[o] > 0 and tf[o] >= min_transmissive.
 *      5. The transmitted child {O, D} of a candidate is rt_capi_refract.h's:
 *         Sphere.  t = h.distance, P = h.point, Q = P - centre_o, N = normalize(Q), eta = 1.0f / ior[o]; c1, k1, T1, s, P2, N2,
 *             c2, k2, T2 by that header's expressions in that header's order;  O = P2 + N2 * 1e-3f,  D = normalize(T2);
 *             exists <=> t >= 0 and !(k1 < 0) and s > 0 and !(k2 < 0).  (The record's own normal is NOT used: it is N
 *             normalised a second time.)
 *         Plane.   ip = d * t + E_k (scale, then add);  N' = dot(normal_o, d) < 0 ? reverse_normal_o : normal_o;
 *             O = ip + N' * 1e-3f,  D = d;  the child always exists.
 *      6. through <=> candidate and exists.
 *      7. mirror  <=> eligible and rf[o] >= min_reflective                                 (rt_mirror.h's, unchanged)
 *      8. follow  = through or mirror.
 *      9. If !follow or k == max_bounces: the terminal record is h, cut = follow ? 1 : 0, and the loop stops.
 *     10. If through (glass wins over mirror on an object that qualifies for both):
 *             ray_{k+1} = {O, O + D}
 *             d    = normalize((O + D) - O)
 *             w.j  = w.j * (tf[o] * h.color.j)
 *             A    unchanged
 *             a sphere, additionally:  L = L + s
 *             tag  = 1u + H((tag << 12) | (uint32_t)o | 0x80000000u) % 0x7fffeu
 *             g    = 1;  k = k + 1
 *     11. Else: rt_mirror.h's mirror step, word for word.
 * The outputs are rt_mirror.h's, with  out_path[i] = k | cut << 8 | g << 10 | tag << 12.  Bit 9 stays 0 (the step kernel uses
 * it in its scratch).  out_hits is required; out_guide, out_weight and out_path may each be NULL, and what is given does not
 * depend on which are.
 *
 * WHAT FOLLOWS.
 *   - With min_transmissive = +INFINITY, or on a scene without refractive objects, every output word is rt_mirror_records' for
 *     the same max_bounces, chunk_rays and min_reflective.
 *   - Through panes alone d keeps its value up to the rounding of normalize((O + D) - O), and the guide's point E + d0 * L is the
 *     terminal's point up to the 1e-3 offsets (DESIGN.md section 29 has the bound): reprojecting it by an earlier camera finds
 *     what stood behind the window then.
 *   - Through a sphere the guide is a definition, not a geometry, as it is for a curved mirror: L counts the chord, the point
 *     lies on the camera ray.
 *   - A candidate without a child -- total reflection at the far side of a sphere with ior < 1, an inside hit (t < 0) -- falls
 *     to the mirror rule: it is followed as a mirror if its `reflective` qualifies, and is the terminal otherwise.
 *   - The chain is this header's, not calculatePixel's bit for bit, in the same way as rt_mirror.h's: the render traces
 *     Ray(O, D) while a ray batch can only say {O, O + D}, and normalize((O + D) - O) may differ from D in the last bits.  At a
 *     silhouette seen through glass the terminal object can therefore differ from what the rendered colour's recursion met
 *     (measured: DESIGN.md section 29).
 *   - max_bounces counts mirrors and glass objects together; a glass sphere costs one.
 *   - A strip or any sub-batch equals the same rays of the whole batch; rows and chunk_rays never change a bit.
 *   - The guide's object is a tagged id and MUST NOT be used to index object tables (rt_mirror.h says what gets which record).
 *     A glass step's tag has bit 31 set in its hash's input, so a pane followed as glass and the same pane followed as a mirror
 *     give different ids.
 *
 * Argument checks, all before any device work, all RT_ERR_INVALID, in rt_mirror.h's order: (1) the scene is NULL; (2) params is
 * NULL; (3) max_bounces outside 0..RT_MIRROR_MAX_BOUNCES; (4) chunk_rays < 0; (5) min_reflective NaN, then min_transmissive
 * NaN; (6) n < 0; (7) rows < 1; (8) rays, then out_hits, NULL while n > 0; (9) the batch is beyond rt_trace_rays' limit;
 * (10) the device call only: d_rays not 4-byte aligned; then d_out_hits or a non-NULL d_out_guide not 16-byte aligned; then a
 * non-NULL weight or path not 4-byte aligned.  n == 0 is RT_OK and launches nothing.
 *
 * NO HOST SYNCHRONISATION in the device call, which can be captured into a graph once the scratch has been grown by an eager
 * call: each chunk enqueues max_bounces + 1 hit queries with a step kernel after each, exactly as rt_mirror_records_device does
 * (and, like it, a call on another stream than the handle's previous call first waits on the host for that previous stream:
 * INTEGRATION.md section 4, "Streams").
 * SCRATCH is rt_mirror_records' 128 bytes per ray of a chunk, kept in the scene handle apart from the mirror call's, and the
 * default chunk is the same.  The object table the step reads (48 bytes an object) is uploaded on the scene's first call.
 * Timing, lock and options are as rt_mirror.h says; rt_glass_info has rt_mirror_info's fields and layout.
 *
 * Not provided: more than one terminal per pixel (an object that both reflects and transmits is looked through, or followed as
 * a mirror, never both); Fresnel weighting; several GPUs; the counting build; a command-line flag.  The compacting form --
 * these chains over the rays still alive, as rt_mirror_compact.h is to rt_mirror.h -- is rt_glass_compact.h's
 * rt_glass_records_compact: whether a chain goes on depends here on the child's geometry (step 5's `exists`), and that
 * header's count pass evaluates steps 3 to 8 by the function its step uses.
 *
 * Buffers past 2^32 bytes: every offset is 64-bit, and tests/test_glass_large_gpu.py holds the device call to it bit for bit
 * on 100 000 007 rays of a refractive scene (4.8 GB of terminal records and of guide records, 2.4 GB of rays): the default
 * chunk (48 chunks, the chunk loop's byte offsets past 2^32), one chunk of 90 000 001 rays whose records and guide state planes
 * pass 2^32 bytes with a tail whose outputs begin past them, and that chunk again without guide and weight.  NOT tested: the
 * weights and the path words past 2^32 bytes (n > 357.9 million, n > 2^30 rays), the rays' element index 6 * ray past 2^32
 * (n > 715 827 882), and the host call rt_glass_records at such sizes (it stages the batch and runs the same chunk loop).
 *
 * rt_glass_params is 16 bytes; rt_glass_info is 32 bytes: rays at 0, chunks at 8, queries at 12, query_ms at 16, step_ms at 24.
 */
#ifndef RT_GLASS_H_
#define RT_GLASS_H_

#include "rt_mirror.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_GLASS_VERSION 1

typedef struct rt_glass_params {
    int32_t max_bounces;       /* 0..RT_MIRROR_MAX_BOUNCES: mirrors and glass objects followed, together                  */
    int32_t chunk_rays;        /* as rt_mirror_params                                                                     */
    float   min_reflective;    /* as rt_mirror_params                                                                     */
    float   min_transmissive;  /* a hit is looked through when its object's tf > 0 and tf >= this; not NaN; +INFINITY:    */
                               /* never                                                                                   */
} rt_glass_params;             /* 16 bytes */

typedef struct rt_glass_info {          /* of the scene's last rt_glass_records* call */
    int64_t rays;                       /* rays of the batch */
    int32_t chunks;                     /* chunks of rays the batch was walked in */
    int32_t queries;                    /* hit queries launched: chunks * (max_bounces + 1) */
    double  query_ms, step_ms;          /* HIP events, summed over the chunks and bounces */
} rt_glass_info;                        /* 32 bytes */

int rt_glass_version(void);

/* host memory, synchronous: n rays in; n records, n records, 3 n floats and n words out, the last three each or NULL */
int rt_glass_records(rt_scene *scene, const rt_glass_params *params, int n, int rows, const float *rays, rt_hit *out_hits,
                     rt_hit *out_guide, float *out_weight, uint32_t *out_path);

/* device memory on the scene's device, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising
 * (above); params is read before the call returns, the rays must stay alive until the stream has drained */
int rt_glass_records_device(rt_scene *scene, const rt_glass_params *params, int n, int rows, const void *d_rays,
                            void *d_out_hits, void *d_out_guide, void *d_out_weight, void *d_out_path, void *hip_stream);

/* the last rt_glass_records* call of the scene (all zero before the first); waits for that call's events */
int rt_get_glass_info(const rt_scene *scene, rt_glass_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RT_GLASS_H_ */
