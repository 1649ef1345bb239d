/*
 * rt_capi_gbuffer.h -- a camera frame's colours and, beside them, each pixel's hit record in one launch: the render passes
 * (AOVs) of object id, depth, point, normal and albedo that compositing, picking overlays and post-processing (fog, depth
 * of field, object mattes) expect next to the image.  Plain C99, versioned on its own (RT_CAPI_GBUFFER_VERSION /
 * rt_capi_gbuffer_version()); rt_capi.h and the other extension headers are unchanged.
 *
 * For columns [x0, x1) of a W x H frame of cam with recursion limit max_depth:
 *   out_rgb[((x-x0)*H + z)*3 + c]   is bit for bit what rt_render gives for the same arguments, in its layout (no clamp, no
 *                                   gamma);
 *   out_hits[(x-x0)*H + z]          is bit for bit the rt_hit (rt_capi_query.h) that rt_intersect_rays gives for the pixel's
 *                                   camera ray {eye_origin, pixel point}, the point built in createEyeRay's fp32 arithmetic
 *                                   (src/Camera.cpp:71-84, dx = (float)x / W, dz = (float)z / H): the record of
 *                                   getCollision(Ray(E, normalize(T - E))) -- object, distance (negative for an inside sphere
 *                                   hit), point (a plane's offset 1e-3 along its normal), normal (re-normalised as the
 *                                   CollisionObject ctor does), the material's or the checker tile's colour, flags
 *                                   (RT_HIT_INSIDE, RT_HIT_LIGHT).  A miss is object -1 and every other bit 0.
 * The record is the nearest hit of the camera ray alone: it does not depend on max_depth, and max_depth = 0 is allowed.  A
 * strip is bit-identical to the same columns of a whole frame, in both outputs.
 *
 * Argument checks, all before any device work, RT_ERR_INVALID in this order -- rt_render's, in rt_render's order, then the
 * record's: the scene is NULL; W or H not positive, or not 0 <= x0 <= x1 <= W; out_rgb is NULL while the strip is not empty;
 * the camera is NULL; max_depth < 0; the strip's colours exceed rt_render's limit; out_hits is NULL while the strip is not
 * empty; the strip's colours and records together exceed 3.2e10 bytes, i.e. (x1 - x0) * H > 533 333 333 pixels (60 bytes
 * each); for the device variant, d_out_hits is not 16-byte aligned.  An empty strip (x0 == x1) is RT_OK and launches nothing.
 *
 * Timing: rt_get_timing() reports the kernel (last_kernel_ms, sum_kernel_ms, as for rt_render); the host variant's
 * last_download_ms covers both copies, colours and records.  rt_get_launch_info() names the *_gbuffer
 * sibling of the kernel rt_render would run and its tile shape.  Error texts, rt_last_error(), the handle's lock and thread
 * safety behave as for rt_render.
 *
 * Speed-only options (rt_capi_tuning.h) apply as for rt_render of the same frame: every decision of the launch is rt_render's
 * -- the PRIMARY table, the HEAVY band, the horizon start row, HELP, "first_row", "tile_z", "cull", "fast", "tables",
 * "tile_prio", and a tile order learned by rt_learn_tile_order for the same shape.
 *
 * Not provided: supersampling, the counting build (rt_render_stats), several GPUs, and a record-only camera launch
 * (rt_intersect_rays on the frame's own rays gives that).
 */
#ifndef RT_CAPI_GBUFFER_H_
#define RT_CAPI_GBUFFER_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_GBUFFER_VERSION 1

int rt_capi_gbuffer_version(void);

/* host memory, synchronous (as rt_render): out_rgb holds 3 (x1 - x0) H floats, out_hits (x1 - x0) H records */
int rt_render_gbuffer(rt_scene *scene, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                      float *out_rgb, rt_hit *out_hits);

/* device memory on the scene's device, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising
 * (as rt_render_device).  d_out_rgb holds 12 (x1 - x0) H bytes, d_out_hits 48 (x1 - x0) H bytes, 16-byte aligned. */
int rt_render_gbuffer_device(rt_scene *scene, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                             void *d_out_rgb, void *d_out_hits, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_GBUFFER_H_ */
