/*
 * rt_capi_rays.h -- trace a batch of caller-supplied primary rays: fisheye, panoramic or lens cameras, jittered or adaptive
 * sampling, picking, many small views of one scene in one launch.  Plain C99, versioned on its own (RT_CAPI_RAYS_VERSION /
 * rt_capi_rays_version()); the drop-in surface of rt_capi.h is unchanged.
 *
 * Ray i is rays[6*i .. 6*i+5] = {E.x, E.y, E.z, T.x, T.y, T.z}, packed fp32: an origin E and a point T it passes through.
 * Its result is calculatePixel(Ray(E, normalize(T - E)), 0) with recursion limit max_depth (src/RayTracer.cpp:448-638): the
 * subtraction and the normalisation are createEyeRay's fp32 arithmetic (src/Camera.cpp:71-84), so a ray is exactly pixel
 * (0, 0) of a 1 x 1 frame whose camera has eye_origin = E, screen_origin = T and zero screen vectors and sizes (T with any
 * -0.0 read as +0.0: the camera adds zeros to it).  It is written to out_rgb[3*i .. 3*i+2], with no clamp (as rt_render).
 *
 * rows is a layout hint and never changes a result.  Ray i is cell (i / rows, i % rows) of an n_cols x rows grid,
 * n_cols = ceil(n / rows), and the kernel tiles that grid the way it tiles a W x H image (rows > n is read as rows = n).  A
 * W x H image's rays in pixels[x][z] order with rows = H are traced in the wavefront tiles rt_render would use; a flat list
 * passes rows = n.  Any order and any rows give the same bits per ray; only the speed differs.
 *
 * n = 0 is RT_OK and launches nothing.  These are RT_ERR_INVALID, checked in this order before any device work: the scene is
 * NULL; n < 0; rows < 1; max_depth < 0; rays or out_rgb is NULL while n > 0; 3n exceeds rt_render's strip limit (or the
 * n_cols x rows grid has 2^31 - 64 cells or more).  Error texts, rt_last_error(), rt_get_timing() (kernel ms, download ms),
 * the handle's lock and thread safety behave as for rt_render; rt_get_launch_info() names the *_rays kernel and its tile
 * shape in cells.
 *
 * Speed-only options (rt_capi_tuning.h) apply as for an image launch of n_cols x rows, except that there is no camera: the
 * PRIMARY table, the HEAVY band ("heavy"), the automatic start row and a learned tile order are never used.  "first_row",
 * "tile_z", "help", "cull", "fast", "tables" and "tile_prio" apply.  Without a "tile_z" option the tile is never wider than
 * n_cols rounded up to a power of two (a flat list gets 1 x 64 tiles).
 *
 * Not provided: ray batches with supersampling, the counting build (rt_render_stats), several GPUs.
 */
#ifndef RT_CAPI_RAYS_H_
#define RT_CAPI_RAYS_H_

#include "rt_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_RAYS_VERSION 1

int rt_capi_rays_version(void);

/* host memory, synchronous (as rt_render) */
int rt_trace_rays(rt_scene *scene, int n, int rows, const float *rays, int max_depth, float *out_rgb);

/* device memory on the scene's device, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising
 * (as rt_render_device); the caller keeps d_rays alive until the stream has drained */
int rt_trace_rays_device(rt_scene *scene, int n, int rows, const void *d_rays, int max_depth, void *d_out_rgb,
                         void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_RAYS_H_ */
