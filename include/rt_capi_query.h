/*
 * rt_capi_query.h -- ask the scene about a batch of caller-supplied rays: what each ray hits (picking, G-buffers of object
 * id, depth, normal and albedo, the caller's own shading) and whether a segment is blocked (the caller's own lights,
 * visibility between points, ambient-occlusion estimators).  Plain C99, versioned on its own (RT_CAPI_QUERY_VERSION /
 * rt_capi_query_version()); rt_capi.h and rt_capi_rays.h are unchanged.
 *
 * INTERSECT.  Ray i is rays[6*i .. 6*i+5] = {E.x, E.y, E.z, T.x, T.y, T.z}, packed fp32, as for rt_trace_rays: an origin E
 * and a point T it passes through, direction normalize(T - E) in createEyeRay's fp32 arithmetic (src/Camera.cpp:71-84).  Its
 * record out_hits[i] is getCollision(Ray(E, normalize(T - E))) over Scene objects [0, n_objects) (src/RayTracer.cpp:50-89):
 * the nearest CollisionObject, the lowest Scene index among equal distances, with the reference's arithmetic bit for bit:
 *   object    the winner's Scene index; -1: no hit
 *   distance  CollisionObject::distance.  A sphere hit from inside reports v - sqrt(d^2), which is negative; its point is
 *             that root's point (src/SceneSphere.cpp:50-168)
 *   point     intersection_point; a plane's is offset 1e-3 along computeNormal(direction) (src/SceneFinitePlane.cpp:100-150,
 *             src/SceneInfinitePlane.cpp likewise)
 *   normal    normal_ray's direction: the object's normal as the CollisionObject ctor re-normalises it
 *   color     the material's colour, or the colour of the checkerboard tile the point lies on
 *   flags     bit 0: an inside hit (sphere); bit 1: the winner is a light
 * A miss is object = -1 and every other field +0.0 / 0.  Only the record is produced: no shading, no shadow rays.  A
 * record's point fed back as E of an occlusion segment towards a light reproduces the reference's shadow ray from that hit.
 *
 * OCCLUDED.  Segment i is segs[6*i .. 6*i+5] = {E, T} in the same layout.  out_blocked[i] is
 * inShadeCollisionDetection(Ray(E, T - E), |T - E|) (src/RayTracer.cpp:709-739): inShade (:743-771) with intersection point
 * E and a light at T.  The scan covers [shadow_begin, shadow_end) of the scene, skips lights and blocks on distance < |T - E|,
 * so a sphere that contains E blocks.  The value is 0 or 1.
 *
 * rows is a layout hint and never changes a result, as for rt_trace_rays: ray i is cell (i / rows, i % rows) of an
 * n_cols x rows grid tiled like an image (rows > n is read as rows = n).  Any order and any rows give the same bits per ray.
 *
 * n = 0 is RT_OK and launches nothing.  These are RT_ERR_INVALID, checked in this order before any device work: the scene is
 * NULL; n < 0; rows < 1; the input or the output is NULL while n > 0; the batch exceeds rt_trace_rays's limit.  Error texts,
 * rt_last_error(), rt_get_timing() (kernel ms, download ms), the handle's lock and thread safety behave as for rt_trace_rays;
 * rt_get_launch_info() names the *_hits or *_occluded kernel and its tile shape in cells.
 *
 * Speed-only options (rt_capi_tuning.h) apply as for a ray batch ("first_row", "tile_z", "cull", "fast", "tables",
 * "tile_prio"); "help" does not apply (a query launch has no HELP desk) and there is no bounce stack.
 *
 * Not provided: supersampling, the counting build (rt_render_stats), several GPUs.
 */
#ifndef RT_CAPI_QUERY_H_
#define RT_CAPI_QUERY_H_

#include "rt_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_QUERY_VERSION 1

/* 48 bytes: the reference's CollisionObject (src/SceneObject.h:36-105), as above */
typedef struct rt_hit {
    int32_t object;
    float distance;
    float point[3];
    float normal[3];
    float color[3];
    int32_t flags;
} rt_hit;

#define RT_HIT_INSIDE 1
#define RT_HIT_LIGHT 2

int rt_capi_query_version(void);

/* host memory, synchronous (as rt_trace_rays) */
int rt_intersect_rays(rt_scene *scene, int n, int rows, const float *rays, rt_hit *out_hits);
int rt_occluded_rays(rt_scene *scene, int n, int rows, const float *segs, uint8_t *out_blocked);

/* device memory on the scene's device, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising
 * (as rt_trace_rays_device); the caller keeps the input alive until the stream has drained.  d_out_hits is 48 n bytes, 16-byte
 * aligned; d_out_blocked is n bytes. */
int rt_intersect_rays_device(rt_scene *scene, int n, int rows, const void *d_rays, void *d_out_hits, void *hip_stream);
int rt_occluded_rays_device(rt_scene *scene, int n, int rows, const void *d_segs, void *d_out_blocked, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_QUERY_H_ */
