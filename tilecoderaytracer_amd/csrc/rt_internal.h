/*
 * rt_internal.h -- what the library's units ask of one another across their object files; nothing here is part of the ABI.
 * rt_capi.hip owns the handle (struct rt_scene), the error text, the argument rules and the launch policy -- one copy per rule.
 * Every other unit reports its errors through rt_internal_set_error and asks the device question through
 * rt_internal_check_device: rt_denoise.hip, rt_image.hip, rt_upsample.hip, rt_temporal.hip and rt_svgf.hip, which launch
 * kernels of their own and nothing else, and rt_adaptive.hip (include/rt_capi_adaptive.h), rt_lens.hip (include/rt_capi_lens.h)
 * rt_indirect.hip (include/rt_capi_indirect.h), rt_mirror.hip (include/rt_mirror.h), rt_mirror_compact.hip
 * (include/rt_mirror_compact.h), rt_glass.hip (include/rt_glass.h) and rt_glass_compact.hip (include/rt_glass_compact.h), which
 * compose rt_capi.hip's launches
 * through the calls below.  The host code those units share among themselves is rt_host.h, which includes this file.
 */
#ifndef RT_INTERNAL_H_
#define RT_INTERNAL_H_

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/rt_capi.h"

extern "C" {

/* A composing unit's place in the handle: its state (the handle's scratch for it and its last call's bookkeeping), made by
 * the unit on its first call; how rt_scene_destroy frees it; and the sum of its last call's stage times if that call made the
 * handle's launch number seq, else < 0 -- what rt_get_timing() reports as last_kernel_ms while the unit's call is the
 * handle's last launch. */
typedef struct rt_internal_unit {
    void *state;
    void (*free_state)(void *state);
    double (*stage_ms)(void *state, uint64_t seq);
} rt_internal_unit;
enum { RT_INTERNAL_UNIT_ADAPTIVE, RT_INTERNAL_UNIT_LENS, RT_INTERNAL_UNIT_INDIRECT, RT_INTERNAL_UNIT_MIRROR,
       RT_INTERNAL_UNIT_MIRROR_COMPACT, RT_INTERNAL_UNIT_PATHS, RT_INTERNAL_UNIT_GLASS, RT_INTERNAL_UNIT_PATHS_COMPACT,
       RT_INTERNAL_UNIT_GLASS_COMPACT, RT_INTERNAL_UNITS };

/* rt_capi.hip: the text behind rt_last_error(); returns code */
int rt_internal_set_error(int code, const char *msg);
/* rt_capi.hip: the device question every entry point asks last -- RT_ERR_NO_DEVICE without a HIP device, RT_ERR_INVALID for an
 * index out of range */
int rt_internal_check_device(int device);

/* ---- rt_capi.hip, for rt_adaptive.hip, rt_lens.hip and rt_indirect.hip ---- */
/* rt_render's checks in rt_render's order (the scene, the strip, the camera, the depth, the strip's size), no device work;
 * rt_internal_check_strip: the same without the scene */
int rt_internal_check_frame(const rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                            const void *out_rgb);
int rt_internal_check_strip(const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth, const void *out_rgb);
/* rt_render_ssaa's rule for the virtual size (samples 2 or 4: samples already checked) */
int rt_internal_check_virtual(const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth, int samples,
                              const void *out_rgb);
/* rt_render_gbuffer's size limit for columns x H pixels of colours and records */
int rt_internal_check_gbuffer_size(long long columns, int H);
/* the handle: its lock (held by the caller of everything below), its device, whether it has area lights, the place where it
 * keeps a unit's state (RT_INTERNAL_UNIT_*), and the number of render-kernel launches it has made */
void rt_internal_lock(rt_scene *s);
void rt_internal_unlock(rt_scene *s);
int rt_internal_scene_device(const rt_scene *s);
int rt_internal_scene_soft(const rt_scene *s);
rt_internal_unit *rt_internal_unit_slot(rt_scene *s, int unit);
uint64_t rt_internal_launch_seq(const rt_scene *s);
/* THE STREAM RULE, its one copy: what a call of this handle enqueues takes
 * effect after everything its earlier calls enqueued, whatever their streams -- they share the bounce stack, the ring of
 * tile-queue counters and every unit's scratch.  If hip_stream is not the stream of the handle's last call, the host waits here
 * for that stream to drain; hip_stream is then the handle's stream.  A call on the same stream waits for nothing.  launch()
 * calls it, and so does every composing unit's run(), after its grow()s and before the first thing it enqueues -- a unit's own
 * kernels (ray generation, say) write its scratch before its first launch().  Under the caller's lock, the device set. */
int rt_internal_order_stream(rt_scene *s, void *hip_stream);
/* launch() of a G-buffer strip and of a ray batch (rt_render_gbuffer_device's and rt_trace_rays_device's, arguments checked by
 * the caller for the former and by the batch's own rules for the latter), under the caller's lock */
int rt_internal_launch_gbuffer(rt_scene *s, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                               void *d_rgb, void *d_hits, void *hip_stream);
int rt_internal_launch_rays(rt_scene *s, int n, int rows, const void *d_rays, int max_depth, void *d_out_rgb, void *hip_stream);
/* launch() of a hit query of a ray batch (rt_intersect_rays_device's), likewise under the caller's lock */
int rt_internal_launch_hits(rt_scene *s, int n, int rows, const void *d_rays, void *d_out_hits, void *hip_stream);
/* the `diffuse` of every Scene object as given to rt_scene_create*, one float each, on the scene's device (uploaded on first
 * use, freed with the handle), and how many there are; under the caller's lock */
int rt_internal_object_diffuse(rt_scene *s, const float **d_kd, int *n_objects);
/* its twin for rt_mirror.hip and rt_mirror_compact.hip (include/rt_mirror.h): the `reflective` of every Scene object, likewise */
int rt_internal_object_reflective(rt_scene *s, const float **d_rf, int *n_objects);
/* its twin for rt_glass.hip and rt_glass_compact.hip (include/rt_glass.h): three float4 per Scene object -- {tf, ior, kind, 0} (tf and ior the object's
 * rt_refraction_desc, tf 0 where it has none; kind RT_KIND_* as a float), {a sphere's origin | a plane's normal}, {- | a plane's
 * reverse_normal} -- likewise */
int rt_internal_object_glass(rt_scene *s, const float4 **d_table, int *n_objects);
/* a device buffer that only grows (the device is synchronised before the old one is freed) */
int rt_internal_grow(void **buf, size_t *bytes, size_t need);

/* ---- rt_indirect.hip, for rt_paths.hip (include/rt_paths.h) ---- */
/* One rt_indirect_raygen_kernel launch, exactly as rt_indirect_diffuse_device enqueues it for a chunk: the n x n gather rays
 * (include/rt_capi_indirect.h) of m records at d_hits, record p sampling with key + p, 24 bytes each at d_rays; m n^2 < 2^31.
 * Device pointers, nothing checked, no wait. */
int rt_internal_indirect_raygen(int samples, uint32_t seed, uint32_t key, uint32_t m, const void *d_hits, void *d_rays,
                                void *hip_stream);

/* ---- rt_mirror_compact.hip ---- */
/* Its instantiation of rt_scan.h's two-level scan, enqueued on hip_stream exactly as the call enqueues it for a bounce's counts
 * (the call itself goes through here, and so do rt_glass_compact.hip and rt_paths_compact.hip, which have no scan kernels of their own), so that a test can give the scan more counts than any batch that fits a device would:
 * of n_counts > 0 counts, d_offsets[i] = the sum of the counts before i in i's group of kScanBlock (n_counts words),
 * d_group_sums[g] and d_group_base[g] = group g's sum and the sum of the groups before it (ceil(n_counts / kScanBlock) words
 * each), *d_total = the sum of all.  Device pointers, nothing checked, no wait. */
int rt_internal_mirror_compact_scan(const uint32_t *d_counts, uint32_t n_counts, uint32_t *d_offsets, uint32_t *d_group_sums,
                                    uint32_t *d_group_base, uint32_t *d_total, void *hip_stream);

}

#endif /* RT_INTERNAL_H_ */
