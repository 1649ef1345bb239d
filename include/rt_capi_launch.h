/*
 * rt_capi_launch.h -- the whole name of the render kernel a handle's last launch ran.  rt_launch_info.kernel
 * (rt_capi_tuning.h) holds 48 bytes, and its size is part of that header's ABI; the catalogue's names (csrc/rt_tables.h,
 * RENDER KERNELS: rt_render_kernel<mode><family>) run to 51 characters, rt_render_kernel_clusters_wide_gbuffer_refract_soft,
 * which rt_launch_info cuts to 47.  Plain C99, versioned on its own (RT_CAPI_LAUNCH_VERSION / rt_capi_launch_version());
 * rt_capi.h, rt_capi_tuning.h and the other extension headers are unchanged.
 *
 * rt_get_launch_kernel(scene, out, n_bytes) copies the NUL-terminated name of the __global__ function the scene's last
 * launch ran (its first pass; "" before the first launch) into out: every launch that rt_get_launch_info() describes --
 * rt_render, rt_render_ssaa, rt_trace_rays, the ray queries, rt_render_gbuffer and their device variants, the counting
 * build.  rt_launch_info.kernel is its first 47 characters.  RT_KERNEL_NAME_BYTES bytes always suffice (the library checks
 * every name of the catalogue against it when it is compiled).  RT_ERR_INVALID, before anything is written: the scene or
 * out is NULL; n_bytes is smaller than the name and its NUL.
 */
#ifndef RT_CAPI_LAUNCH_H_
#define RT_CAPI_LAUNCH_H_

#include "rt_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_LAUNCH_VERSION 1
#define RT_KERNEL_NAME_BYTES 64

int rt_capi_launch_version(void);

int rt_get_launch_kernel(const rt_scene *scene, char *out, int n_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_LAUNCH_H_ */
