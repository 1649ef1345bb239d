/*
 * rt_kernel_rays.hip -- the ray-batch kernels of include/rt_capi_rays.h for gfx950: rt_kernel.hip's five non-counting kernels
 * over a caller's rays instead of a camera's.  Ray i = {E, T} is cell (i / rows, i % rows) of an n_cols x rows grid, tiled as
 * an image is; its direction is normalize(T - E), and the level-0 scans take the wavefront's bounds of the origins, without
 * the PRIMARY table (render_tile, kRays).  Same body, same launch bounds as the sibling each one is named after; the host
 * launches them with RtParams::n_rays / rays set and picks the sibling of what it would pick for the image (rt_capi.hip,
 * choose_kernel()).
 */
#define RT_KERNEL_BODY_ONLY 1
#include "rt_kernel.hip"

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)
rt_render_kernel_rays(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, false, false, true, false, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)
rt_render_kernel_items_rays(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, false, false, false, false, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)
rt_render_kernel_large_rays(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, true, false, false, false, false, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_CLUSTERS)
rt_render_kernel_clusters_rays(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, true, false, false, false, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_WIDE)
rt_render_kernel_clusters_wide_rays(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, true, true, false, false, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}
