/*
 * rt_kernel_gbuffer.hip -- the G-buffer kernels of include/rt_capi_gbuffer.h for gfx950: rt_kernel.hip's five non-counting
 * kernels over a camera's frame, each pixel's colour as the plain kernel gives it and, beside it, the rt_hit record of its
 * camera ray's nearest hit -- phase 1 of level 0 has every field of it in registers (render_tile, kGbuffer).  Same body, same
 * launch bounds as the sibling each one is named after; the host takes every decision of rt_render for the frame, launches
 * them with RtParams::gbuffer_hits set and picks the sibling of what it would pick for the frame (rt_capi.hip,
 * choose_kernel()).
 */
#define RT_KERNEL_BODY_ONLY 1
#include "rt_kernel.hip"

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)
rt_render_kernel_gbuffer(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, false, false, true, false, false, RT_QUERY_NONE, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)
rt_render_kernel_items_gbuffer(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, false, false, false, false, false, RT_QUERY_NONE, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)
rt_render_kernel_large_gbuffer(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, true, false, false, false, false, false, RT_QUERY_NONE, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_CLUSTERS)
rt_render_kernel_clusters_gbuffer(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, true, false, false, false, false, RT_QUERY_NONE, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_WIDE)
rt_render_kernel_clusters_wide_gbuffer(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, true, true, false, false, false, RT_QUERY_NONE, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}
