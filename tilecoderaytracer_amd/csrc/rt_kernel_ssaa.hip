/*
 * rt_kernel_ssaa.hip -- the supersampling kernels of include/rt_capi_ssaa.h for gfx950: rt_kernel.hip's five
 * non-counting kernels over the virtual kW x kH image of k x k samples per pixel, each pixel's samples averaged in the
 * wavefront at the store (render_tile, kSsaa).  Same body, same launch bounds as the sibling each one is named after; the
 * host launches them with RtParams::ssaa_log2 = 1 or 2 and picks the sibling of what it would pick without supersampling
 * (rt_capi.hip, choose_kernel()).
 */
#define RT_KERNEL_BODY_ONLY 1
#include "rt_kernel.hip"

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)
rt_render_kernel_ssaa(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, false, false, true, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)
rt_render_kernel_items_ssaa(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, false, false, false, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)
rt_render_kernel_large_ssaa(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, true, false, false, false, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_CLUSTERS)
rt_render_kernel_clusters_ssaa(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, true, false, false, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}

extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_WIDE)
rt_render_kernel_clusters_wide_ssaa(RT_KERNEL_ARGS) {
    RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);
    render_body<false, false, true, true, false, true>(p, image, out, tile_counter, bounce_stack, nullptr, help_area);
}
