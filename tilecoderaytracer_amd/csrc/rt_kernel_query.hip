/*
 * rt_kernel_query.hip -- the ray-query kernels of include/rt_capi_query.h for gfx950: rt_kernel.hip's five non-counting
 * kernels over a caller's ray batch (as rt_kernel_rays.hip), asking one question per ray instead of shading it.  The *_hits
 * kernels store getCollision's record (hits_tile()), the *_occluded kernels inShadeCollisionDetection's verdict for a segment
 * (occluded_tile(), with the bundle cull generalised to segments that end apart).  Same body, same launch bounds as the
 * sibling each one is named after; the host launches them as a ray batch at depth 0 and picks the sibling of what it would
 * pick for the batch (rt_capi.hip, choose_kernel()).
 */
#define RT_KERNEL_BODY_ONLY 1
#include "rt_kernel.hip"

#define RT_QUERY_KERNELS(suffix, query)                                                                                     \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel_##suffix(RT_KERNEL_ARGS) {                                                                             \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, false, false, true, false, true, query>(p, image, out, tile_counter, bounce_stack, nullptr, help_area); \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel_items_##suffix(RT_KERNEL_ARGS) {                                                                       \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, false, false, false, false, true, query>(p, image, out, tile_counter, bounce_stack, nullptr, help_area); \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel_large_##suffix(RT_KERNEL_ARGS) {                                                                       \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, true, false, false, false, false, true, query>(p, image, out, tile_counter, bounce_stack, nullptr, help_area); \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_CLUSTERS)                       \
    rt_render_kernel_clusters_##suffix(RT_KERNEL_ARGS) {                                                                    \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, true, false, false, false, true, query>(p, image, out, tile_counter, bounce_stack, nullptr, help_area); \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_WIDE)                          \
    rt_render_kernel_clusters_wide_##suffix(RT_KERNEL_ARGS) {                                                               \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, true, true, false, false, true, query>(p, image, out, tile_counter, bounce_stack, nullptr, help_area); \
    }

RT_QUERY_KERNELS(hits, RT_QUERY_HITS)
RT_QUERY_KERNELS(occluded, RT_QUERY_OCCLUDED)
