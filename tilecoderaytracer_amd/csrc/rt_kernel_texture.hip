/*
 * rt_kernel_texture.hip -- the image-texture kernels of include/rt_capi_texture.h for gfx950: the *_image sibling of each
 * non-counting camera, supersampling, ray-batch, nearest-hit query and G-buffer kernel -- the same body with planes that may
 * sample an image (render_tile / hits_tile, kImages): a hit's texture selector is its texel's index, the colour a plain load
 * of that texel wherever the checkerboard's colour would be taken.  Same launch bounds as the sibling each one is named after;
 * the host takes every decision it takes for the same call on a scene without images and picks the *_image sibling when the
 * scene references an image (rt_capi.hip, choose_kernel()).  The occlusion queries read no colour: their kernels serve both.
 */
#define RT_KERNEL_BODY_ONLY 1
#include "rt_kernel.hip"

/* render_body<kStats, kGlobalTables, kClusters, kRoomy, kFast, kSsaa, kRays, kQuery, kGbuffer, kImages> for the five kernels of
 * one call: plain (FAST tables), items, large, clusters, clusters_wide */
#define RT_IMAGE_KERNELS(suffix, ssaa, rays, query, gbuffer)                                                                 \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel##suffix##_image(RT_KERNEL_ARGS) {                                                                      \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, false, false, true, ssaa, rays, query, gbuffer, true>(p, image, out, tile_counter,        \
                                                                                       bounce_stack, nullptr, help_area);   \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel_items##suffix##_image(RT_KERNEL_ARGS) {                                                                \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, false, false, false, ssaa, rays, query, gbuffer, true>(p, image, out, tile_counter,       \
                                                                                        bounce_stack, nullptr, help_area);  \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel_large##suffix##_image(RT_KERNEL_ARGS) {                                                                \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, true, false, false, false, ssaa, rays, query, gbuffer, true>(p, image, out, tile_counter,        \
                                                                                       bounce_stack, nullptr, help_area);   \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_CLUSTERS)                       \
    rt_render_kernel_clusters##suffix##_image(RT_KERNEL_ARGS) {                                                             \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, true, false, false, ssaa, rays, query, gbuffer, true>(p, image, out, tile_counter,        \
                                                                                       bounce_stack, nullptr, help_area);   \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_WIDE)                          \
    rt_render_kernel_clusters_wide##suffix##_image(RT_KERNEL_ARGS) {                                                        \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, true, true, false, ssaa, rays, query, gbuffer, true>(p, image, out, tile_counter,         \
                                                                                      bounce_stack, nullptr, help_area);    \
    }

RT_IMAGE_KERNELS(, false, false, RT_QUERY_NONE, false)
RT_IMAGE_KERNELS(_ssaa, true, false, RT_QUERY_NONE, false)
RT_IMAGE_KERNELS(_rays, false, true, RT_QUERY_NONE, false)
RT_IMAGE_KERNELS(_hits, false, true, RT_QUERY_HITS, false)
RT_IMAGE_KERNELS(_gbuffer, false, false, RT_QUERY_NONE, true)
