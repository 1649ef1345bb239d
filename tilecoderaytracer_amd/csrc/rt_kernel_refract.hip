/*
 * rt_kernel_refract.hip -- the refraction kernels of include/rt_capi_refract.h for gfx950: the *_refract sibling of each
 * camera, supersampling, ray-batch and G-buffer kernel of the five table modes -- the image-texture body (a refractive scene
 * is always packed as an image scene) with the bounce chain walked as a ray tree (render_tile(), kRefract).  Same launch
 * bounds as the sibling each one is named after; the host picks them when the scene has a refractive object (rt_capi.hip,
 * choose_kernel()).  The ray queries answer geometry only and keep their kernels.
 */
#define RT_KERNEL_BODY_ONLY 1
#include "rt_kernel.hip"

/* render_body<kStats, kGlobalTables, kClusters, kRoomy, kFast, kSsaa, kRays, kQuery, kGbuffer, kImages, kRefract> for the five
 * kernels of one call: plain (FAST tables), items, large, clusters, clusters_wide */
#define RT_REFRACT_KERNELS(suffix, ssaa, rays, gbuffer)                                                                      \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel##suffix##_refract(RT_KERNEL_ARGS) {                                                                    \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, false, false, true, ssaa, rays, RT_QUERY_NONE, gbuffer, true, true>(                      \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area);                                                 \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel_items##suffix##_refract(RT_KERNEL_ARGS) {                                                              \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, false, false, false, ssaa, rays, RT_QUERY_NONE, gbuffer, true, true>(                     \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area);                                                 \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel_large##suffix##_refract(RT_KERNEL_ARGS) {                                                              \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, true, false, false, false, ssaa, rays, RT_QUERY_NONE, gbuffer, true, true>(                      \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area);                                                 \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_CLUSTERS)                       \
    rt_render_kernel_clusters##suffix##_refract(RT_KERNEL_ARGS) {                                                           \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, true, false, false, ssaa, rays, RT_QUERY_NONE, gbuffer, true, true>(                      \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area);                                                 \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_WIDE)                          \
    rt_render_kernel_clusters_wide##suffix##_refract(RT_KERNEL_ARGS) {                                                      \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, true, true, false, ssaa, rays, RT_QUERY_NONE, gbuffer, true, true>(                       \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area);                                                 \
    }

RT_REFRACT_KERNELS(, false, false, false)
RT_REFRACT_KERNELS(_ssaa, true, false, false)
RT_REFRACT_KERNELS(_rays, false, true, false)
RT_REFRACT_KERNELS(_gbuffer, false, false, true)
