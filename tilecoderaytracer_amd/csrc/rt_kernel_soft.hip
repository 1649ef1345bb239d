/*
 * rt_kernel_soft.hip -- the soft-shadow kernels of include/rt_capi_soft.h for gfx950: the *_soft sibling of each camera,
 * supersampling, ray-batch and G-buffer kernel of the five table modes -- the image-texture body (an area-light scene is always
 * packed as an image scene) whose lights with a radius run one shadow scan per sample of their disc (render_tile(), kSoft) --
 * and the *_refract_soft sibling of each refraction kernel.  Same launch bounds as the sibling each one is named after; the host
 * picks them when the scene has an area light (rt_capi.hip, choose_kernel()); the large-table ones ask for the eight wavefronts per
 * SIMD their siblings reach unasked (below).  The launch's sampling seed is one more kernel
 * argument behind the shared ones (rt_tables.h, RT_SOFT_QUADS), so RtParams and the other kernels do not change.
 */
#define RT_KERNEL_BODY_ONLY 1
#include "rt_kernel.hip"

#define RT_SOFT_KERNEL_ARGS RT_KERNEL_ARGS, const uint32_t shadow_seed

/* The large-table siblings (tables in global memory) need 52-62 VGPRs and so run 8 wavefronts per SIMD although their bound
 * asks for RT_WAVES_PER_SIMD only; the sample loop would take their soft siblings to 72 registers and 7 wavefronts.  These ask
 * for the 8 their siblings reach (no *_soft kernel runs below its sibling's occupancy). */
#define RT_WAVES_PER_SIMD_LARGE_SOFT 8

/* render_body<kStats, kGlobalTables, kClusters, kRoomy, kFast, kSsaa, kRays, kQuery, kGbuffer, kImages, kRefract, kSoft> for the
 * five kernels of one call: plain (FAST tables), items, large, clusters, clusters_wide */
#define RT_SOFT_KERNELS(suffix, ssaa, rays, gbuffer, refract, tail)                                                         \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel##suffix##tail(RT_SOFT_KERNEL_ARGS) {                                                                   \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, false, false, true, ssaa, rays, RT_QUERY_NONE, gbuffer, true, refract, true>(             \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area, shadow_seed);                                    \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD)                                         \
    rt_render_kernel_items##suffix##tail(RT_SOFT_KERNEL_ARGS) {                                                             \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, false, false, false, ssaa, rays, RT_QUERY_NONE, gbuffer, true, refract, true>(            \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area, shadow_seed);                                    \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND, RT_WAVES_PER_SIMD_LARGE_SOFT)                              \
    rt_render_kernel_large##suffix##tail(RT_SOFT_KERNEL_ARGS) {                                                             \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, true, false, false, false, ssaa, rays, RT_QUERY_NONE, gbuffer, true, refract, true>(             \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area, shadow_seed);                                    \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_CLUSTERS)                       \
    rt_render_kernel_clusters##suffix##tail(RT_SOFT_KERNEL_ARGS) {                                                          \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, true, false, false, ssaa, rays, RT_QUERY_NONE, gbuffer, true, refract, true>(             \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area, shadow_seed);                                    \
    }                                                                                                                       \
    extern "C" __global__ void __launch_bounds__(RT_BLOCK_BOUND_CLUSTERS, RT_WAVES_PER_SIMD_WIDE)                          \
    rt_render_kernel_clusters_wide##suffix##tail(RT_SOFT_KERNEL_ARGS) {                                                     \
        RT_PARAMS_FROM_KERNARG(p, p_in_kernarg);                                                                            \
        render_body<false, false, true, true, false, ssaa, rays, RT_QUERY_NONE, gbuffer, true, refract, true>(              \
            p, image, out, tile_counter, bounce_stack, nullptr, help_area, shadow_seed);                                    \
    }

RT_SOFT_KERNELS(, false, false, false, false, _soft)
RT_SOFT_KERNELS(_ssaa, true, false, false, false, _soft)
RT_SOFT_KERNELS(_rays, false, true, false, false, _soft)
RT_SOFT_KERNELS(_gbuffer, false, false, true, false, _soft)
RT_SOFT_KERNELS(, false, false, false, true, _refract_soft)
RT_SOFT_KERNELS(_ssaa, true, false, false, true, _refract_soft)
RT_SOFT_KERNELS(_rays, false, true, false, true, _refract_soft)
RT_SOFT_KERNELS(_gbuffer, false, false, true, true, _refract_soft)
