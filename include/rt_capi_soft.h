/*
 * rt_capi_soft.h -- soft shadows: spherical lights sampled as area lights inside every render kernel.  The reference traces one
 * shadow segment per light to its centre (inShade, src/RayTracer.cpp:743-771), so even a large light casts razor-edged
 * shadows; this header defines a stratified visibility estimate over the light's disc.  Plain C99, versioned on its own
 * (RT_CAPI_SOFT_VERSION / rt_capi_soft_version()); rt_capi.h, rt_capi_tuning.h, rt_object_desc, RT_CAPI_VERSION and
 * RT_CAPI_TUNING_VERSION are unchanged.
 *
 * CREATE.  rt_scene_create_soft(desc, n_images, images, n_refractive, refractive, n_area_lights, area_lights, ...) is
 * rt_scene_create_refractive with a list of area lights beside it.  Entries with radius == 0 are ignored; when none is left the
 * call is exactly rt_scene_create_refractive: the same tables, the same kernels, the same bits (which in turn falls back to
 * rt_scene_create_textured and rt_scene_create).
 *
 * DEFINITION.  All arithmetic is IEEE fp32 with no contraction; dot, add, sub, scale, normalize and length are the reference's
 * vector3d operations (the oracle's v_* operations), in the order written.  H(x) is the 32-bit integer hash "lowbias32":
 *
 *     x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16       (uint32 arithmetic)
 *
 * At a shaded hit (not a light) of level k, with point P, for the light with ordinal l among the scene's lights (Scene order),
 * centre C, radius r and n x n samples:
 *
 *     L    = normalize(sub(C, P))          (the reference's light_ray: the cosine and specular terms still use it)
 *     A    = fabsf(L.x) < 0.5f ? (1,0,0) : (0,1,0)
 *     U    = normalize(cross(A, L))        V = cross(L, U)
 *            cross(a,b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
 *     h    = H(H(H(H(seed ^ 0x9e3779b9u) ^ key) ^ (uint32)k) ^ (uint32)l)
 *     step = 2.0f / (float)n
 *     for i, j in [0, n):  s = i*n + j
 *         hs  = H(h ^ s)
 *         xi1 = (float)(hs >> 8) * 0x1p-24f          xi2 = (float)(H(hs ^ 0x9e3779b9u) >> 8) * 0x1p-24f
 *         a   = ((float)i + xi1) * step - 1.0f       b   = ((float)j + xi2) * step - 1.0f
 *         dx  = a * sqrtf(1.0f - (b*b) * 0.5f)       dy  = b * sqrtf(1.0f - (a*a) * 0.5f)   (square -> disc, no trigonometry)
 *         Q   = add(C, add(scale(U, r*dx), scale(V, r*dy)))
 *         sample s is visible  <=>  !inShadeCollisionDetection(Ray(P, sub(Q, P)), length(sub(Q, P)))
 *     m = visible samples, S = n*n
 *     m == 0: the light adds nothing (the reference's in-shade branch: neither term, and the clamp does not run)
 *     m >  0: f = (float)m / (float)S; the reference's cosineShade and specular code run unchanged except
 *             factor      = factor * f         (after factor = cos * diffuse * intensity)
 *             spec_factor = spec_factor * f    (after spec_factor = pow_factor * specular)
 *
 * key: camera launches (rt_render*, rt_render_gbuffer*): x * H + z in uint32, with the frame's global column x and height H,
 * so a strip is bit-identical to the same columns of the full frame; supersampled launches: the same over the virtual kW x kH
 * launch; ray batches (rt_trace_rays*): the ray index.  In a refractive scene (include/rt_capi_refract.h) k is the node's
 * level in the ray tree.  seed: rt_scene_set_shadow_seed(), 0 by default.
 *
 * A light that is not in the list keeps the reference's hard shadow: one segment to C, no sampling and no hashing (it is not
 * evaluated as Q = C + 0, which could flip the sign of a zero).  When f = 1, x * 1.0f == x: a pixel none of whose samples is
 * blocked is bit-identical to the hard-shadow render.
 *
 * LIMITS.  The samples are drawn on a disc facing P, not on the sphere; there is no importance weighting (every sample counts
 * 1 / S); a sample that a NaN spoils gets the verdict the reference's scan gives it.  Glass still blocks fully.
 *
 * COST.  One shadow scan per sample: an area light costs S = n*n times the hard light's shadow scans at each shading point.
 *
 * ERRORS.  All before any device work.  RT_ERR_INVALID: desc or out is NULL; n_area_lights < 0; area_lights is NULL while
 * n_area_lights > 0; then entry by entry (entries with radius == 0 included): an object index out of range, an object that is
 * not a light, an object listed twice, samples outside 1..8, a negative, NaN or infinite radius.  Then
 * rt_scene_create_refractive's checks.
 *
 * CALLS.  On a scene with area lights, bit-exact to the definition above: rt_render / _device, rt_render_ssaa / _device,
 * rt_trace_rays / _device and rt_render_gbuffer / _device (the colours; its hit records do not change); rt_get_launch_info()
 * names the *_soft kernel: the name of the kernel the same call runs on a scene with neither images, refraction nor area
 * lights, + "_soft", or + "_refract_soft" when the scene is refractive (e.g. rt_render_kernel_ssaa_soft,
 * rt_render_kernel_rays_refract_soft).  An area-light scene is always packed as an image scene, so its ray queries
 * (rt_intersect_rays, rt_occluded_rays: geometry, unchanged) run the *_image kernels.  Not provided: the counting build
 * (rt_render_stats, rt_learn_tile_order: RT_ERR_INVALID on a scene with area lights) and the multi-GPU path.
 */
#ifndef RT_CAPI_SOFT_H_
#define RT_CAPI_SOFT_H_

#include "rt_capi.h"
#include "rt_capi_texture.h"
#include "rt_capi_refract.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_SOFT_VERSION 1

typedef struct rt_area_light_desc {
    int32_t object;            /* Scene index of a light (is_light != 0), any kind                      */
    int32_t samples;           /* n: n x n stratified samples per shading point, 1 <= n <= 8            */
    float   radius;            /* r: radius of the light's disc, finite, >= 0 (0: entry ignored)        */
} rt_area_light_desc;

int rt_capi_soft_version(void);

/* rt_scene_create_refractive with area lights */
int rt_scene_create_soft(const rt_scene_desc *desc, int n_images, const rt_image_texture_desc *images,
                         int n_refractive, const rt_refraction_desc *refractive,
                         int n_area_lights, const rt_area_light_desc *area_lights, int device, rt_scene **out);

/* the sampling seed of the scene's later launches (default 0); a launch already enqueued keeps its seed */
int rt_scene_set_shadow_seed(rt_scene *scene, uint32_t seed);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_SOFT_H_ */
