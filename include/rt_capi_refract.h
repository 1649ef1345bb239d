/*
 * rt_capi_refract.h -- refraction: transmissive spheres and panes, traced inside every render kernel.  The reference leaves
 * refraction as an open TODO after its reflection term (src/RayTracer.cpp:606-616) and keeps ObjMaterial::refractive_factor
 * (src/ObjMaterial.h:18,52) unused; this header defines the transmission term it would add.  Plain C99, versioned on its own
 * (RT_CAPI_REFRACT_VERSION / rt_capi_refract_version()); rt_capi.h, rt_object_desc and RT_CAPI_VERSION are unchanged.
 *
 * CREATE.  rt_scene_create_refractive(desc, n_images, images, n_refractive, refractive, ...) is rt_scene_create_textured with
 * a list of refractive objects beside it.  Entries with refractive == 0 are ignored; when none is left the call is exactly
 * rt_scene_create_textured: the same tables, the same kernels, the same bits.
 *
 * DEFINITION.  All arithmetic is IEEE fp32 with no contraction; dot, scale, add, sub and normalize are the reference's
 * vector3d operations (the oracle's v_dot / v_scale / v_add / v_sub / v_normalize), in the order written.  At a shaded hit
 * of level k (not a light) on an object with transmission factor tf > 0:
 *
 *     final_k = (local_k + (rf * C_refl) * oc) + (tf * C_refr) * oc
 *
 * The reflection term is the reference's and is added first, only if rf > 0.  The transmission term is added second, only
 * if the transmitted child exists.  C_refr = calculatePixel(child, k + 1): NULL_COLOR when k + 1 > max_depth (the child's
 * existence is still decided by the geometry below, on the last level too).  oc is the texel- or checkerboard-resolved
 * object colour, as in the reflection term.
 *
 * Sphere, outside hit (t >= 0: the reference's insideHit == false).  P = d t + E and N are the hit record's, Q = sub(P,
 * centre), N = normalize(Q), eta = 1.0f / ior:
 *     c1 = -dot(N, d)
 *     k1 = 1 - (eta * eta) * (1 - c1 * c1)                 k1 < 0: no child
 *     T1 = normalize(add(scale(d, eta), scale(N, eta * c1 - sqrtf(k1))))
 *     s  = -2.0f * dot(T1, Q)                               !(s > 0): no child
 *     P2 = add(P, scale(T1, s))
 *     N2 = normalize(sub(P2, centre))
 *     c2 = dot(N2, T1)
 *     k2 = 1 - (ior * ior) * (1 - c2 * c2)                  k2 < 0: no child
 *     T2 = sub(scale(T1, ior), scale(N2, ior * c2 - sqrtf(k2)))
 *     child = { origin add(P2, scale(N2, 1e-3f)), direction normalize(T2) }
 * The sphere is solid glass crossed along one chord.  Two limits follow: objects inside a glass sphere are not seen through
 * it, and internal reflections are not followed (a ray that would be totally reflected inside has no child).
 *
 * Sphere, inside hit (t < 0): no transmitted child (the reference reports such hits behind the ray).
 *
 * Plane (infinite or finite): a thin pane, no bending.  ip = d t + E is the point before the 1e-3 offset, N' the other of the
 * plane's two stored normals (normal / reverse_normal: the one the hit record did not choose):
 *     child = { origin add(ip, scale(N', 1e-3f)), direction d }   (d's bits unchanged)
 *
 * Otherwise a refractive object is an ordinary object: it is hit, shaded and reflects as before, and it blocks shadow rays
 * fully (no coloured shadows).  rt_intersect_rays and rt_occluded_rays answer geometry and do not change; rt_render_gbuffer's
 * records stay the primary hit, its colours include refraction.
 *
 * COST.  The rays traced per pixel are the size of its ray tree: an object that both reflects and transmits doubles the rays
 * at each level it is met, up to 2^(max_depth + 1) - 1 per pixel.  The tree is not capped; choose max_depth accordingly.  The
 * bounce stack stays max_depth + 1 levels per lane, at 48 bytes a level instead of 16.
 *
 * ERRORS.  All before any device work.  RT_ERR_INVALID: desc or out is NULL; n_refractive < 0; refractive is NULL while
 * n_refractive > 0; then entry by entry (entries with refractive == 0 included): an object index out of range, an object
 * listed twice, a light, a NaN or negative refractive, an ior that is not finite and > 0.  Then rt_scene_create_textured's
 * checks.
 *
 * CALLS.  On a refractive scene, bit-exact to the definition above: rt_render / _device, rt_render_ssaa / _device,
 * rt_trace_rays / _device and rt_render_gbuffer / _device; rt_get_launch_info() names the *_refract kernel, whose name is the
 * name of the kernel the same call runs on the scene with neither images nor refraction, + "_refract" (e.g.
 * rt_render_kernel_ssaa_refract).  A refractive scene is always packed as an image scene, every checkerboard as its 2 x 2
 * CHECKER image (the same pixels), so its ray queries run the *_image kernels.
 *
 * Not provided: the counting build (rt_render_stats, rt_learn_tile_order: RT_ERR_INVALID on a refractive scene) and the
 * multi-GPU path.  Out of scope: nested or interior objects inside glass, internal reflections, Fresnel weighting,
 * absorption and coloured shadows.
 */
#ifndef RT_CAPI_REFRACT_H_
#define RT_CAPI_REFRACT_H_

#include "rt_capi.h"
#include "rt_capi_texture.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_REFRACT_VERSION 1

typedef struct rt_refraction_desc {
    int32_t object;      /* Scene index of a sphere or plane, not a light                                  */
    float   refractive;  /* tf, ObjMaterial::refractive_factor: >= 0 (not NaN)                              */
    float   ior;         /* index of refraction of a sphere's interior: finite, > 0 (read for spheres only) */
} rt_refraction_desc;

int rt_capi_refract_version(void);

/* rt_scene_create_textured with refractive objects */
int rt_scene_create_refractive(const rt_scene_desc *desc, int n_images, const rt_image_texture_desc *images,
                               int n_refractive, const rt_refraction_desc *refractive, int device, rt_scene **out);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_REFRACT_H_ */
