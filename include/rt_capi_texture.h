/*
 * rt_capi_texture.h -- image textures for planes: a bitmap the reference's ObjTexture::getTexturePixel(x, y) would return
 * texel by texel (src/ObjTexture.h:31), sampled inside every render kernel.  Plain C99, versioned on its own
 * (RT_CAPI_TEXTURE_VERSION / rt_capi_texture_version()); rt_capi.h and the other extension headers are unchanged.
 *
 * TEXTURE INDICES.  rt_scene_create_textured(desc, n_images, images, ...) takes desc as rt_scene_create does and n_images
 * images beside it.  An object's `texture` keeps its meanings -- -1 none, [0, n_textures) a checkerboard -- and an index in
 * [n_textures, n_textures + n_images) is image texture - n_textures.  rt_scene_create still rejects such indices.  With
 * n_images == 0 the call is rt_scene_create: the same tables, the same kernels, the same pixels.
 *
 * WHICH OBJECTS.  As in the reference, only planes (infinite and finite) sample a texture; a sphere's texture is ignored.
 *
 * TEXTURE COORDINATES.  The checkerboard's: x = PO . horizontal, y = PO . vertical, PO = ip - the plane's texture origin
 * (SceneObject::origin of an infinite plane, plane_origin of a finite one), ip the hit point before the 1e-3 offset along the
 * normal (src/SceneInfinitePlane.cpp:57-95, src/SceneFinitePlane.cpp:128-131).
 *
 * FOLD.  (x, y) into one copy of the image, in fp32; x with w = width, y the same way with height:
 *   RT_TEX_WRAP_CHECKER  Texture_CheckerBoard::getTexturePixel's fold: x >= 0 ? fmodf(x, w) : fmodf(fmodf(-x, w) + w / 2, w)
 *   RT_TEX_WRAP_REPEAT   r = fmodf(x, w); x' = r < 0 ? r + w : r
 *   RT_TEX_WRAP_CLAMP    x' = x; if x' < 0 then x' = 0; if x' > w then x' = w  (a NaN passes unchanged)
 * TEXEL.  With b_k = fl(fl(w k) / texels_w), the column is i = (texels_w - 1) - #{k in [1, texels_w) : x' < b_k} -- for a
 * finite x' the largest i with b_i <= x'; a NaN gives the last column -- and the row j likewise from y', height and texels_h.
 * The hit's colour is texels[(j * texels_w + i) * 3 + 0..2], used wherever the reference uses the collision's getColor():
 * object_color in cosine and specular shading, the reflection combine final = local + (rf * child) * colour, a textured
 * light's intensity * colour, and rt_hit.color of the ray queries (rt_capi_query.h) and of the G-buffer
 * (rt_capi_gbuffer.h).  Shadows do not change.
 *
 * Two consequences:
 *   - a 2 x 2 image with RT_TEX_WRAP_CHECKER, texels (0,0) light, (1,0) dark, (0,1) dark, (1,1) light, and the checkerboard's
 *     width and height reproduces the checkerboard bit for bit (b_1 = fl(w / 2), the checkerboard's own threshold);
 *   - an image whose texels all equal c reproduces an untextured plane of colour c bit for bit.
 *
 * ERRORS.  All before any device work, in this order.  RT_ERR_INVALID: desc or out is NULL; n_images < 0; images is NULL
 * while n_images > 0; then image by image: texels is NULL, texels_w or texels_h < 1, width or height not finite and > 0, an
 * unknown wrap.  RT_ERR_CAPACITY: more than RT_MAX_SCENE_TEXELS texels in all the images together (one 1024 x 1024 image
 * fits).  Then rt_scene_create's checks of desc, with texture indices allowed up to n_textures + n_images - 1.
 *
 * CALLS.  On a scene with images, bit-exact to the definition above: rt_render / _device, rt_render_ssaa / _device,
 * rt_trace_rays / _device, rt_intersect_rays / _device, rt_occluded_rays / _device (no colour involved), rt_render_gbuffer /
 * _device, and the speed-only options of rt_set_option.  When a plane references an image, rt_get_launch_info() names the
 * *_image sibling of the kernel the same call runs on a scene without images, and every checkerboard is sampled as its
 * 2 x 2 CHECKER image (the same pixels); otherwise the scene is rt_scene_create's.  The texels are copied at create: the
 * caller's array may go at once.
 *
 * Not provided: the counting build -- rt_render_stats, and rt_learn_tile_order, which renders with it, return RT_ERR_INVALID
 * on a scene that references an image -- and the multi-GPU path (rt_multi_*, rt_render_multi), which takes no images.
 * Filtering (bilinear, mipmaps), textures on spheres and 8-bit texel formats are not offered.
 */
#ifndef RT_CAPI_TEXTURE_H_
#define RT_CAPI_TEXTURE_H_

#include "rt_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_TEXTURE_VERSION 1

/* texels per scene, all images together: 2^20 (the bounce stack keeps a texel's index in 20 bits) */
#define RT_MAX_SCENE_TEXELS 1048576

enum { RT_TEX_WRAP_CHECKER = 0, RT_TEX_WRAP_REPEAT = 1, RT_TEX_WRAP_CLAMP = 2 };

typedef struct rt_image_texture_desc {
    int32_t      texels_w, texels_h;   /* >= 1 */
    float        width, height;        /* world size of one copy of the image: ObjTexture::width / height, > 0, finite */
    int32_t      wrap;                 /* RT_TEX_WRAP_* */
    const float *texels;               /* host, fp32 rgb, texel (i, j) at texels[(j * texels_w + i) * 3 + c]; copied */
} rt_image_texture_desc;

int rt_capi_texture_version(void);

/* rt_scene_create with images: texture index n_textures + k is images[k] */
int rt_scene_create_textured(const rt_scene_desc *desc, int n_images, const rt_image_texture_desc *images, int device,
                             rt_scene **out);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_TEXTURE_H_ */
