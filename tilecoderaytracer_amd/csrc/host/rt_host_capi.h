/*
 * rt_host_capi.h -- C glue over the C++ host model (celio_model.hpp) so that
 * Python (tests, bench.py) can build scenes with the reference's API calls and
 * obtain the flattened rt_scene_desc / rt_camera_desc.  This is NOT the
 * drop-in boundary (that is include/rt_capi.h); it is how non-C++ callers
 * reach the host side that sits above it.  All functions return 0 on success
 * unless stated otherwise.
 */
#ifndef RT_HOST_CAPI_H_
#define RT_HOST_CAPI_H_

#include "../../../include/rt_capi.h"
#include "../../../include/rt_capi_texture.h"
#include "../../../include/rt_capi_refract.h"
#include "../../../include/rt_capi_soft.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rth_scene rth_scene;   /* a Scene + a Camera + their flattened form */

int  rth_scene_new(rth_scene **out);                     /* empty Scene(), default Camera() */
int  rth_scene_builtin(rth_scene **out);                 /* Scene::initialize()             */
int  rth_scene_two_mirrors(rth_scene **out);             /* Scene::initializeTwoMirrors()   */
int  rth_scene_grid(int n, int shadows, rth_scene **out);/* build_grid_scene()              */
void rth_scene_free(rth_scene *s);

/* primitive constructors + addObject(); return the object's index, or -1 */
int rth_add_sphere(rth_scene *s, const float origin[3], float radius);
int rth_add_infinite_plane(rth_scene *s, const float o[3], const float n[3], const float h[3]);
int rth_add_finite_plane_corners(rth_scene *s, const float o[3], const float vcorner[3], const float hcorner[3]);
int rth_add_finite_plane_axes(rth_scene *s, const float o[3], const float n[3], const float h[3],
                              float v_dist, float h_dist);
int rth_object_count(const rth_scene *s);

/* getObject(idx)->... setters */
int rth_set_color(rth_scene *s, int idx, const float rgb[3]);
int rth_set_diffuse(rth_scene *s, int idx, float f);
int rth_set_specular(rth_scene *s, int idx, float f);
int rth_set_reflective(rth_scene *s, int idx, float f);
/* ObjMaterial::setRefractiveFactor and setRefractiveIndex (include/rt_capi_refract.h) */
int rth_set_refraction(rth_scene *s, int idx, float factor, float ior);
/* SceneObject::setAreaLight (include/rt_capi_soft.h): n x n samples on a disc of the radius (< 0: the object's own) */
int rth_set_area_light(rth_scene *s, int idx, int samples, float radius);
int rth_set_checkerboard(rth_scene *s, int idx, const float light[3], const float dark[3], float w, float h);
/* a Texture_Image (include/rt_capi_texture.h): texels_w x texels_h fp32 rgb texels, copied; 1 on a bad argument */
int rth_set_image_texture(rth_scene *s, int idx, int texels_w, int texels_h, const float *texels, float w, float h, int wrap);
int rth_set_light(rth_scene *s, int idx);
int rth_set_intensity(rth_scene *s, int idx, float f);
int rth_set_object_indices(rth_scene *s, int my_rank, int group_size);   /* Scene::SetObjectIndices */
int rth_camera_two_mirrors(rth_scene *s);                                /* Camera::setSceneTwoMirrors */
int rth_camera_eye_ray(const rth_scene *s, float dx, float dy, float origin[3], float dir[3]);

/* flattened views; valid until the scene is modified or freed */
const rt_scene_desc  *rth_scene_desc(rth_scene *s);
const rt_camera_desc *rth_camera_desc(rth_scene *s);
/* the flattened scene's images (texture indices n_textures + k): their count, *images set to the array (NULL if none) */
int rth_scene_images(rth_scene *s, const rt_image_texture_desc **images);
/* the flattened scene's refractive objects: their count, *refractions set to the array (NULL if none) */
int rth_scene_refractions(rth_scene *s, const rt_refraction_desc **refractions);
/* the flattened scene's area lights: their count, *area_lights set to the array (NULL if none) */
int rth_scene_area_lights(rth_scene *s, const rt_area_light_desc **area_lights);

/* byte-exact raytracer_screen.txt (src/RayTracer.cpp:2022-2061, 1574-1626) */
int rth_write_screen_txt(const char *path, int W, int H, const float *rgb,
                         double run_time_s, double us_per_pixel);
/* the same with CORE_NUM = n_cores in the header (one "core" per GPU; > 1 writes the static
 * partition's label, src/RayTracer.cpp:2037-2058) */
int rth_write_screen_txt_cores(const char *path, int W, int H, const float *rgb,
                               double run_time_s, double us_per_pixel, int n_cores);
/* screen_ppm.hpp: a binary PPM of H rows of 3 W bytes, pitch_bytes apart in memory (0 ok / 1 error) */
int rth_write_screen_ppm(const char *path, int W, int H, const uint8_t *rows, uint64_t pitch_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RT_HOST_CAPI_H_ */
