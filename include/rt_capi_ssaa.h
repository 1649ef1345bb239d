/*
 * rt_capi_ssaa.h -- anti-aliased frames: k x k supersampling, averaged inside
 * the render kernel.  Plain C99, versioned on its own (RT_CAPI_SSAA_VERSION /
 * rt_capi_ssaa_version()); the drop-in surface of rt_capi.h is unchanged.
 *
 * The reference takes one sample per pixel, at the pixel's corner:
 * dx = x / W, dz = z / H, then createEyeRay (src/RayTracer.cpp:916-918,
 * src/Camera.cpp:71-84).  With samples = k, output pixel (x, z) of a W x H
 * frame is defined as follows:
 *
 *   - sample (i, j), 0 <= i, j < k, is calculatePixel(createEyeRay(dx, dz), 0)
 *     with dx = (float)(k*x + i) / (float)(k*W), dz = (float)(k*z + j) / (float)(k*H),
 *     both in fp32: exactly pixel (k*x + i, k*z + j) of an rt_render(kW, kH) frame;
 *   - the samples are summed in fp32 in the order s = i*k + j, strictly
 *     sequentially (acc = S0; acc = acc + S1; ...), without contraction;
 *   - each channel is then divided by (float)(k*k) -- for k = 2, 4 the same as
 *     multiplying by 2^-2, 2^-4;
 *   - no clamp and no gamma: the reference has no final clamp, so values above
 *     1 stay.
 *
 * samples = 1 is rt_render / rt_render_device: the same kernel, the same bits.
 * samples = 2 or 4 run the sibling kernel over the virtual kW x kH image and
 * average each pixel's k x k samples in the wavefront before the one store per
 * output pixel; no buffer of k*k*W*H pixels exists anywhere.  Any other value
 * is RT_ERR_INVALID.
 *
 * Strips are in OUTPUT columns: [x0, x1) of the W x H image, and a strip is
 * bit-identical to the same columns of a whole frame.  The output layout is
 * rt_render's, at W x H: out_rgb[((x-x0)*H + z)*3 + c].  Error codes,
 * rt_last_error(), rt_get_timing() and rt_get_launch_info() (the kernel that
 * ran, its tile shape in virtual pixels) behave as for rt_render.  samples and
 * the virtual size (k*W, k*H, columns [k*x0, k*x1)) are checked before the
 * device is touched, by the rules rt_render applies to its arguments.
 * Speed-only options (rt_capi_tuning.h) apply as for rt_render; a tile shape
 * that cannot hold whole pixels (option "tile_z" below k or above 64 / k) is
 * replaced by the nearest one that can.
 */
#ifndef RT_CAPI_SSAA_H_
#define RT_CAPI_SSAA_H_

#include "rt_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_SSAA_VERSION 1

int rt_capi_ssaa_version(void);

/* host memory, synchronous (as rt_render) */
int rt_render_ssaa(rt_scene *scene, const rt_camera_desc *cam, int W, int H, int x0, int x1,
                   int max_depth, int samples, float *out_rgb);

/* device memory on the scene's device, enqueued on hip_stream (a hipStream_t; NULL = the null
 * stream) without synchronising (as rt_render_device) */
int rt_render_ssaa_device(rt_scene *scene, const rt_camera_desc *cam, int W, int H, int x0, int x1,
                          int max_depth, int samples, void *d_out_rgb, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_SSAA_H_ */
