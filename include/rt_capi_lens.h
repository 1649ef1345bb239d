/*
 * rt_capi_lens.h -- depth of field: a thin-lens camera in place of the pinhole every other call uses.  Each pixel takes
 * n x n samples; sample s starts at its own point of the lens and passes through the point where the pinhole ray of its
 * sub-pixel meets the focal plane, so what lies on that plane is sharp and everything else blurs with its distance from it.
 * The rays are generated on the device, traced as ray batches (rt_capi_rays.h: the "lens cameras" that header names) and
 * averaged there; nothing but the frame crosses the bus.  Plain C99, versioned on its own (RT_CAPI_LENS_VERSION /
 * rt_capi_lens_version()); rt_capi.h and the other extension headers are unchanged.
 *
 * THE DEFINITION, which the GPU meets bit for bit.  All arithmetic is IEEE fp32, in the order written, without contraction.
 * H(x) is the 32-bit hash "lowbias32" of rt_capi_soft.h, and the map from the square to the disc (a, b -> u, v) is that
 * header's too.  For pixel (x, z) of the W x H frame, x the frame's (global) column, with n = samples:
 *
 *     S = n*n      g = focus - 1.0f      step = 2.0f / (float)n
 *     h = H(H(seed ^ 0x9e3779b9u) ^ (uint32)(x*H + z))      rot = h % S                        (uint32 arithmetic)
 *
 * and for sample s = i*n + j, i, j in [0, n):
 *
 *     P    = the pixel point of createEyeRay (src/Camera.cpp:71-84) at dx = (float)(n*x + i) / (float)(n*W) and
 *            dz = (float)(n*z + j) / (float)(n*H):
 *                sx = dx*screen_width - screen_halfwidth      sz = dz*screen_height - screen_halfheight
 *                P.c = (screen_origin.c + vector_horizontal.c*sx) + vector_vertical.c*sz
 *            (exactly rt_render_ssaa's arithmetic for pixel (n*x + i, n*z + j) of the virtual image, rt_capi_ssaa.h)
 *     T.c  = P.c + (P.c - E.c) * g                                                              (E = eye_origin)
 *     sp   = (s + rot) % S      li = sp / n      lj = sp % n        (the lens stratum: the sample order rotated per pixel)
 *     hs   = H(h ^ s)
 *     xi1  = (float)(hs >> 8) * 0x1p-24f              xi2 = (float)(H(hs ^ 0x9e3779b9u) >> 8) * 0x1p-24f
 *     a    = ((float)li + xi1)*step - 1.0f            b   = ((float)lj + xi2)*step - 1.0f
 *     u    = a*sqrtf(1.0f - (b*b)*0.5f)               v   = b*sqrtf(1.0f - (a*a)*0.5f)
 *     O.c  = E.c + (vector_horizontal.c*(aperture*u) + vector_vertical.c*(aperture*v))
 *            with aperture == 0:  O = E itself (it is not evaluated as E + 0, which could flip the sign of a zero)
 *     ray s = {O, T}      colour_s = the colour rt_trace_rays gives that ray at max_depth
 *
 *     out_rgb[p] = (((colour_0 + colour_1) + colour_2) + ... + colour_{S-1}) / (float)S     per channel, strictly in order of s
 *
 * with p = (x - x0)*H + z, three floats each (rt_render's layout).  rt_lens_rays* write ray s of pixel p at
 * out_rays[6*(p*S + s) .. +5] = {O.x, O.y, O.z, T.x, T.y, T.z}, whatever order the library traces them in.
 *
 * WHAT FOLLOWS.
 *   - The sampling key is the pixel's number in the whole frame: a strip equals the same columns of the frame bit for bit,
 *     and chunk_columns never changes a bit.  The key x*H + z is taken modulo 2^32: on a frame of more than 2^32 pixels the
 *     pixels 2^32 apart share their lens points (their targets still differ).
 *   - aperture = 0 and focus = 1: every ray is {E, P}, so the frame is rt_render_ssaa's for n = 1, 2, 4 and rt_render's for
 *     n = 1 -- for every camera whose screen_origin has no -0.0 component (rt_trace_rays reads a -0.0 of its target as +0.0,
 *     rt_capi_rays.h; the caveat rt_capi_adaptive.h carries).
 *   - aperture = 0 and focus != 1: the same rays aimed at a rescaled target; the frame agrees with rt_render_ssaa's up to
 *     rounding only.
 *   - The focal surface is the screen plane scaled by focus about the eye, a plane parallel to the screen: focus = d / d0
 *     puts it at distance d when the screen is at d0 from the eye.
 *   - The lens is the ellipse spanned by aperture*vector_horizontal and aperture*vector_vertical about the eye: a disc of
 *     radius aperture for orthonormal screen vectors.  Every sample counts 1 / S; each pixel's S samples occupy the S strata
 *     of the lens once each.
 *
 * SOFT-SHADOW SCENES (rt_scene_create_soft with at least one area light) are refused with RT_ERR_INVALID: a ray batch keys
 * its shadow samples by the ray index (rt_capi_soft.h), so the frame would change with chunk_columns (the reason
 * rt_capi_adaptive.h gives).  Image textures and refraction work unchanged.
 *
 * rt_lens_rays* are the ray generation alone: no scene, a device index, RT_ERR_NO_DEVICE without one (the conventions of
 * rt_denoise).  out_rays holds 6 (x1 - x0) H S floats.
 *
 * Argument checks, all before any device work, RT_ERR_INVALID in this order.  rt_render_lens*: (1) rt_render's, in
 * rt_render's order (the scene is NULL; W or H not positive, or not 0 <= x0 <= x1 <= W; out_rgb is NULL while the strip is
 * not empty; the camera is NULL; max_depth < 0; the strip's colours exceed rt_render's limit); (2) params is NULL;
 * (3) samples outside 1..8; (4) chunk_columns negative; (5) aperture negative, NaN or infinite; (6) focus NaN, infinite or
 * not > 0; (7) n*W or n*H not below 2^31; (8) one column's rays, H*S, beyond the ray-batch limit of 2^31 - 65; (9) for the
 * device variant, d_out_rgb not 4-byte aligned; (10) last, the scene has area lights.  rt_lens_rays*: the same list without
 * the scene, the depth and (10), out_rays in out_rgb's place, and in place of (8) the strip's rays: 6 (x1 - x0) H S floats
 * beyond rt_render's limit of 8e9; then RT_ERR_NO_DEVICE, or a device index out of range.  An empty strip (x0 == x1) is RT_OK
 * and launches nothing.
 *
 * NO HOST SYNCHRONISATION.  rt_render_lens_device and rt_lens_rays_device are enqueued on hip_stream and return; unlike
 * rt_render_adaptive_device nothing is read back, the launches depend on the arguments alone.  (Scratch that has to grow is
 * reallocated first, which waits for the device as any allocation does; a call that fits the handle's scratch, on the
 * stream of the handle's previous call, waits for nothing.  On another stream it first waits on the host for that previous
 * stream, as every call of a handle does: INTEGRATION.md section 4, "Streams".)
 *
 * SCRATCH lives in the scene handle and only grows: the rays and the sample colours of one chunk of columns, 36 S bytes a
 * pixel.  chunk_columns = 0 is the library's default: the most columns whose rays and sample colours stay within 256 MiB,
 * and at least one; no chunk_columns gives a launch more than 2^31 - 65 rays.  The host variant adds its output, 12 bytes a
 * pixel of the strip.  All offsets are 64-bit.
 *
 * Timing: rt_lens_info's three stage times are HIP-event times on the call's stream, summed over the chunks.
 * rt_get_timing().last_kernel_ms is their sum for as long as the lens call is the handle's last launch; launches and
 * sum_kernel_ms count the ray-batch launches as for any other call, and rt_get_launch_info() describes the call's last one
 * (a *_rays kernel).  The handle's lock is held for the whole call.  Speed-only options (rt_capi_tuning.h) apply as for
 * rt_trace_rays.
 *
 * Not provided: soft-shadow scenes, several GPUs, the counting build, importance-weighted or polygonal apertures, a jitter of
 * the sub-pixel positions (the targets are rt_render_ssaa's regular grid; only the lens points are hashed).
 *
 * rt_lens_info is 48 bytes: pixels at 0, rays at 8, chunks at 16, raygen_ms at 24, trace_ms at 32, resolve_ms at 40;
 * rt_lens_params is 20 bytes.
 */
#ifndef RT_CAPI_LENS_H_
#define RT_CAPI_LENS_H_

#include "rt_capi_rays.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_LENS_VERSION 1

typedef struct rt_lens_params {
    int32_t  samples;        /* n, 1..8: n x n samples per pixel                                          */
    int32_t  chunk_columns;  /* >= 0; most columns traced per launch, 0: library default; never changes   */
                             /* a result                                                                  */
    uint32_t seed;
    float    aperture;       /* lens radius in units of the screen vectors' length; finite, >= 0          */
    float    focus;          /* focal plane's distance as a multiple of the screen's; finite, > 0         */
} rt_lens_params;            /* 20 bytes */

typedef struct rt_lens_info {          /* of the scene's last rt_render_lens* call */
    int64_t pixels, rays;              /* strip pixels; rays traced (pixels * S) */
    int32_t chunks;                    /* chunks of columns the strip was traced in */
    double  raygen_ms, trace_ms, resolve_ms;   /* HIP events, summed over the chunks */
} rt_lens_info;                        /* 48 bytes */

int rt_capi_lens_version(void);

/* the rays alone; host memory, synchronous */
int rt_lens_rays(const rt_camera_desc *cam, int W, int H, int x0, int x1, const rt_lens_params *params, int device,
                 float *out_rays);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising;
 * d_out_rays 4-byte aligned */
int rt_lens_rays_device(const rt_camera_desc *cam, int W, int H, int x0, int x1, const rt_lens_params *params, int device,
                        void *d_out_rays, void *hip_stream);

/* host memory, synchronous (as rt_render): out_rgb holds 3 (x1 - x0) H floats */
int rt_render_lens(rt_scene *scene, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                   const rt_lens_params *params, float *out_rgb);

/* device memory on the scene's device, enqueued on hip_stream without synchronising (above) */
int rt_render_lens_device(rt_scene *scene, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                          const rt_lens_params *params, void *d_out_rgb, void *hip_stream);

/* the last rt_render_lens* call of the scene (all zero before the first); waits for that call's events */
int rt_get_lens_info(const rt_scene *scene, rt_lens_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_LENS_H_ */
