/*
 * rt_capi_adaptive.h -- the cheap way to an anti-aliased frame: one sample per pixel everywhere, then k x k samples for the
 * pixels an edge passes through and for no others.  A first pass renders the strip's colours and hit records
 * (rt_render_gbuffer), a flag pass compares each pixel with the other corners of its footprint, and only the flagged pixels
 * are traced again, as ray batches (rt_trace_rays), and averaged as rt_capi_ssaa.h defines.  Plain C99, versioned on its own
 * (RT_CAPI_ADAPTIVE_VERSION / rt_capi_adaptive_version()); rt_capi.h and the other extension headers are unchanged.
 *
 * THE DEFINITION, which the GPU meets bit for bit.  All arithmetic is IEEE fp32, in the order written, without contraction.
 *
 * FLAGS of a rectangle of Wn x H pixels in pixels[x][z] order (pixel (x, z) is element p = x*H + z), from its colours rgb
 * and its records hits.  For pixels p and q
 *
 *   differ(p, q) = 1  if hits[p].object != hits[q].object
 *                = 1  if hits[p].object >= 0 and !(t >= normal_cos),
 *                         t = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z          (n = hits[].normal)
 *                = 1  if for any channel c:  !(fabsf(rgb[p].c - rgb[q].c) <= color_threshold)
 *                = 0  otherwise
 *   flag[p] = flag_all || differ(p, (x+1, z)) || differ(p, (x, z+1)) || differ(p, (x+1, z+1))
 *
 * Only neighbours inside the rectangle exist: the last column has no (x+1, .), the last row no (., z+1).  Every comparison
 * is written so that a NaN flags the pixel: a NaN normal component, a NaN colour, and inf - inf among them.  Two misses
 * (object -1 both) are compared by their colours alone.
 *
 * Why these three neighbours.  The reference samples a pixel at its CORNER (rt_capi_ssaa.h): pixel (x, z) is the ray through
 * (x / W, z / H), and its k x k samples cover [x, x+1) x [z, z+1).  The three neighbours are the other corners of that
 * footprint.  An edge that runs between the samples of x and x+1 therefore runs through pixel x's footprint and not through
 * pixel x+1's: it is pixel x that gains from more samples, and the test looks right and up only, never left or down.
 *
 * FRAME.  For columns [x0, x1) of a W x H frame of cam with recursion limit max_depth:
 *   first    is rt_render_gbuffer of columns [x0, min(x1 + 1, W)): one halo column on the right where the frame has one;
 *   flags    are the FLAGS of that rectangle, cropped to its first x1 - x0 columns;
 *   out_rgb[p] = flag[p] && samples > 1 ? A(p) : first.rgb[p],      p = (x - x0)*H + z, three floats each (rt_render's layout);
 *   out_flags[p] = flag[p], one byte each, 0 or 1 (out_flags may be NULL).
 * A(p) is rt_capi_ssaa.h's average with k = samples: sample (i, j) is the colour rt_trace_rays gives for the ray
 * {eye_origin, pixel point}, the pixel point built in createEyeRay's arithmetic with dx = (float)(k*x + i) / (float)(k*W) and
 * dz = (float)(k*z + j) / (float)(k*H); the samples are summed strictly in the order s = i*k + j, then each channel is divided
 * by (float)(k*k).
 *
 * So the frame is where(flags, rt_render_ssaa, rt_render) bit for bit, for every camera whose screen_origin has no -0.0
 * component.  With a -0.0 there, rt_trace_rays' documented reading of its target applies to the refined pixels
 * (rt_capi_rays.h: a -0.0 of the target is read as +0.0); a pixel point can only be -0.0 if screen_origin is.  With
 * samples = 1 the frame is rt_render's and the flags are still reported; with flag_all = 1 it is rt_render_ssaa's.  A strip
 * equals the same columns of the whole frame, in both outputs: that is what the halo column is for.  chunk_pixels never
 * changes a result.  Every one of the k x k samples of a flagged pixel is traced (sample (0, 0) is not taken from the first
 * pass), so rt_adaptive_info.rays = flagged * k * k.
 *
 * rt_adaptive_flags* are the flag pass alone, on a caller's rectangle: no scene, a device index, RT_ERR_NO_DEVICE without
 * one (the conventions of rt_denoise).  rgb holds 3 Wn H floats, hits Wn H records, out_flags Wn H bytes.
 *
 * SOFT-SHADOW SCENES (rt_scene_create_soft with at least one area light) are refused with RT_ERR_INVALID: their sampling
 * key is the pixel number in camera launches and the ray index in ray batches (rt_capi_soft.h), so a refined pixel would not
 * be rt_render_ssaa's and would change with chunk_pixels.  Image textures and refraction work unchanged.
 *
 * Argument checks, all before any device work, RT_ERR_INVALID in this order.  rt_render_adaptive*: rt_render's, in
 * rt_render's order (the scene is NULL; W or H not positive, or not 0 <= x0 <= x1 <= W; out_rgb is NULL while the strip is
 * not empty; the camera is NULL; max_depth < 0; the strip's colours exceed rt_render's limit); params is NULL; samples not
 * 1, 2 or 4; flag_all not 0 or 1; chunk_pixels negative; color_threshold negative, NaN or infinite; normal_cos NaN or outside
 * [-1, 1]; for samples > 1 the virtual size by rt_render_ssaa's rule (samples * W and samples * H below 2^31, the virtual
 * strip within rt_render's limit); the strip plus its halo column beyond rt_render_gbuffer's limit (533 333 333 pixels); for
 * the device variant, d_out_rgb not 4-byte aligned; last, the scene has area lights.  rt_adaptive_flags*: params is NULL;
 * the params' checks as above (samples, flag_all, chunk_pixels, color_threshold, normal_cos); Wn or H not positive; the
 * rectangle beyond 533 333 333 pixels; rgb, hits or out_flags is NULL; for the device variant, d_hits not 16-byte or d_rgb
 * not 4-byte aligned; then RT_ERR_NO_DEVICE, or a device index out of range.  An empty strip (x0 == x1) is RT_OK and launches
 * nothing.
 *
 * THE DEVICE VARIANT SYNCHRONISES hip_stream ONCE.  The number of flagged pixels decides the launches of the second pass,
 * and the host reads it, four bytes through pinned memory, after the flag pass.  rt_render_adaptive_device therefore cannot
 * be captured into a graph (hipGraph, torch.cuda.graph).  Everything else is enqueued: when the call returns, the second
 * pass may still be running on hip_stream.  rt_adaptive_flags_device is enqueued without synchronising.  (Besides: scratch
 * that has to grow is reallocated first, which waits for the device; and a call on another stream than the handle's previous
 * call first waits on the host for that previous stream, as every call of a handle does: INTEGRATION.md section 4, "Streams".)
 *
 * SCRATCH lives in the scene handle and only grows: the first pass's colours and records (60 bytes a pixel of the strip and
 * its halo; a strip that ends at the frame's right edge has no halo and renders its colours straight into the output, 48
 * bytes a pixel), the flags, the per-block counts and the list (5 bytes a pixel and a little), and the rays and sample
 * colours of at most chunk_pixels flagged pixels (36 k^2 bytes each).  chunk_pixels = 0 is the library's default: the most
 * pixels whose rays and sample colours stay within 256 MiB -- 1 864 135 pixels for k = 2, 466 033 for k = 4 -- and no
 * chunk_pixels gives a launch more than 2^26 pixels.  A 4096 x 4096 frame holds about 1 GB for the first pass (0.8 GB as a
 * whole frame, 1.0 GB as a strip with a halo) and 0.1 GB for the flags and the list; the host variant adds its outputs, 13
 * bytes a pixel.
 *
 * Timing: rt_adaptive_info's four stage times are HIP-event times on the call's stream (flag_ms: the flag, scan and list
 * kernels; trace_ms: ray generation and the ray-batch launches; resolve_ms: the averages).  rt_get_timing().last_kernel_ms is
 * their sum for as long as the adaptive call is the handle's last launch; launches and sum_kernel_ms count the render-kernel
 * launches (the first pass and one per chunk) as for any other call, and rt_get_launch_info() describes the call's last
 * render-kernel launch.  The handle's lock is held for the whole call.  Speed-only options (rt_capi_tuning.h) apply to the
 * first pass as for rt_render_gbuffer and to the second as for rt_trace_rays.
 *
 * Not provided: soft-shadow scenes (giving ray batches a caller's sampling key means changing the render kernels), several
 * GPUs, the counting build, returning the first pass's records, growing the flagged set (dilation, a second refinement).
 */
#ifndef RT_CAPI_ADAPTIVE_H_
#define RT_CAPI_ADAPTIVE_H_

#include "rt_capi_gbuffer.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_ADAPTIVE_VERSION 1

typedef struct rt_adaptive_params {
    int32_t samples;          /* 1, 2 or 4 (k); 1: first pass only, flags still reported            */
    int32_t flag_all;         /* 0 / 1; 1: every pixel is refined (the frame is rt_render_ssaa's)   */
    int32_t chunk_pixels;     /* >= 0; most flagged pixels traced per launch, 0: library default;   */
                              /* never changes a result                                             */
    float   color_threshold;  /* finite, >= 0; suggested 1/32                                       */
    float   normal_cos;       /* in [-1, 1]; suggested 0.9                                          */
} rt_adaptive_params;

typedef struct rt_adaptive_info {      /* of the scene's last rt_render_adaptive* call */
    int64_t pixels, flagged, rays;     /* strip pixels; of them refined; rays traced in the second pass */
    int32_t chunks;
    double  first_pass_ms, flag_ms, trace_ms, resolve_ms;   /* HIP events */
} rt_adaptive_info;

int rt_capi_adaptive_version(void);

/* the flag pass alone; host memory, synchronous */
int rt_adaptive_flags(int device, const rt_adaptive_params *params, int Wn, int H, const float *rgb, const rt_hit *hits,
                      uint8_t *out_flags);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream) without synchronising;
 * d_hits 16-byte aligned, d_rgb 4-byte aligned */
int rt_adaptive_flags_device(int device, const rt_adaptive_params *params, int Wn, int H, const void *d_rgb, const void *d_hits,
                             void *d_out_flags, void *hip_stream);

/* host memory, synchronous (as rt_render): out_rgb holds 3 (x1 - x0) H floats, out_flags (x1 - x0) H bytes or is NULL */
int rt_render_adaptive(rt_scene *scene, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                       const rt_adaptive_params *params, float *out_rgb, uint8_t *out_flags /* may be NULL */);

/* device memory on the scene's device, on hip_stream, which is synchronised once (above) */
int rt_render_adaptive_device(rt_scene *scene, const rt_camera_desc *cam, int W, int H, int x0, int x1, int max_depth,
                              const rt_adaptive_params *params, void *d_out_rgb, void *d_out_flags /* may be NULL */,
                              void *hip_stream);

/* the last rt_render_adaptive* call of the scene (all zero before the first); waits for that call's events */
int rt_get_adaptive_info(const rt_scene *scene, rt_adaptive_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_ADAPTIVE_H_ */
