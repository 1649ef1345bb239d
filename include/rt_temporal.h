/*
 * rt_temporal.h -- temporal accumulation: the noisy terms of a frame (soft shadows, rt_ambient_occlusion and
 * rt_indirect_diffuse at one or two samples, the gather at 1/s^2 density) are cheap at one sample a pixel, and every sampled call
 * takes a seed, so a caller who renders a sequence can draw other samples each frame.  This call combines those frames: it carries
 * last frame's accumulated value to this frame's pixels through the hit records, keeps it only where the records say it is still
 * the same surface, blends the new sample in, and keeps the first two moments of luminance so that a variance exists.  Plain C99,
 * versioned on its own (RT_CAPI_TEMPORAL_VERSION / rt_capi_temporal_version()); rt_capi.h and the other extension headers are
 * unchanged.  Like rt_denoise the calls take a device index and no scene; the rt_camera_desc of the previous frame is all the
 * motion information a static scene needs.
 *
 * LAYOUT.  pixels[x][z], z contiguous, as everywhere.  The CURRENT frame may be a strip, columns [x0, x1) of a W x H frame,
 * Wn = x1 - x0: cur[((x-x0)*H + z)*channels + c] and cur_hits[(x-x0)*H + z] (rt_hit, include/rt_capi_query.h, as rt_render_gbuffer
 * writes them).  The PREVIOUS frame is always whole, W x H: prev_hits[x*H + z], prev_value[(x*H + z)*channels + c],
 * prev_moments[(x*H + z)*2 + {0, 1}], prev_len[x*H + z], all fp32 -- the out_* of the previous call and the records it was given.
 * The outputs are the strip's: out_value (Wn H channels), out_moments (Wn H 2), out_len (Wn H), out_variance (Wn H floats; may be
 * NULL), out_flags (Wn H bytes; may be NULL).  prev_hits == NULL means "first frame": then prev_value, prev_moments, prev_len and
 * cam_prev must be NULL too, and with prev_hits given none of them may be.  No output may overlap a prev_* buffer -- a pixel's
 * taps are other pixels' history -- so a caller ping-pongs two sets.  out_value may be cur.
 *
 * DEFINITION.  The GPU result is bit-exact to this.  All arithmetic is IEEE fp32, one rounding per operation, no contraction, a
 * correctly rounded divide, in the order written; every comparison is written so that a NaN means "no history" or "skip" (a numpy
 * restatement needs where(t > 0, t, 0), not maximum).
 *   dot(a, b)   = (a.x*b.x + a.y*b.y) + a.z*b.z
 *   cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
 *   lum(c)      = (0.25f*c.r + 0.5f*c.g) + 0.25f*c.b for 3 channels, the value itself for 1
 * For pixel p = (x, z), x in [x0, x1): h = cur_hits[(x-x0)*H + z], c = cur[...], l = lum(c).
 *
 *   1. NO HISTORY: the first frame; or h is dead (h.object < 0 or h.flags & RT_HIT_LIGHT); or steps 2 to 4 end with nothing.
 *      Then out_value = c word for word, moments (l, l*l), len 1.0f, variance +0.0f, flag 1.
 *   2. IDENTITY: the 16 floats of cam_prev equal those of cam as BITS.  The only tap is cell (x, z) with bw = 1.0f; it still
 *      passes the tap tests of step 4.
 *   3. REPROJECTION, otherwise, with cam_prev's eye = eye_origin, so = screen_origin, hv = vector_horizontal, vv = vector_vertical:
 *        O = so - eye;  nh = cross(hv, vv);  na = cross(vv, O);  nb = cross(O, hv);  q = dot(O, nh)
 *        D = h.point - eye;  s = dot(D, nh).  No history unless s*q > 0.
 *        a = dot(D, na) / s;  b = dot(D, nb) / s
 *        px = ((a + screen_halfwidth) / screen_width) * (float)W;  pz = ((b + screen_halfheight) / screen_height) * (float)H
 *        No history unless px > -1 && px < (float)W && pz > -1 && pz < (float)H.
 *        i0 = floor(px), j0 = floor(pz);  fx = px - (float)i0, fz = pz - (float)j0   (the subtractions are exact)
 *        Taps, for a in 0..1, for b in 0..1, in this order: the cell is (i0+a, j0+b); skip it if it lies outside [0, W) x [0, H);
 *        bw = (a ? fx : 1.0f - fx) * (b ? fz : 1.0f - fz); skip unless bw > 0.
 *   4. TAP TESTS AND SUMS.  With g = prev_hits[cell], skip the tap unless all of
 *        g.object == h.object;  (g.flags & 3) == (h.flags & 3)
 *        with match_color: the three colour words of g and h are equal as BITS
 *        dot(h.normal, g.normal) >= normal_cos
 *        with plane_eps > 0: e = g.point - h.point (per component), d = dot(e, h.normal), and d*d <= plane_eps*plane_eps
 *      For a tap that passes, starting from acc = 0 and wsum = 0: acc.k = acc.k + bw * prev.k[cell] for every history word k (the
 *      channels of prev_value, m1 and m2 of prev_moments, len) and wsum = wsum + bw.  The history words of a tap that does not
 *      pass are never read.  If wsum > 0 is false there is no history.
 *   5. BLEND.  hk = acc.k / wsum.  N = hlen + 1.0f; if (!(N <= (float)max_history)) N = (float)max_history.
 *        ac = 1.0f / N; if (!(ac >= alpha)) ac = alpha.  am likewise from alpha_moments.
 *        out_value.c = hc + ac * (c - hc) per channel;  m1 = hm1 + am * (l - hm1);  m2 = hm2 + am * (l*l - hm2);  len = N
 *        v = m2 - m1*m1; variance = v > 0 ? v : +0.0f;  flag 0.
 *
 * WHAT FOLLOWS.  With equal cameras and alpha = 0, frame k is the running mean of frames 1..k up to max_history frames, and an
 * exponential average with weight 1 / max_history after.  A pixel whose history equals its sample keeps its bits (finite values;
 * -0.0 becomes +0.0).  A strip equals the frame's columns, because the previous frame is always whole.  The variance is that of
 * the luminance samples the history has seen, not of their mean; it is 0 while len is 1.
 *
 * Not provided: history behind glass (the record is the pane's; for mirrors, include/rt_mirror.h makes the guide records),
 * supersampled frames (they have no records), several GPUs, the counting build.  The spatial variance estimate for short
 * histories and the variance-steered filter are include/rt_svgf.h.  Objects that move between the frames (these records carry no
 * motion) are include/rt_motion.h: the same calls with one rigid motion per object.  History that went stale on a surface that
 * stayed (a shadow moved, a light changed) is clipped by include/rt_clamp.h, a call of its own after this one.
 *
 * ERRORS.  Int codes and rt_last_error() as everywhere.  All argument checks come before any device work, RT_ERR_INVALID in this
 * order: params is NULL; channels not 1 or 3; match_color not 0 or 1; max_history outside 1..65535; normal_cos NaN or outside
 * -1..1; plane_eps negative, NaN or infinite; alpha, then alpha_moments, NaN or outside 0..1; W or H not positive; x0 < 0, x1 > W
 * or x0 >= x1; W * H > 533 333 333 pixels (rt_render_gbuffer's limit); cam, cur, cur_hits, out_value, out_moments or out_len NULL,
 * then the first-frame rule above; for the device variant, records not 16-byte aligned, then floats not 4-byte aligned, then an
 * output overlapping a prev_* buffer.  Then, without a HIP device, RT_ERR_NO_DEVICE; a device index out of range is
 * RT_ERR_INVALID.  Every offset is 64-bit, and a frame of any admitted shape is one launch.
 */
#ifndef RT_TEMPORAL_H_
#define RT_TEMPORAL_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_TEMPORAL_VERSION 1

typedef struct rt_temporal_params {
    int32_t channels;        /* 1 or 3 */
    int32_t match_color;     /* 0 / 1: a tap must carry the pixel's colour words, as bits */
    int32_t max_history;     /* 1..65535: cap of the history length */
    float   normal_cos;      /* finite, -1..1: a tap needs n_p . n_q >= normal_cos */
    float   plane_eps;       /* finite, >= 0; 0: no plane test */
    float   alpha;           /* finite, 0..1: floor of the colour blend weight */
    float   alpha_moments;   /* finite, 0..1: floor of the moments' blend weight */
} rt_temporal_params;        /* 28 bytes */

int rt_capi_temporal_version(void);

/* host memory, synchronous.  kernel_ms may be NULL; otherwise it receives the time between HIP events around the kernel, without
 * the copies. */
int rt_temporal_accumulate(int device, const rt_temporal_params *params, const rt_camera_desc *cam_prev, const rt_camera_desc *cam,
                           int W, int H, int x0, int x1, const float *cur, const rt_hit *cur_hits, const rt_hit *prev_hits,
                           const float *prev_value, const float *prev_moments, const float *prev_len, float *out_value,
                           float *out_moments, float *out_len, float *out_variance, uint8_t *out_flags, double *kernel_ms);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream): enqueues only, allocates nothing and
 * never synchronises.  The cameras and params are read before the call returns; the buffers stay valid until the stream has
 * drained.  Records 16-byte aligned, floats 4-byte aligned. */
int rt_temporal_accumulate_device(int device, const rt_temporal_params *params, const rt_camera_desc *cam_prev,
                                  const rt_camera_desc *cam, int W, int H, int x0, int x1, const void *d_cur, const void *d_cur_hits,
                                  const void *d_prev_hits, const void *d_prev_value, const void *d_prev_moments,
                                  const void *d_prev_len, void *d_out_value, void *d_out_moments, void *d_out_len,
                                  void *d_out_variance, void *d_out_flags, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_TEMPORAL_H_ */
