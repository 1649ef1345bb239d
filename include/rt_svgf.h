/*
 * rt_svgf.h -- the last stage of the sampled pipeline: a spatial filter for the frames rt_temporal_accumulate (include/
 * rt_temporal.h) combines, steered by the variance that call carries.  rt_denoise (include/rt_capi_denoise.h) takes one
 * sigma_color for the whole frame; here the colour term's tolerance is each pixel's own luminance variance, so a region the
 * history has already cleaned is left alone and a noisy one is smoothed, and where the history is too short for its moments to
 * mean anything the variance is estimated from the neighbours' moments instead.  The pipeline is G-buffer, sampled term,
 * rt_temporal_accumulate, this filter, rt_encode_image.  Plain C99, versioned on its own (RT_CAPI_SVGF_VERSION /
 * rt_capi_svgf_version()); rt_capi.h and the other extension headers are unchanged.  Like rt_denoise the calls take a device
 * index and no scene.
 *
 * INPUT.  What rt_temporal_accumulate writes for a rectangle of Wn x H pixels in pixels[x][z] order (z contiguous):
 * value[(x*H + z)*channels + c], hits[x*H + z] (rt_hit, include/rt_capi_query.h), moments[(x*H + z)*2 + {0, 1}] and len[x*H + z],
 * all fp32.  The rectangle is a whole frame or a strip; as in rt_denoise, taps outside it do not exist.  The outputs are
 * out_value (Wn H channels), out_variance (Wn H; may be NULL) and out_estimate (Wn H; may be NULL).
 *
 * DEFINITION.  The GPU result is bit-exact to this.  All arithmetic is IEEE fp32, one rounding per operation, no contraction, a
 * correctly rounded divide, in the order written; every comparison is written so that a NaN means "skip" (a numpy restatement
 * needs where(t > 0, t, 0), not maximum).
 *   lum(c)    = (0.25f*c.r + 0.5f*c.g) + 0.25f*c.b for 3 channels, the value itself for 1
 *   dead(p)   : hits[p].object < 0 or hits[p].flags & RT_HIT_LIGHT
 *   key(p, q) : hits[q].object == hits[p].object, (hits[q].flags & 3) == (hits[p].flags & 3) and, with match_color, the three
 *               colour words of hits[q] and hits[p] equal as BITS
 *   geo(p, q) : t = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z;  wn = t > 0 ? t : 0;  normal_squarings times: wn = wn*wn
 *               with sigma_plane > 0 and invp = 1.0f / (sigma_plane*sigma_plane):  e = point_q - point_p (per component),
 *               d = (e.x*n_p.x + e.y*n_p.y) + e.z*n_p.z,  u = 1.0f - (d*d)*invp,  wn = wn * (u > 0 ? u : 0)
 *               (rt_upsample_guided's plane term).  The result is wn.
 * With m1 = moments[p*2], m2 = moments[p*2 + 1], r = spatial_radius, for pixel p = (x, z):
 *
 *   A. THE ESTIMATE var0[p].  If dead(p), var0 = +0.0f.  Otherwise vt = m2 - m1*m1; vt = vt > 0 ? vt : +0.0f.
 *      If len[p] >= (float)min_history, var0 = vt.  Otherwise, from a1 = a2 = ws = 0,
 *        for a in -r..r (x offset), for b in -r..r (z offset), in this order, q = (x+a, z+b) inside the rectangle:
 *            w = geo(p, q); skip unless key(p, q) and w > 0
 *            a1 = a1 + w*m1[q];  a2 = a2 + w*m2[q];  ws = ws + w
 *        if ws > 0:  s1 = a1/ws;  s2 = a2/ws;  vs = s2 - s1*s1;  vs = vs > 0 ? vs : +0.0f
 *                    k = (float)min_history / len[p];  if (!(k >= 1.0f)) k = 1.0f;  var0 = vs*k
 *        otherwise   var0 = vt
 *      out_estimate, where given, receives var0.
 *
 *   B. ITERATIONS i = 0 .. iterations-1, step s = 1 << i, each over (in, vin): iteration 0 reads (value, var0), each later one
 *      the complete output of the one before it.  With h = {1/16, 1/4, 3/8, 1/4, 1/16} (rt_denoise's B3 spline) and
 *      g = {1/4, 1/2, 1/4}:
 *        if dead(p): out[p] = in[p] and vout[p] = vin[p], bit for bit.  Otherwise
 *        gv = gs = 0;  for a in -1..1, for b in -1..1, in this order, q = (x+a, z+b) inside the rectangle (UNIT step, no key test):
 *            gv = gv + (g[a+1]*g[b+1]) * vin[q];  gs = gs + g[a+1]*g[b+1]
 *        vf = gv / gs                                   (inside the frame gs is exactly 1)
 *        if sigma_l > 0:  invl = 1.0f / ((sigma_l*sigma_l) * vf + epsilon)        (sigma_l*sigma_l is one fp32 product)
 *        acc = 0; vacc = 0; wsum = 0
 *        for a in -2..2, for b in -2..2, in this order, q = (x + a*s, z + b*s) inside the rectangle:
 *            skip unless key(p, q)
 *            w = (h[a+2]*h[b+2]) * geo(p, q)
 *            if sigma_l > 0:  d = lum(in[q]) - lum(in[p]);  u = 1.0f - (d*d)*invl;  w = w * (u > 0 ? u : 0)
 *            skip unless w > 0
 *            acc.c = acc.c + w*in[q].c per channel;  vacc = vacc + (w*w)*vin[q];  wsum = wsum + w
 *        if wsum > 0:  out.c = acc.c / wsum;  vout = vacc / (wsum*wsum).  Otherwise out = in and vout = vin.
 *      The last iteration's out is out_value and its vout is out_variance.
 *
 * The luminance term is rt_denoise's compact quadratic with the tolerance taken from the pixel's own variance: no exp and no sqrt,
 * so the result can be bit-exact.  A NaN anywhere in a weight drops the tap and never spreads through a weight; a NaN value or
 * variance spreads only as in[q] or vin[q] of a tap whose weight is positive.
 *
 * WHAT FOLLOWS.  With sigma_l = 0, sigma_plane = 0, match_color = 1 and 3 channels, on records without inside hits, out_value is
 * rt_denoise's at sigma_color = 0 bit for bit.  A strip filtered alone differs from the frame's columns only within
 * spatial_radius + 2 * (2^iterations - 1) columns of its edges.  On a flat interior region with constant input variance v and
 * sigma_l = 0 one iteration gives v * (35/128)^2 up to rounding (the sum of the squared B3 weights is (35/128)^2).
 *
 * Not provided: feeding the first iteration's output back into the history, moving objects, refracted content (the record is
 * the pane's; for mirrors, include/rt_mirror.h makes the guide records), several GPUs, the counting build, supersampled frames
 * (they have no records).
 *
 * ERRORS.  Int codes and rt_last_error() as everywhere.  All argument checks come before any device work, RT_ERR_INVALID in this
 * order: params is NULL; channels not 1 or 3; iterations outside 1..5; normal_squarings outside 0..6; match_color not 0 or 1;
 * min_history outside 1..65535; spatial_radius outside 1..3; sigma_l, then sigma_plane, negative, NaN or infinite; epsilon not
 * finite or not > 0; Wn or H not positive; Wn * H > 533 333 333 pixels (rt_render_gbuffer's limit); a NULL required buffer (value,
 * hits, moments, len, out_value; for the device variant also d_scratch); for the device variant, records or scratch not 16-byte
 * aligned, then floats not 4-byte aligned, then an output overlapping an input, another output or the scratch.  Then, without a
 * HIP device, RT_ERR_NO_DEVICE; a device index out of range is RT_ERR_INVALID.  rt_svgf_scratch_bytes returns 0 for arguments the
 * other calls refuse.  Every offset is 64-bit.
 */
#ifndef RT_SVGF_H_
#define RT_SVGF_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_SVGF_VERSION 1

typedef struct rt_svgf_params {
    int32_t channels;          /* 1 or 3 */
    int32_t iterations;        /* 1..5: steps 1, 2, 4, 8, 16 */
    int32_t normal_squarings;  /* 0..6 */
    int32_t match_color;       /* 0 / 1: a tap must carry the pixel's colour words, as bits */
    int32_t min_history;       /* 1..65535: below this length the variance is estimated spatially */
    int32_t spatial_radius;    /* 1..3: that estimate's window is (2r+1)^2 */
    float   sigma_l;           /* finite, >= 0; 0: no luminance term */
    float   sigma_plane;       /* finite, >= 0; 0: no plane term */
    float   epsilon;           /* finite, > 0: added to sigma_l^2 * variance */
} rt_svgf_params;              /* 36 bytes */

int rt_capi_svgf_version(void);

/* host memory, synchronous.  out_value may be value; out_variance and out_estimate may be NULL.  kernel_ms may be NULL; otherwise
 * it receives the time between HIP events around the filter's kernels, without the copies. */
int rt_svgf_filter(int device, const rt_svgf_params *params, int Wn, int H, const float *value, const rt_hit *hits,
                   const float *moments, const float *len, float *out_value, float *out_variance, float *out_estimate,
                   double *kernel_ms);

/* the bytes of d_scratch rt_svgf_filter_device needs for these arguments (the packed guide, the values with their variance --
 * two frames of them for more than one iteration -- and, where a pass of its own makes it, the luminance term's tolerance); 0 for
 * arguments the calls refuse */
uint64_t rt_svgf_scratch_bytes(const rt_svgf_params *params, int Wn, int H);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream): enqueues only, allocates nothing and
 * never synchronises, so it follows rt_temporal_accumulate_device on the same stream without a host wait.  The inputs are only
 * read; d_out_variance and d_out_estimate may be NULL; d_scratch holds rt_svgf_scratch_bytes() bytes.  No output may overlap an
 * input, another output or the scratch, and the scratch no input.  Records and scratch 16-byte aligned, floats 4-byte aligned.
 * All stay valid until the stream has drained. */
int rt_svgf_filter_device(int device, const rt_svgf_params *params, int Wn, int H, const void *d_value, const void *d_hits,
                          const void *d_moments, const void *d_len, void *d_out_value, void *d_out_variance, void *d_out_estimate,
                          void *d_scratch, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_SVGF_H_ */
