/*
 * rt_gradient.h -- temporal-gradient weights for an accumulated history (the A-SVGF idea).  rt_temporal_accumulate
 * (include/rt_temporal.h) and rt_motion_accumulate (include/rt_motion.h) keep a pixel's history whenever its hit record says "same
 * surface"; where the LIGHT on a surface that stayed changes -- a mover's shadow slides over the floor, a light is switched -- the
 * old value stays in the history.  rt_history_clamp (include/rt_clamp.h) judges that from the current frame's neighbourhood alone,
 * so it cannot tell noise from change.  A temporal gradient can: shade the SAME points with the SAME random numbers in this frame's
 * scene and in the previous frame's, at one cell per s x s pixels, and look at the difference.  Where nothing that lights a point
 * changed the two values are equal as bits, whatever the noise, and the history is provably left alone; where they differ the
 * history is stale by a known relative amount, lambda, and rt_gradient_reweight blends it towards this frame's sample by lambda.
 * The pipeline is G-buffer, sampled term, rt_temporal_accumulate or rt_motion_accumulate, this call, rt_history_clamp,
 * rt_svgf_filter, rt_encode_image.  Plain C99, versioned on its own (RT_CAPI_GRADIENT_VERSION / rt_capi_gradient_version()); no
 * other header changes a declaration.  Like rt_history_clamp the calls take a device index and no scene: how the two cell frames
 * are made is the caller's (rt_render_gbuffer of both poses under this frame's camera at W/s x H/s, then rt_indirect_diffuse or
 * rt_ambient_occlusion with equal seed and key0, give them).
 *
 * LAYOUT.  A rectangle of Wn x H pixels in pixels[x][z] order (z contiguous), a whole frame or a strip, rt_clamp.h's.
 * cur[(x*H + z)*channels + k] and hits[x*H + z] (rt_hit, include/rt_capi_query.h) are what the accumulate call was GIVEN for this
 * frame; value (as cur), moments[(x*H + z)*2 + {0, 1}] and len[x*H + z] are what it WROTE.  All fp32.  With s = scale,
 * Wl = ceil(Wn / s) and Hl = ceil(H / s); cell (i, j) is stored at i*Hl + j and belongs to pixel (i*s, j*s), rt_capi_upsample.h's
 * layout.  now_lo and then_lo hold Wl*Hl*channels floats: the term at the cells in this frame's scene and in the previous frame's.
 * lo_hits holds the Wl*Hl records now_lo was made from; then_hits the records then_lo was made from, and may be NULL.  The outputs
 * are out_value, out_moments, out_len, out_variance (Wn H floats; may be NULL), out_lambda (Wn H floats; may be NULL) and out_flags
 * (Wn H bytes; may be NULL).  out_value, out_moments and out_len may BE value, moments and len (the same pointer): a pixel reads no
 * other pixel's history, so the call runs in place on the accumulate call's outputs.  No output may overlap cur, hits, now_lo,
 * then_lo, lo_hits or then_hits, or overlap anything else partially.  One kernel launch, no scratch.
 *
 * DEFINITION.  The GPU result is bit-exact to this.  All arithmetic is IEEE fp32, one rounding per operation, no contraction, a
 * correctly rounded divide, in the order written; every comparison is written so that a NaN means "skip" or "leave" (a numpy
 * restatement needs where(t > 0, t, 0), not maximum).  lum and dead are rt_clamp.h's, word for word:
 *   lum(c)    = (0.25f*c.r + 0.5f*c.g) + 0.25f*c.b for 3 channels, the value itself for 1
 *   dead(g)   : g.object < 0 or g.flags & RT_HIT_LIGHT
 * Per cell q, with g = lo_hits[q]:
 *      ln = lum(now_lo[q]);  lt = lum(then_lo[q])
 *      d = ln - lt;  if (d < 0) d = -d
 *      m = ln;  if (lt > m) m = lt
 *      if then_hits != NULL and (then_hits[q].object != g.object or (then_hits[q].flags & 3) != (g.flags & 3)):
 *          d = m                 -- the geometry under the cell changed: a full gradient
 * For pixel p = (x, z), with h = hits[p], c = cur[p], v = value[p], m1 = moments[p*2], m2 = moments[p*2 + 1], L = len[p],
 * l = lum(c), s = scale, r = radius:
 *
 *   1. LEFT ALONE.  If dead(h), or !(L > 1.0f) (no history, a first frame, or NaN): every output word of p is its input word, bit
 *      for bit; its flag is 0; its out_lambda is +0.0f; its out_variance is as in step 6.
 *   2. CELLS.  i0 = x / s, j0 = z / s (integers).  From cnt = 0, num = 0, den = 0:
 *        for a in -r..r+1 (cell column i0+a), for b in -r..r+1 (cell row j0+b), in this order:
 *            skip the cell unless 0 <= i0+a < Wl and 0 <= j0+b < Hl;  g = lo_hits[(i0+a)*Hl + (j0+b)]
 *            skip if dead(g)
 *            skip unless g.object == h.object and (g.flags & 3) == (h.flags & 3)
 *            with match_color: skip unless the three colour words of g and h are equal as BITS
 *            skip unless (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z >= normal_cos        (n_p = h.normal, n_q = g.normal)
 *            a cell that counts:  cnt = cnt + 1;  num = num + d(q);  den = den + m(q)
 *      The words of a cell that does not count have no influence on any output word (an implementation may load them and drop
 *      them).  If cnt == 0: the pixel is left as in step 1, with flag 2.
 *   3. WEIGHT.  t = den > den_floor ? num / den : +0.0f;  lambda = gain * t;  if (lambda > 1.0f) lambda = 1.0f
 *      out_lambda = lambda > 0 ? lambda : +0.0f.  If !(lambda > lambda_min): the pixel is left as in step 1, with flag 0 (its
 *      out_lambda stays what this step gave it).
 *   4. RESTART, if lambda == 1.0f, flag 3: out_value = c word for word; moments (l, l*l); len 1.0f -- what the accumulate calls
 *      write for a pixel without history.
 *   5. REBLEND, otherwise, flag 1:
 *            v'.k = v.k + lambda*(c.k - v.k)
 *            m1' = m1 + lambda*(l - m1)
 *            m2' = m2 + lambda*(l*l - m2)
 *            a = 1.0f / L;  a2 = a + lambda*(1.0f - a);  L' = 1.0f / a2
 *            if (!(L' >= 1.0f)) L' = 1.0f;  if (!(L' <= L)) L' = L
 *   6. out_variance = t > 0 ? t : +0.0f with t = m2' - m1'*m1', taken from the OUTPUT moments of the pixel.
 *
 * WHAT FOLLOWS.  With now_lo and then_lo equal as bits (NaNs apart), and then_hits NULL or equal to lo_hits, every output word is
 * the input's: d is +0.0 in every cell, so is lambda, and lambda_min >= 0.  A pixel with lambda <= lambda_min keeps every word and
 * its variance, the accumulate call's bit for bit.  gain 0 is the identity.  The call is NOT idempotent: applied to its own output
 * it blends again (lambda depends on the cell frames alone, not on the history), so it runs once a frame.  Noise common to both
 * cell frames cancels only where the term is evaluated with the same random numbers in both scenes: that is why the cell frames
 * are rendered under ONE camera with equal seed and key0.  Taps outside the rectangle do not exist: a strip [x0, x1) with
 * x0 % s == 0, given the frame's cells [x0/s, ceil(x1/s)), equals the frame's columns except those whose window reaches cells
 * beyond the strip's.  Order in the pipeline: accumulate, this call, then rt_history_clamp, then the filter -- the clamp sees the
 * re-blended history, and a restarted pixel (len 1) is left alone by it.
 *
 * Not provided: forward projection of previous samples (both cell frames are this frame's points, so a surface seen only in the
 * previous frame has no gradient), a spatial filter of lambda beyond the window, several GPUs, the counting build, supersampled
 * frames (they have no records), mirrored or refracted content other than through guide records (include/rt_mirror.h,
 * include/rt_glass.h), a command-line flag (the executable has no animated scene).  Not tested: buffers past 2^32 bytes (every
 * offset is a 64-bit element index by construction).
 *
 * ERRORS.  Int codes and rt_last_error() as everywhere.  All argument checks come before any device work, RT_ERR_INVALID in this
 * order: params is NULL; channels not 1 or 3; scale outside 2..8; radius outside 0..2; match_color not 0 or 1; normal_cos NaN or
 * outside -1..1; gain negative, NaN or infinite; lambda_min NaN or outside 0..1; den_floor negative, NaN or infinite; Wn or H not
 * positive; Wn * H > 533 333 333 pixels (rt_render_gbuffer's limit), or ceil(Wn / 4) * ceil(H / 64) >= 2^24 (a launch has fewer
 * than 2^32 work-items, 256 for every tile of 4 x 64 pixels: only rectangles under 8 rows high reach it); a NULL required buffer
 * (cur, hits, value, moments, len, now_lo, then_lo, lo_hits, out_value, out_moments, out_len); for the device variant, records
 * (hits, lo_hits, then_hits) not 16-byte aligned, then floats not 4-byte aligned, then a forbidden overlap: an output overlapping
 * cur, hits or a cell buffer, another output, its own input other than exactly, or a different input.  Then, without a HIP
 * device, RT_ERR_NO_DEVICE; a device index out of range is RT_ERR_INVALID.  Every offset is 64-bit.
 */
#ifndef RT_GRADIENT_H_
#define RT_GRADIENT_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_GRADIENT_VERSION 1

typedef struct rt_gradient_params {
    int32_t channels;      /* 1 or 3 */
    int32_t scale;         /* s, 2..8: one cell per s x s pixels, rt_capi_upsample.h's layout */
    int32_t radius;        /* r, 0..2: the window is (2r+2)^2 cells */
    int32_t match_color;   /* 0 / 1: a cell must carry the pixel's colour words, as bits */
    float   normal_cos;    /* finite, -1..1 */
    float   gain;          /* finite, >= 0 */
    float   lambda_min;    /* finite, 0..1: at or below it a pixel is left alone */
    float   den_floor;     /* finite, >= 0: at or below it the cells' light is too dim to judge, lambda = 0 */
} rt_gradient_params;      /* 32 bytes */

int rt_capi_gradient_version(void);

/* host memory, synchronous.  out_value, out_moments and out_len may be value, moments and len; then_hits, out_variance, out_lambda
 * and out_flags may be NULL.  out_flags: 0 untouched, 1 re-blended, 2 left alone for no counted cell, 3 restarted.  kernel_ms may
 * be NULL; otherwise it receives the time between HIP events around the kernel, without the copies. */
int rt_gradient_reweight(int device, const rt_gradient_params *params, int Wn, int H, const float *cur, const rt_hit *hits,
                         const float *value, const float *moments, const float *len, const float *now_lo, const float *then_lo,
                         const rt_hit *lo_hits, const rt_hit *then_hits, float *out_value, float *out_moments, float *out_len,
                         float *out_variance, float *out_lambda, uint8_t *out_flags, double *kernel_ms);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream): one kernel launch; enqueues only,
 * allocates nothing, never synchronises and needs no scratch, so it follows rt_temporal_accumulate_device or
 * rt_motion_accumulate_device on the same stream without a host wait, in place on their outputs if wanted, and can be captured in
 * a graph.  d_then_hits, d_out_variance, d_out_lambda and d_out_flags may be NULL.  Records 16-byte aligned, floats 4-byte
 * aligned.  All stay valid until the stream has drained. */
int rt_gradient_reweight_device(int device, const rt_gradient_params *params, int Wn, int H, const void *d_cur, const void *d_hits,
                                const void *d_value, const void *d_moments, const void *d_len, const void *d_now_lo,
                                const void *d_then_lo, const void *d_lo_hits, const void *d_then_hits, void *d_out_value,
                                void *d_out_moments, void *d_out_len, void *d_out_variance, void *d_out_lambda, void *d_out_flags,
                                void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_GRADIENT_H_ */
