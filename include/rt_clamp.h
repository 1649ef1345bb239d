/*
 * rt_clamp.h -- neighbourhood clipping of an accumulated history.  rt_temporal_accumulate (include/rt_temporal.h) and
 * rt_motion_accumulate (include/rt_motion.h) keep a pixel's history whenever its hit record says "same surface"; where the LIGHT
 * on a surface that stayed changes -- a mover's shadow slides over the floor, a reflection passes, a light is switched -- the old
 * value stays in the history and fades only as 1/N.  rt_history_clamp runs after the blend: each pixel's accumulated value is
 * clipped to a box made from THIS frame's samples on the same surface around it, and where it had to be clipped the history
 * length is cut and the moments are shifted, so that the next frames blend fast and rt_svgf_filter (include/rt_svgf.h) estimates
 * the pixel's variance spatially.  The pipeline is G-buffer, sampled term, rt_temporal_accumulate or rt_motion_accumulate, this
 * call, rt_svgf_filter, rt_encode_image.  Plain C99, versioned on its own (RT_CAPI_CLAMP_VERSION / rt_capi_clamp_version());
 * no other header changes a declaration.  Like rt_svgf_filter the calls take a device index and no scene.
 *
 * INPUT.  A rectangle of Wn x H pixels in pixels[x][z] order (z contiguous), a whole frame or a strip, rt_svgf.h's; taps outside
 * it do not exist.  cur[(x*H + z)*channels + k] and hits[x*H + z] (rt_hit, include/rt_capi_query.h) are what the accumulate call
 * was GIVEN for this frame; value (as cur), moments[(x*H + z)*2 + {0, 1}] and len[x*H + z] are what it WROTE.  All fp32.  The
 * outputs are out_value, out_moments, out_len, out_variance (Wn H; may be NULL) and out_flags (Wn H bytes; may be NULL).
 * out_value, out_moments and out_len may BE value, moments and len (the same pointer): a pixel reads no other pixel's history, so
 * the call runs in place on the accumulate call's outputs.  No output may overlap cur or hits, which are read at neighbours, or
 * overlap anything else partially.  The calls need no scratch: rt_history_clamp_device takes no buffer beside these.
 *
 * DEFINITION.  The GPU result is bit-exact to this.  All arithmetic is IEEE fp32, one rounding per operation, no contraction, a
 * correctly rounded divide and square root, in the order written; every comparison is written so that a NaN means "skip" or
 * "leave" (a numpy restatement needs where(t > 0, t, 0), not maximum).  lum, dead and key are rt_svgf.h's, word for word:
 *   lum(c)    = (0.25f*c.r + 0.5f*c.g) + 0.25f*c.b for 3 channels, the value itself for 1
 *   dead(p)   : hits[p].object < 0 or hits[p].flags & RT_HIT_LIGHT
 *   key(p, q) : hits[q].object == hits[p].object, (hits[q].flags & 3) == (hits[p].flags & 3) and, with match_color, the three
 *               colour words of hits[q] and hits[p] equal as BITS
 * For pixel p = (x, z), with c = cur[p], v = value[p], m1 = moments[p*2], m2 = moments[p*2 + 1], L = len[p], r = radius:
 *
 *   1. LEFT ALONE.  If dead(p), or !(L > 1.0f) (no history, a first frame, or NaN): every output word of p is its input word, bit
 *      for bit; its flag is 0; its out_variance is as in step 5.
 *   2. TAPS.  From cnt = 0, s1 = s2 = 0 and mn = mx = c (per channel):
 *        for a in -r..r (x offset), for b in -r..r (z offset), in this order, q = (x+a, z+b) inside the rectangle:
 *            q = p always counts, untested.  Any other q counts only if it is not dead, key(p, q) holds and
 *                (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z >= normal_cos
 *            for a tap that counts:  cnt = cnt + 1.0f  and per channel k
 *                s1.k = s1.k + cur[q].k;  s2.k = s2.k + cur[q].k*cur[q].k
 *                if (cur[q].k < mn.k) mn.k = cur[q].k;  if (cur[q].k > mx.k) mx.k = cur[q].k
 *      The cur words of a tap that does not count have no influence on any output word (an implementation may load them, inside
 *      the rectangle, and drop them).
 *      If cnt < (float)min_taps: the pixel is left as in step 1, with flag 2.
 *   3. BOX.  box 0: lo = mn, hi = mx.  box 1, per channel:
 *            mean = s1/cnt;  e2 = s2/cnt;  var = e2 - mean*mean;  var = var > 0 ? var : +0.0f
 *            w = gamma * sqrtf(var);  lo = mean - w;  hi = mean + w
 *   4. CLIP.  Per channel: v' = v; if (v < lo) v' = lo; if (v' > hi) v' = hi.  The pixel is clipped if either `if` fired in any
 *      channel.  Not clipped: every word as in step 1, with flag 0.  Clipped, with flag 1:
 *            out_value = v'
 *            L' = L;  if (!(L <= (float)clip_history)) L' = (float)clip_history
 *            m1' = m1 + (lum(v') - lum(v))
 *            m2' = m2 + (m1'*m1' - m1*m1)
 *   5. out_variance = t > 0 ? t : +0.0f with t = m2' - m1'*m1', taken from the OUTPUT moments of the pixel.
 *
 * WHAT FOLLOWS.  For a pixel that is not clipped all words and the variance are the accumulate call's, bit for bit -- +0.0 for a
 * pixel without history included.  The call applied to its own output changes nothing, bit for bit: the box depends on cur alone
 * and a clipped value sits on the box.  With box 0 a pixel whose value lies within its own window's samples is never touched.
 * With box 0 and min_taps = 1 an isolated pixel's history is replaced by its own sample: min_taps exists for that reason.  A
 * strip differs from the frame's columns only within `radius` columns of its edges.  Cutting len below rt_svgf_params.min_history
 * makes rt_svgf_filter estimate that pixel's variance spatially: that is the intended hand-over.
 *
 * Not provided: the clip fused into the accumulate kernel (a clip before the blend), temporal-gradient (A-SVGF) weights (they are
 * include/rt_gradient.h's, a call of its own that runs before this one), several GPUs, the counting build, supersampled frames
 * (they have no records), a command-line flag (the executable has no animated scene).  Not tested: buffers past 2^32 bytes (every offset is a 64-bit element index by construction).  Not tested either, and
 * deliberately never launched: a rectangle of H = 1 with Wn >= 268 435 453.  The checks admit it (Wn * H <= 533 333 333); its one
 * row of tiles is 2^26 or more workgroups of 64 x 4 threads, 2^32 or more threads along x, and what HIP does with such a launch --
 * refuse it, or run a truncated grid -- is not known here.
 *
 * ERRORS.  Int codes and rt_last_error() as everywhere.  All argument checks come before any device work, RT_ERR_INVALID in this
 * order: params is NULL; channels not 1 or 3; box not 0 or 1; radius outside 1..3; match_color not 0 or 1; min_taps outside
 * 1..49; clip_history outside 1..65535; normal_cos NaN or outside -1..1; gamma negative, NaN or infinite; Wn or H not positive;
 * Wn * H > 533 333 333 pixels (rt_render_gbuffer's limit); a NULL required buffer (cur, hits, value, moments, len, out_value,
 * out_moments, out_len); for the device variant, records not 16-byte aligned, then floats not 4-byte aligned, then a forbidden
 * overlap: an output overlapping cur or hits, another output, its own input other than exactly, or a different input.  Then,
 * without a HIP device, RT_ERR_NO_DEVICE; a device index out of range is RT_ERR_INVALID.  Every offset is 64-bit.
 */
#ifndef RT_CLAMP_H_
#define RT_CLAMP_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_CLAMP_VERSION 1

typedef struct rt_clamp_params {
    int32_t channels;      /* 1 or 3 */
    int32_t box;           /* 0: extremes (min / max of the taps), 1: moments (mean -/+ gamma * sd) */
    int32_t radius;        /* 1..3: the window is (2r+1)^2 */
    int32_t match_color;   /* 0 / 1: a tap must carry the pixel's colour words, as bits */
    int32_t min_taps;      /* 1..49: with fewer counted taps the pixel is left alone */
    int32_t clip_history;  /* 1..65535: a clipped pixel's length becomes at most this */
    float   normal_cos;    /* finite, -1..1 */
    float   gamma;         /* finite, >= 0; read only with box 1 */
} rt_clamp_params;         /* 32 bytes */

int rt_capi_clamp_version(void);

/* host memory, synchronous.  out_value, out_moments and out_len may be value, moments and len; out_variance and out_flags may be
 * NULL.  out_flags: 0 untouched, 1 clipped, 2 left alone for fewer than min_taps taps.  kernel_ms may be NULL; otherwise it
 * receives the time between HIP events around the kernel, without the copies. */
int rt_history_clamp(int device, const rt_clamp_params *params, int Wn, int H, const float *cur, const rt_hit *hits,
                     const float *value, const float *moments, const float *len, float *out_value, float *out_moments,
                     float *out_len, float *out_variance, uint8_t *out_flags, double *kernel_ms);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream): one kernel launch; enqueues only,
 * allocates nothing, never synchronises and needs no scratch, so it follows rt_temporal_accumulate_device or
 * rt_motion_accumulate_device on the same stream without a host wait, in place on their outputs if wanted.  d_out_variance and
 * d_out_flags may be NULL.  Records 16-byte aligned, floats 4-byte aligned.  All stay valid until the stream has drained. */
int rt_history_clamp_device(int device, const rt_clamp_params *params, int Wn, int H, const void *d_cur, const void *d_hits,
                            const void *d_value, const void *d_moments, const void *d_len, void *d_out_value,
                            void *d_out_moments, void *d_out_len, void *d_out_variance, void *d_out_flags, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_CLAMP_H_ */
