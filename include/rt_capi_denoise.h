/*
 * rt_capi_denoise.h -- cleaning up a noisy frame: an edge-avoiding a-trous wavelet filter over a frame's colours, steered by the
 * hit records rt_render_gbuffer writes beside them (include/rt_capi_gbuffer.h).  Soft shadows (include/rt_capi_soft.h) cost
 * n x n shadow scans per light and shading point; one sample (n = 1) and this filter is the cheap way to a smooth penumbra.
 * Plain C99, versioned on its own (RT_CAPI_DENOISE_VERSION / rt_capi_denoise_version()); rt_capi.h and the other extension
 * headers are unchanged.  The filter takes no scene: any colours with any records can be filtered.
 *
 * INPUT.  A rectangle of Wn x H pixels in pixels[x][z] order (z contiguous): colours rgb[(x*H + z)*3 + c] as rt_render writes
 * them and guide records hits[x*H + z] (rt_hit, include/rt_capi_query.h) as rt_render_gbuffer writes them.  Wn is whatever the
 * caller passes, a whole frame or a strip; taps outside the rectangle do not exist.  So a strip filtered alone differs from the
 * same columns of the filtered frame within 2 * (2^iterations - 1) columns of its edges, and nowhere else.
 *
 * DEFINITION.  The GPU result is bit-exact to this.  All arithmetic is IEEE fp32 with no contraction and a correctly rounded
 * divide, in the order written.  Iteration i = 0 .. iterations-1 has step s = 1 << i and reads the complete output of iteration
 * i-1 as `in` (iteration 0 reads rgb); the last iteration's output is the result.  With h = {1/16, 1/4, 3/8, 1/4, 1/16} (the B3
 * spline: every product h[j]*h[k] is exact in fp32) and lum(c) = (0.25f*c.r + 0.5f*c.g) + 0.25f*c.b, for pixel p = (x, z):
 *
 *     pass-through (out[p] = in[p], bit for bit) if hits[p].object < 0 or (hits[p].flags & RT_HIT_LIGHT)
 *     inv = sigma_color > 0 ? 1.0f / ((sigma_color * 2^-i) * (sigma_color * 2^-i)) : unused
 *     acc = (0,0,0); wsum = 0
 *     for a in -2..2 (x offset), for b in -2..2 (z offset), in this order:
 *         q = (x + a*s, z + b*s); skip if outside the rectangle
 *         skip unless hits[q].object == hits[p].object and the three words of hits[q].color equal those of hits[p].color as
 *              BITS (same object, same material / checker tile / texel: the filter never crosses albedo)
 *         t  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z     (n = hits[].normal)
 *         wn = t > 0 ? t : 0;  repeat normal_squarings times: wn = wn*wn
 *         w  = (h[a+2]*h[b+2]) * wn
 *         if sigma_color > 0:  d = lum(in[q]) - lum(in[p]);  u = 1.0f - (d*d)*inv;  w = w * (u > 0 ? u : 0)
 *         skip unless w > 0
 *         acc.c = acc.c + w * in[q].c   (c = r, g, b);   wsum = wsum + w
 *     out[p] = wsum > 0 ? acc / wsum : in[p]                 (three divides)
 *
 * Every comparison is written so that a NaN gives "skip": a NaN anywhere in a weight drops the tap, 0 * NaN never enters acc,
 * and a NaN or infinite colour never spreads through a weight -- only as in[q] of a tap whose weight is positive and finite.
 * (A numpy restatement needs where(t > 0, t, 0), not maximum.)  2^-i is exact; the colour term narrows as the step widens.
 *
 * LIMITS.  Reflections and refractions seen in a surface are filtered by that surface's geometry plus the colour term only;
 * an image texture magnified less than a few pixels per texel leaves nothing to average (every texel is its own albedo);
 * hard shadow edges soften by what sigma_color lets through.  There is no temporal accumulation, no variance estimate and no
 * albedo demodulation, no multi-GPU path, and supersampled frames (include/rt_capi_ssaa.h) have no records to filter by.
 *
 * ERRORS.  Int codes and rt_last_error() as everywhere.  All argument checks come before any device work, RT_ERR_INVALID in
 * this order: params is NULL; iterations outside 1..5; normal_squarings outside 0..6; sigma_color negative, NaN or infinite;
 * Wn or H not positive; Wn * H > 533 333 333 pixels (rt_render_gbuffer's limit: 3.2e10 bytes of colours and records); a NULL
 * buffer (rgb, hits, out_rgb; for the device variant also d_scratch); for the device variant, d_hits or d_scratch not 16-byte
 * aligned, then d_rgb or d_out_rgb not 4-byte aligned; for the device variant, d_out_rgb overlapping d_rgb.  Then, without a HIP
 * device, RT_ERR_NO_DEVICE; a device index out of range is RT_ERR_INVALID.  rt_denoise_scratch_bytes returns 0 for arguments
 * the other calls refuse.
 */
#ifndef RT_CAPI_DENOISE_H_
#define RT_CAPI_DENOISE_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_DENOISE_VERSION 1

typedef struct rt_denoise_params {
    int32_t iterations;          /* 1..5: steps 1, 2, 4, 8, 16 -- a footprint of 4 * (2^iterations - 1) + 1 pixels a side */
    int32_t normal_squarings;    /* 0..6: the normal weight is max(n_p . n_q, 0) ^ (2 ^ normal_squarings)                 */
    float   sigma_color;         /* finite, >= 0; 0: no colour term                                                       */
} rt_denoise_params;

int rt_capi_denoise_version(void);

/* host memory, synchronous: rgb and out_rgb hold 3 Wn H floats (they may be the same buffer), hits Wn H records.  kernel_ms may
 * be NULL; otherwise it receives the time between HIP events around the filter's kernels, without the copies. */
int rt_denoise(int device, const rt_denoise_params *params, int Wn, int H, const float *rgb, const rt_hit *hits, float *out_rgb,
               double *kernel_ms);

/* the bytes of d_scratch rt_denoise_device needs for these arguments (the packed guide, 32 bytes a pixel, and one frame of
 * colours with their luminance, 16 bytes a pixel -- two frames for more than one iteration) */
uint64_t rt_denoise_scratch_bytes(const rt_denoise_params *params, int Wn, int H);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream): enqueues only, allocates nothing
 * and never synchronises, so it follows rt_render_gbuffer_device on the same stream without a host wait.  d_rgb (12 Wn H bytes)
 * and d_hits (48 Wn H bytes, 16-byte aligned) are only read; d_out_rgb (12 Wn H bytes) must not overlap d_rgb; d_scratch holds
 * rt_denoise_scratch_bytes() bytes, 16-byte aligned, and must overlap none of the others.  All stay valid until the stream has
 * drained. */
int rt_denoise_device(int device, const rt_denoise_params *params, int Wn, int H, const void *d_rgb, const void *d_hits,
                      void *d_out_rgb, void *d_scratch, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_DENOISE_H_ */
