/*
 * rt_capi_upsample.h -- gathering at 1/s^2 density: rt_ambient_occlusion (include/rt_capi_ao.h) and rt_indirect_diffuse
 * (include/rt_capi_indirect.h) trace n x n rays for every record they are given, and both terms are smooth wherever the surface
 * is.  So gather for every s-th pixel in both directions only, and carry the result to full resolution by a joint-bilateral
 * filter steered by the full-resolution records -- which say exactly where the surface changes.  Plain C99, versioned on its own
 * (RT_CAPI_UPSAMPLE_VERSION / rt_capi_upsample_version()); rt_capi.h and the other extension headers are unchanged.  Like
 * rt_denoise the calls take a device index and no scene: any values with any records can be carried.
 *
 * LAYOUT.  A rectangle of Wn x H pixels in pixels[x][z] order (z contiguous), records hits[x*H + z] (rt_hit,
 * include/rt_capi_query.h) as rt_render_gbuffer writes them.  Pixel (x, z) of a frame is the camera ray through (x/W, z/H), so
 * "the low-resolution frame" of scale s is simply the records at pixels (i*s, j*s) of the frame one has: no second render, no
 * half-pixel offset, and Wn and H need not be multiples of s.  Wl = ceil(Wn / s), Hl = ceil(H / s); low-resolution cell (i, j) is
 * stored at i*Hl + j and belongs to pixel (i*s, j*s), which always exists.  Low-resolution values are lo[(i*Hl + j)*channels + c],
 * full-resolution ones out[(x*H + z)*channels + c].
 *
 * SUBSAMPLE.  out_lo[i*Hl + j] = hits[(i*s)*H + j*s], word for word.  With white = 1 the three colour words of a live record
 * (object >= 0 and not RT_HIT_LIGHT) are replaced by 1.0f; a dead record is copied as it is.  Of white records
 * rt_indirect_diffuse returns (kd * gain) * mean: irradiance without the albedo, which `modulate` below puts back per pixel.
 *
 * UPSAMPLE: DEFINITION.  The GPU result is bit-exact to this.  All arithmetic is IEEE fp32, one rounding per operation, no
 * contraction, a correctly rounded divide, in the order written; every comparison is written so that a NaN means "skip" (a numpy
 * restatement needs where(t > 0, t, 0), not maximum).  For pixel p = (x, z), h = hits[p], c ranging over the channels:
 *
 *   1. dead: h.object < 0 or (h.flags & RT_HIT_LIGHT).  Then v.c = dead_value, flag 0, and `modulate` does not apply.
 *   2. i0 = x / s, j0 = z / s, fx = x - i0*s, fz = z - j0*s (integers).  own sample: if fx == 0 and fz == 0 then
 *      v = lo[i0, j0] word for word, flag 0.
 *   3. otherwise acc = 0, wsum = 0, and for a in 0..1, for b in 0..1, in this order:
 *        the cell is (i0+a, j0+b); skip it if i0+a >= Wl or j0+b >= Hl
 *        tent = (float)((a ? fx : s-fx) * (b ? fz : s-fz))      (an exact integer); skip if it is 0
 *        g = hits[((i0+a)*s)*H + (j0+b)*s]
 *        skip unless g.object == h.object and (g.flags & 3) == (h.flags & 3)
 *        with match_color: skip unless the three colour words of g and h are equal as BITS
 *        t  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z          (n_p = h.normal, n_q = g.normal)
 *        wn = t > 0 ? t : 0;  repeat normal_squarings times: wn = wn*wn
 *        w  = tent * wn
 *        if sigma_plane > 0, with inv = 1.0f / (sigma_plane*sigma_plane):
 *            e = g.point - h.point (per component);  d = (e.x*n_p.x + e.y*n_p.y) + e.z*n_p.z
 *            u = 1.0f - (d*d)*inv;  w = w * (u > 0 ? u : 0)
 *        skip unless w > 0
 *        acc.c = acc.c + w * lo[cell].c;  wsum = wsum + w
 *   4. if wsum > 0: v = acc / wsum, flag 0.  Otherwise the pixel is a HOLE: flag 1, and v is the same sum with w = tent alone
 *      over the cells that exist and whose tent is not 0 (cell (i0, j0) always is one: the sum is never empty).
 *   5. modulate: for a pixel that is not dead, v.c = v.c * h.color.c.
 *   6. out = base ? base + v : v   (never evaluated as 0 + v).
 *   7. out_flags[p], if asked for, is the flag byte.
 *
 * WHAT FOLLOWS.  The gathered pixels keep the gather's bits.  A filter never crosses an object or the inside / outside and
 * light bits of its records, and with match_color never a checker tile or texel.  Taps outside the rectangle do not exist: a
 * strip [x0, x1) with x0 % s == 0 upsampled alone equals the frame's columns except those whose right-hand cell (x/s + 1) lies
 * beyond the strip's cells, i.e. columns from ((x1-1)/s)*s + 1 on where x1 is not the frame's end.  A strip's low-resolution records
 * are the frame's cells [x0/s, ceil(x1/s)), and key0 = (x0/s)*Hl gives rt_ambient_occlusion and rt_indirect_diffuse the frame's
 * sampling keys for them.  Holes are pixels none of whose four cells lies on their surface (thin objects, mostly): they are
 * reported, not hidden, so that a caller may gather for them at full resolution.
 *
 * Not provided: several GPUs, the counting build, supersampled frames (they have no records), scales above 8, filtering across
 * refracted content (a pane's record is the pane's; for mirrors, include/rt_mirror.h makes the guide records of what they
 * show), and hole refinement without a host read-back of the flags.
 *
 * ERRORS.  Int codes and rt_last_error() as everywhere.  All argument checks come before any device work, RT_ERR_INVALID in this
 * order: params is NULL; scale outside 2..8; channels not 1 or 3; normal_squarings outside 0..6; match_color, modulate (for the
 * subsample: white) not 0 or 1; modulate with channels 1; sigma_plane negative, NaN or infinite; dead_value NaN or infinite; Wn
 * or H not positive; Wn * H > 533 333 333 pixels (rt_render_gbuffer's limit), or ceil(Wn / 4) * ceil(H / 64) >= 2^24 (a launch
 * has fewer than 2^32 work-items, 256 for every tile of 4 x 64 pixels: only rectangles under 8 rows high reach it); a NULL
 * buffer (hits, lo, out; hits, out_lo); for the device variants, records not 16-byte aligned, then floats (and, for the subsample, nothing else) not 4-byte aligned; for
 * rt_upsample_guided_device, d_out overlapping d_lo.  Then, without a HIP device, RT_ERR_NO_DEVICE; a device index out of range
 * is RT_ERR_INVALID.  Every offset is 64-bit.
 */
#ifndef RT_CAPI_UPSAMPLE_H_
#define RT_CAPI_UPSAMPLE_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_UPSAMPLE_VERSION 1

typedef struct rt_upsample_params {
    int32_t scale;             /* s, 2..8 */
    int32_t channels;          /* 1 (AO's plane) or 3 */
    int32_t normal_squarings;  /* 0..6, as rt_denoise */
    int32_t match_color;       /* 0 / 1: a tap must carry the pixel's colour words, as bits */
    int32_t modulate;          /* 0 / 1: multiply by the pixel's own colour (channels must be 3) */
    float   sigma_plane;       /* finite, >= 0; 0: no plane term */
    float   dead_value;        /* finite: the value of a pixel with no surface (1 for AO, 0 for light) */
} rt_upsample_params;          /* 28 bytes */

int rt_capi_upsample_version(void);

/* host memory, synchronous: hits holds Wn H records, out_lo ceil(Wn/scale) ceil(H/scale) */
int rt_subsample_hits(int device, int scale, int white, int Wn, int H, const rt_hit *hits, rt_hit *out_lo);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream): enqueues only, allocates nothing
 * and never synchronises.  Both 16-byte aligned; they must not overlap. */
int rt_subsample_hits_device(int device, int scale, int white, int Wn, int H, const void *d_hits, void *d_out_lo, void *hip_stream);

/* host memory, synchronous: hits Wn H records, lo Wl Hl channels floats, base (NULL: none; it may be out) and out Wn H channels
 * floats, out_flags (NULL: not wanted) Wn H bytes.  kernel_ms may be NULL; otherwise it receives the time between HIP events
 * around the kernel, without the copies. */
int rt_upsample_guided(int device, const rt_upsample_params *p, int Wn, int H, const rt_hit *hits, const float *lo,
                       const float *base, float *out, uint8_t *out_flags, double *kernel_ms);

/* device memory, as rt_subsample_hits_device: d_hits (16-byte aligned), d_lo and d_base are only read, d_base (NULL: none) may
 * be d_out, d_out must not overlap d_lo, d_out_flags may be NULL.  All stay valid until the stream has drained. */
int rt_upsample_guided_device(int device, const rt_upsample_params *p, int Wn, int H, const void *d_hits, const void *d_lo,
                              const void *d_base, void *d_out, void *d_out_flags, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_UPSAMPLE_H_ */
