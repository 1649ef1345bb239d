/*
 * rt_capi_image.h -- the last stage of a renderer: a frame's fp32 colours, pixels[x][z] order (columns outermost, z contiguous,
 * z pointing up), converted on the GPU into 8-bit scanlines, the order every image format and display wants.  Colours are already
 * display-referred (calculatePixel clamps to 1.0, src/RayTracer.cpp:627-629); what this adds is exposure, a transfer curve and
 * the transpose, and a download of 3 or 4 bytes a pixel instead of 12.  Plain C99, versioned on its own (RT_CAPI_IMAGE_VERSION /
 * rt_capi_image_version()); rt_capi.h and the other extension headers are unchanged.  The conversion takes no scene: any colours
 * can be encoded.  The int codes (RT_OK, RT_ERR_*) and rt_last_error() are rt_capi.h's.
 *
 * INPUT.  rgb[(x*H + z)*3 + c], Wn columns of H pixels, as rt_render, rt_render_ssaa and rt_denoise write them.  Wn is whatever
 * the caller passes, a whole frame or a strip.
 *
 * DEFINITION.  The GPU result is bit-exact to this.  With C = channels, T[1..255] the thresholds of the transfer and
 * row(z) = bottom_up ? z : H-1-z, for every x in [0, Wn), z in [0, H), c in 0..2:
 *
 *     v    = rgb[(x*H + z)*3 + c] * exposure              one IEEE fp32 multiply, denormals kept
 *     code = the number of k in 1..255 with v >= T[k]     (a NaN v compares false everywhere: code 0)
 *     out[row(z)*pitch_bytes + x*C + c] = code;           for C == 4:  out[row(z)*pitch_bytes + x*4 + 3] = 255
 *
 * Every byte of out that is not named above is left untouched: the pitch_bytes - Wn*C bytes after a row's end, and everything
 * before and after the rows.  So a strip [x0, x1) of a wider image is encoded by passing out + x0*C and the image's pitch, and the
 * result is byte-identical to those columns of the whole frame's encode.
 *
 * A code is defined by comparisons alone, never by evaluating the curve: the 255 thresholds ARE the transfer, a float either
 * reaches T[k] or it does not, and no pow() of any library or device takes part.  T must be non-decreasing and hold no NaN;
 * equal entries (codes that never occur) and +-inf are allowed.
 *
 * BUILT-IN TABLES (rt_image_transfer_table returns them; out_T[k-1] = T[k]).
 *     RT_TRANSFER_LINEAR   T[k] = (float)((2k-1) / 510.0), computed in double: code = round(255 v), halves up.
 *     RT_TRANSFER_SRGB     T[k] = (float)E((k - 0.5)/255.0), computed in double, E(u) = u/12.92 for u <= 0.04045 and
 *                          pow((u+0.055)/1.055, 2.4) otherwise: code = round(255 sRGB_encode(v)).  The library carries this table
 *                          as 255 literals; they, not the formula, are the definition.
 *     RT_TRANSFER_CUSTOM   params->thresholds: 255 floats T[1..255] in host memory, copied by the call.
 *
 * ERRORS.  All argument checks come before any device work, RT_ERR_INVALID in this order: params is NULL; channels not 3 or 4;
 * bottom_up not 0 or 1; transfer unknown; exposure NaN, infinite or <= 0; transfer CUSTOM and thresholds NULL, holding a NaN or
 * descending; Wn or H not positive; 3 Wn H > 8e9 ("strip too large", rt_render's limit: every frame rt_render can make can be
 * encoded); pitch_bytes < Wn C, or pitch_bytes H > 3.2e10; channels 4 and pitch_bytes not a multiple of 4; a NULL buffer; for the
 * device variant, d_rgb not 4-byte aligned, then channels 4 and d_out not 4-byte aligned, then d_out's extent ((H-1) pitch_bytes
 * + Wn C bytes) overlapping d_rgb's.  With channels 3, d_out and pitch_bytes may have any alignment.  Then, without a HIP device,
 * RT_ERR_NO_DEVICE; a device index out of range is RT_ERR_INVALID.  rt_image_transfer_table refuses RT_TRANSFER_CUSTOM, an unknown
 * transfer and a NULL out_T with RT_ERR_INVALID.
 */
#ifndef RT_CAPI_IMAGE_H_
#define RT_CAPI_IMAGE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_IMAGE_VERSION 1

enum { RT_TRANSFER_SRGB = 0, RT_TRANSFER_LINEAR = 1, RT_TRANSFER_CUSTOM = 2 };

typedef struct rt_image_params {
    int32_t channels;        /* 3: r,g,b   4: r,g,b,255                                                               */
    int32_t bottom_up;       /* 0: row 0 is z = H-1 (top of the picture)   1: row 0 is z = 0                          */
    int32_t transfer;        /* RT_TRANSFER_*                                                                         */
    float   exposure;        /* finite, > 0                                                                           */
    const float *thresholds; /* RT_TRANSFER_CUSTOM: 255 floats T[1..255] (host memory, copied by the call); else ignored */
} rt_image_params;

int rt_capi_image_version(void);

/* the built-in tables: out_T[k-1] = T[k], k = 1..255 */
int rt_image_transfer_table(int transfer, float out_T[255]);

/* host memory, synchronous: rgb holds 3 Wn H floats, out H rows of pitch_bytes (the last one may end after Wn C bytes); only the
 * bytes the definition names are written.  kernel_ms may be NULL; otherwise it receives the time between HIP events around the
 * kernel, without the copies. */
int rt_encode_image(int device, const rt_image_params *params, int Wn, int H, const float *rgb, uint8_t *out, uint64_t pitch_bytes,
                    double *kernel_ms);

/* device memory on `device`, enqueued on hip_stream (a hipStream_t; NULL = the null stream): enqueues only, allocates nothing and
 * never synchronises -- the table travels in the kernel's arguments, so there is no scratch buffer -- and so follows
 * rt_render_device, rt_render_ssaa_device or rt_denoise_device on the same stream without a host wait.  d_rgb (12 Wn H bytes) is
 * only read; both buffers stay valid until the stream has drained. */
int rt_encode_image_device(int device, const rt_image_params *params, int Wn, int H, const void *d_rgb, void *d_out,
                           uint64_t pitch_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_CAPI_IMAGE_H_ */
