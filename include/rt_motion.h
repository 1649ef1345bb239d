/*
 * rt_motion.h -- temporal accumulation that follows moving objects.  rt_temporal_accumulate (include/rt_temporal.h) reprojects a
 * pixel's hit point through the previous camera only, so a pixel on an object that moved lands on a previous cell that holds
 * another surface: it restarts at length 1 or blends in history of other surface points.  The record already names its object;
 * these calls take, beside rt_temporal_accumulate's arguments, one rigid motion per object "to the previous frame" and apply it
 * before the reprojection and in the tap tests.  Plain C99, versioned on its own (RT_CAPI_MOTION_VERSION /
 * rt_capi_motion_version()); no other header changes a declaration, and rt_temporal_params is rt_temporal.h's.
 *
 * THE TABLE.  motions[o], o in [0, n_motions), is the motion of Scene object o (rt_hit.object): 12 floats m[0..11], the rows
 * {m0 m1 m2 | m3}, {m4 m5 m6 | m7}, {m8 m9 m10 | m11} of a 3 x 3 linear part and a translation, which carry a point of the object
 * in the CURRENT frame to where that surface point was in the PREVIOUS frame.  The linear part is meant to be a rotation; nothing
 * checks that, and nothing renormalises.  Layout, strips, the previous frame's buffers, the outputs and the first-frame rule are
 * rt_temporal.h's, word for word.
 *
 * DEFINITION.  The GPU result is bit-exact to this.  It is rt_temporal.h's DEFINITION, and every word of that definition stands;
 * three places change, for a live record h with o = h.object, P = h.point, N = h.normal:
 *   STATIC OR MOVING.  h is static if motions is NULL, or o >= n_motions, or the 12 words of motions[o] equal, as BITS, those
 *      of {1,0,0,0, 0,1,0,0, 0,0,1,0} with every zero +0.0f.  Otherwise h is moving.
 *   WHERE THE POINT AND NORMAL WERE.  For a static record Pp = P and Np = N, word for word, no arithmetic.  For a moving record,
 *      with m = motions[o].m, one rounding per operation in this order, for k = 0, 1, 2 (x, y, z):
 *        Pp.k = ((m[4k]*P.x + m[4k+1]*P.y) + m[4k+2]*P.z) + m[4k+3]
 *        Np.k =  (m[4k]*N.x + m[4k+1]*N.y) + m[4k+2]*N.z
 *   Step 2 (IDENTITY) applies only when the two cameras are equal as bits AND the record is static.  A moving record always goes
 *      through step 3, also under equal cameras (cam_prev's words are then cam's).
 *   Step 3: D = Pp - eye; everything after that as written.
 *   Step 4: the normal test is dot(Np, g.normal) >= normal_cos; the plane test is e = g.point - Pp, d = dot(e, Np),
 *      d*d <= plane_eps*plane_eps.  Object, side and colour are compared with h as in rt_temporal.h.
 *
 * WHAT FOLLOWS.  With n_motions == 0, or a table of identity entries only, or a table shorter than every object index that
 * occurs, the call is rt_temporal_accumulate word for word.  A strip equals the frame's columns.  A NaN anywhere in a motion
 * gives that object's pixels no history, by the way the comparisons are written (Pp.k and Np.k are NaN, so s or the normal test
 * fails).  The motion table is never read on a first frame.
 *
 * Not provided: history is not invalidated here where a mover's shadow or reflection passes over a surface that stayed
 * (include/rt_clamp.h clips such history to the frame's neighbourhood, as a call of its own after this one; alpha fades it
 * everywhere); deforming or scaling objects; history behind glass (mirrors: include/rt_mirror.h);
 * supersampled frames; several GPUs; the counting build; a command-line flag (the executable has no animated scene).
 *
 * ERRORS.  The checks are rt_temporal_accumulate's, in its order, each RT_ERR_INVALID and each before any device work.  The new
 * ones: after the first-frame rule, n_motions < 0 or n_motions > 4096 (the scene's object limit), then motions NULL while
 * n_motions > 0.  In the device variant d_motions not 16-byte aligned is refused in the same clause as the records'
 * alignment, and the overlap check includes the table (no output may share a byte with it).
 */
#ifndef RT_MOTION_H_
#define RT_MOTION_H_

#include "rt_capi_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_CAPI_MOTION_VERSION 1

struct rt_temporal_params;               /* include/rt_temporal.h has it; a caller includes that header to fill one */

typedef struct rt_object_motion {
    float m[12];             /* rows {m0 m1 m2 m3}, {m4 .. m7}, {m8 .. m11}: linear part and translation */
} rt_object_motion;          /* 48 bytes */

int rt_capi_motion_version(void);

/* host memory, synchronous: rt_temporal_accumulate with the table.  kernel_ms may be NULL. */
int rt_motion_accumulate(int device, const struct rt_temporal_params *params, const rt_camera_desc *cam_prev,
                         const rt_camera_desc *cam, int W, int H, int x0, int x1, const rt_object_motion *motions, int n_motions,
                         const float *cur, const rt_hit *cur_hits, const rt_hit *prev_hits, const float *prev_value,
                         const float *prev_moments, const float *prev_len, float *out_value, float *out_moments, float *out_len,
                         float *out_variance, uint8_t *out_flags, double *kernel_ms);

/* device memory on `device`, enqueued on hip_stream: enqueues only, allocates nothing and never synchronises.  d_motions is
 * device memory of the caller, 16-byte aligned, valid until the stream has drained; its contents are not checked. */
int rt_motion_accumulate_device(int device, const struct rt_temporal_params *params, const rt_camera_desc *cam_prev,
                                const rt_camera_desc *cam, int W, int H, int x0, int x1, const void *d_motions, int n_motions,
                                const void *d_cur, const void *d_cur_hits, const void *d_prev_hits, const void *d_prev_value,
                                const void *d_prev_moments, const void *d_prev_len, void *d_out_value, void *d_out_moments,
                                void *d_out_len, void *d_out_variance, void *d_out_flags, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_MOTION_H_ */
