/*
 * rt_motion.hip -- implementation of include/rt_motion.h: rt_temporal_accumulate with one rigid motion per object, applied to a
 * record's point and normal before the reprojection and in the tap tests.  The header is the definition; the kernel is bit-exact
 * to it.  The kernel is the one copy in rt_accumulate_body.h, rt_temporal_kernel, which rt_temporal.hip instantiates without a
 * table and this unit with one.
 *
 * SHAPE.  rt_temporal.hip's: one lane a pixel, 64 lanes along z, the current records staged through LDS,
 * workgroups striding over the tiles.  A lane whose record is live and whose object has an entry reads that entry's 48 bytes and
 * compares them with the identity's bits; only a lane whose entry differs computes Pp and Np and leaves the identity path.  A
 * call that cannot have a moving record -- a first frame, n_motions 0, or on the host path a table whose entries are all the
 * identity's bits -- is handed to rt_temporal_accumulate_device as it is: the same kernel, the same words.  On the host path
 * the table is cut after its last entry that differs from the identity (the entries behind are static by either rule).
 *
 * Two ways of reading the table were built and measured (profiles/motion_experiments.txt): (a) three 16-byte loads per lane
 * from global memory, (b) the table staged in LDS once per workgroup before its loop over the tiles, for tables of at most
 * kLdsMotions entries.  At 4096 x 4096 with three channels and every sphere moved, (b) is within the spread of (a) at 32 entries
 * (0.549 against 0.550 ms under equal cameras) and slower at 170 (0.561 against 0.548 ms): a frame of that size is one
 * workgroup a tile, so every tile pays the staging, while (a)'s loads hit the caches whatever the table's length.  (a) is the
 * path the library has, for every length; RT_MOTION_LDS=1 would give tables of at most kLdsMotions entries to (b).  (b) is
 * compiled, with an entry point that names the path (rt_internal_motion_variant), only into a build with
 * -DRT_MOTION_VARIANTS=1 (`make variant`), which is what scripts/motion_experiments.py needs to repeat the comparison.
 */
#include "../../include/rt_motion.h"
#include "rt_accumulate_body.h"

static_assert(sizeof(rt_object_motion) == 48, "rt_object_motion layout");

#ifndef RT_MOTION_LDS
#define RT_MOTION_LDS 0                /* 1: tables of at most kLdsMotions entries are staged in LDS (path b) */
#endif
#ifndef RT_MOTION_VARIANTS
#define RT_MOTION_VARIANTS 0           /* 1: both paths, and the entry point that names one */
#endif

namespace {

constexpr int kMaxMotions = 4096;      /* the scene's object limit */

template <int kC, int kTable>
void launch(dim3 grid, hipStream_t stream, const Buffers &b, const void *d_motions, int n_motions, const Args &A) {
    /* never a first frame (that one reads no table), always the staged records */
    hipLaunchKernelGGL((rt_temporal_kernel<kC, false, true, kTable, const uint4 *, int>), grid, dim3(kTileZ, kTileX), 0, stream,
                       static_cast<const float *>(b.cur), static_cast<const uint4 *>(b.cur_hits), static_cast<const uint4 *>(b.prev_hits),
                       static_cast<const float *>(b.prev_value), static_cast<const float *>(b.prev_moments),
                       static_cast<const float *>(b.prev_len), static_cast<float *>(b.out_value),
                       static_cast<float *>(b.out_moments), static_cast<float *>(b.out_len), static_cast<float *>(b.out_variance),
                       static_cast<uint8_t *>(b.out_flags), A, static_cast<const uint4 *>(d_motions), n_motions);
}

/* the table's checks, after the first-frame rule */
int check_table(const void *motions, int n_motions) {
    if (n_motions < 0 || n_motions > kMaxMotions) return fail(RT_ERR_INVALID, "n_motions must be 0..4096");
    if (!motions && n_motions > 0) return fail(RT_ERR_INVALID, "motions is NULL while n_motions > 0");
    return RT_OK;
}

/* the kernel, enqueued on stream; every argument already checked, the device current, the buffers and the table the device's.
 * path: kTableGlobal, kTableLds, or kNoTable for the library's own choice */
int enqueue(int device, const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam, int W, int H, int x0,
            int x1, const void *d_motions, int n_motions, const Buffers &b, hipStream_t stream, int path) {
    if (!cam_prev || n_motions == 0)       /* no record can be moving: rt_temporal.hip's kernel, and the table is never read */
        return rt_temporal_accumulate_device(device, pr, cam_prev, cam, W, H, x0, x1, b.cur, b.cur_hits, b.prev_hits, b.prev_value,
                                             b.prev_moments, b.prev_len, b.out_value, b.out_moments, b.out_len, b.out_variance,
                                             b.out_flags, stream);
    const Args A = make_args(pr, cam_prev, cam, W, H, x0, x1);
    const dim3 grid = grid_of(A);
    if (path == kNoTable) path = RT_MOTION_LDS && n_motions <= kLdsMotions ? kTableLds : kTableGlobal;
#if RT_MOTION_LDS || RT_MOTION_VARIANTS
    if (path == kTableLds) {
        if (n_motions > kLdsMotions) return fail(RT_ERR_INVALID, "the table does not fit the LDS path");
        pr->channels == 3 ? launch<3, kTableLds>(grid, stream, b, d_motions, n_motions, A)
                          : launch<1, kTableLds>(grid, stream, b, d_motions, n_motions, A);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
#endif
    pr->channels == 3 ? launch<3, kTableGlobal>(grid, stream, b, d_motions, n_motions, A)
                      : launch<1, kTableGlobal>(grid, stream, b, d_motions, n_motions, A);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

/* rt_motion_accumulate_device's checks and launch */
int accumulate_device(int device, const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam, int W,
                      int H, int x0, int x1, const void *d_motions, int n_motions, const Buffers &b, void *hip_stream, int path) {
    int rc = check_params(pr, W, H, x0, x1);
    if (rc) return rc;
    if ((rc = check_buffers(cam_prev, cam, b.cur, b.cur_hits, b.prev_hits, b.prev_value, b.prev_moments, b.prev_len, b.out_value,
                            b.out_moments, b.out_len)))
        return rc;
    if ((rc = check_table(d_motions, n_motions))) return rc;
    if ((rc = check_device_buffers(pr, W, H, x0, x1, b, d_motions, (size_t)n_motions * sizeof(rt_object_motion), true))) return rc;
    if ((rc = rt_internal_check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue(device, pr, cam_prev, cam, W, H, x0, x1, d_motions, n_motions, b, static_cast<hipStream_t>(hip_stream), path);
}

/* the entries of a host table up to its last one that differs from the identity's bits: those behind are static by either rule */
int entries_that_matter(const rt_object_motion *motions, int n_motions) {
    static const rt_object_motion identity = {{1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f}};
    while (n_motions > 0 && std::memcmp(&motions[n_motions - 1], &identity, sizeof identity) == 0) n_motions -= 1;
    return n_motions;
}

} // namespace

extern "C" {

int rt_capi_motion_version(void) { return RT_CAPI_MOTION_VERSION; }

int rt_motion_accumulate(int device, const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam, int W,
                         int H, int x0, int x1, const rt_object_motion *motions, int n_motions, const float *cur,
                         const rt_hit *cur_hits, const rt_hit *prev_hits, const float *prev_value, const float *prev_moments,
                         const float *prev_len, float *out_value, float *out_moments, float *out_len, float *out_variance,
                         uint8_t *out_flags, double *kernel_ms) {
    int rc = check_params(pr, W, H, x0, x1);
    if (rc) return rc;
    if ((rc = check_buffers(cam_prev, cam, cur, cur_hits, prev_hits, prev_value, prev_moments, prev_len, out_value, out_moments,
                            out_len)))
        return rc;
    if ((rc = check_table(motions, n_motions))) return rc;
    if ((rc = rt_internal_check_device(device))) return rc;
    const int n = cam_prev ? entries_that_matter(motions, n_motions) : 0;      /* (a first frame never reads the table) */
    const size_t strip = (size_t)(x1 - x0) * (size_t)H, frame = (size_t)W * (size_t)H, cb = (size_t)pr->channels * sizeof(float);
    const HostIn in[7] = {{cur, strip * cb},        {cur_hits, strip * sizeof(rt_hit)}, {prev_hits, frame * sizeof(rt_hit)},
                          {prev_value, frame * cb}, {prev_moments, frame * 8},          {prev_len, frame * 4},
                          {n ? motions : nullptr, (size_t)n * sizeof(rt_object_motion)}};
    const HostOut out[5] = {{out_value, strip * cb}, {out_moments, strip * 8}, {out_len, strip * 4}, {out_variance, strip * 4},
                            {out_flags, strip}};
    return staged_call(device, in, 7, out, 5, 0, kernel_ms, [&](void *const *d_in, void *const *d_out, void *) {
        const Buffers b{d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], d_in[5], d_out[0], d_out[1], d_out[2], d_out[3], d_out[4]};
        return enqueue(device, pr, cam_prev, cam, W, H, x0, x1, d_in[6], n, b, nullptr, kNoTable);
    });
}

int rt_motion_accumulate_device(int device, const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam,
                                int W, int H, int x0, int x1, const void *d_motions, int n_motions, const void *d_cur,
                                const void *d_cur_hits, const void *d_prev_hits, const void *d_prev_value, const void *d_prev_moments,
                                const void *d_prev_len, void *d_out_value, void *d_out_moments, void *d_out_len, void *d_out_variance,
                                void *d_out_flags, void *hip_stream) {
    const Buffers b{d_cur, d_cur_hits, d_prev_hits, d_prev_value, d_prev_moments, d_prev_len, d_out_value, d_out_moments, d_out_len,
                    d_out_variance, d_out_flags};
    return accumulate_device(device, pr, cam_prev, cam, W, H, x0, x1, d_motions, n_motions, b, hip_stream, kNoTable);
}

#if RT_MOTION_VARIANTS
/* development aid, not in the header: rt_motion_accumulate_device with the table path named (1: global memory, 2: LDS, which
 * refuses a table of more than 170 entries), for the comparison recorded in profiles/motion_experiments.txt */
int rt_internal_motion_variant(int device, const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam,
                               int W, int H, int x0, int x1, const void *d_motions, int n_motions, const void *d_cur,
                               const void *d_cur_hits, const void *d_prev_hits, const void *d_prev_value, const void *d_prev_moments,
                               const void *d_prev_len, void *d_out_value, void *d_out_moments, void *d_out_len, void *d_out_variance,
                               void *d_out_flags, void *hip_stream, int path) {
    if (path != kTableGlobal && path != kTableLds) return fail(RT_ERR_INVALID, "path must be 1 or 2");
    const Buffers b{d_cur, d_cur_hits, d_prev_hits, d_prev_value, d_prev_moments, d_prev_len, d_out_value, d_out_moments, d_out_len,
                    d_out_variance, d_out_flags};
    return accumulate_device(device, pr, cam_prev, cam, W, H, x0, x1, d_motions, n_motions, b, hip_stream, path);
}
#endif

} // extern "C"
