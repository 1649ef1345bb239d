/*
 * rt_temporal.hip -- implementation of include/rt_temporal.h: last frame's accumulated value carried to this frame's pixels
 * through the hit records, blended with the new sample, with the first two moments of luminance.  The header is the definition;
 * the kernel is bit-exact to it (the library's arithmetic flags: no contraction, correctly rounded divide, denormals kept).
 *
 * SHAPE.  The pass is memory-bound.  One lane a pixel, the 64 lanes of a wavefront along z, the contiguous
 * axis: a wavefront's 64 current records are 3 KiB contiguous, and the sample and every store are coalesced.  What depends on the previous camera alone -- the three cross products and q -- is computed once on the host, in
 * the same fp32 operations, and reaches the kernel as arguments: wave-uniform.  The (up to) four previous records of a pixel are
 * a gather; neighbouring lanes reproject to neighbouring cells of the previous frame, so their addresses are nearly contiguous
 * and the caches serve the overlap.  A tap's history words are loaded only after its record has passed the tests.  A workgroup is
 * 4 wavefronts on 4 neighbouring columns; workgroups stride over the tiles, so that a frame of any admitted shape is one launch.
 *
 * Two ways of fetching the current records were built and measured (profiles/temporal_experiments.txt): three 16-byte loads per
 * lane, 48 bytes apart between neighbouring lanes, or kStage: each wavefront's 3 KiB of current records staged through LDS by 192
 * lane-contiguous 16-byte loads.  At 4096 x 4096 with three channels the staged kernel takes 0.49-0.50 ms under equal cameras and
 * 0.77-0.81 ms under a trucked one, the other 0.52 and 0.85-0.87 ms, a device copy of the same 161 bytes a pixel 0.52-0.53 ms.  The
 * staged kernel is the one the library has; the other is compiled, with an entry point that names the variant
 * (rt_internal_temporal_variant), only into a build with -DRT_TEMPORAL_VARIANTS=1 (`make variant`), which is what
 * scripts/temporal_experiments.py needs to repeat the comparison.
 *
 * The kernel, rt_temporal_kernel, and the argument checks stand in rt_accumulate_body.h, which rt_motion.hip shares: this unit
 * instantiates the kernel without a motion table.
 */
#include "rt_accumulate_body.h"

#ifndef RT_TEMPORAL_VARIANTS
#define RT_TEMPORAL_VARIANTS 0         /* 1: also the variant that was measured and not kept, and the entry point that names it */
#endif

namespace {

template <int kC, bool kFirst, bool kStage>
void launch(dim3 grid, hipStream_t stream, const Buffers &b, const Args &A) {
    hipLaunchKernelGGL((rt_temporal_kernel<kC, kFirst, kStage, kNoTable>), grid, dim3(kTileZ, kTileX), 0, stream,
                       static_cast<const float *>(b.cur), static_cast<const uint4 *>(b.cur_hits),
                       static_cast<const uint4 *>(b.prev_hits), static_cast<const float *>(b.prev_value),
                       static_cast<const float *>(b.prev_moments), static_cast<const float *>(b.prev_len),
                       static_cast<float *>(b.out_value), static_cast<float *>(b.out_moments), static_cast<float *>(b.out_len),
                       static_cast<float *>(b.out_variance), static_cast<uint8_t *>(b.out_flags), A);
}

template <bool kStage>
void launch_any(int channels, bool first, dim3 grid, hipStream_t stream, const Buffers &b, const Args &A) {
    if (channels == 3) first ? launch<3, true, kStage>(grid, stream, b, A) : launch<3, false, kStage>(grid, stream, b, A);
    else first ? launch<1, true, kStage>(grid, stream, b, A) : launch<1, false, kStage>(grid, stream, b, A);
}

/* the kernel, enqueued on stream; every argument already checked, the device current, the buffers the device's */
int enqueue(const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam, int W, int H, int x0, int x1,
            const Buffers &b, hipStream_t stream, bool staged) {
    const Args A = make_args(pr, cam_prev, cam, W, H, x0, x1);
    const bool first = cam_prev == nullptr;
    const dim3 grid = grid_of(A);
#if RT_TEMPORAL_VARIANTS
    if (!staged) {
        launch_any<false>(pr->channels, first, grid, stream, b, A);
        HIP_TRY(hipGetLastError());
        return RT_OK;
    }
#endif
    (void)staged;
    launch_any<true>(pr->channels, first, grid, stream, b, A);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

/* rt_temporal_accumulate_device's checks and launch; staged: the variant (true in a build that has one) */
int accumulate_device(int device, const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam, int W,
                      int H, int x0, int x1, const Buffers &b, void *hip_stream, bool staged) {
    int rc = check_params(pr, W, H, x0, x1);
    if (rc) return rc;
    if ((rc = check_buffers(cam_prev, cam, b.cur, b.cur_hits, b.prev_hits, b.prev_value, b.prev_moments, b.prev_len, b.out_value,
                            b.out_moments, b.out_len)))
        return rc;
    if ((rc = check_device_buffers(pr, W, H, x0, x1, b, nullptr, 0, false))) return rc;
    if ((rc = rt_internal_check_device(device))) return rc;
    HIP_TRY(hipSetDevice(device));
    return enqueue(pr, cam_prev, cam, W, H, x0, x1, b, static_cast<hipStream_t>(hip_stream), staged);
}

} // namespace

extern "C" {

int rt_capi_temporal_version(void) { return RT_CAPI_TEMPORAL_VERSION; }

int rt_temporal_accumulate(int device, const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam, int W,
                           int H, int x0, int x1, const float *cur, const rt_hit *cur_hits, const rt_hit *prev_hits,
                           const float *prev_value, const float *prev_moments, const float *prev_len, float *out_value,
                           float *out_moments, float *out_len, float *out_variance, uint8_t *out_flags, double *kernel_ms) {
    int rc = check_params(pr, W, H, x0, x1);
    if (rc) return rc;
    if ((rc = check_buffers(cam_prev, cam, cur, cur_hits, prev_hits, prev_value, prev_moments, prev_len, out_value, out_moments,
                            out_len)))
        return rc;
    if ((rc = rt_internal_check_device(device))) return rc;
    const size_t strip = (size_t)(x1 - x0) * (size_t)H, frame = (size_t)W * (size_t)H, cb = (size_t)pr->channels * sizeof(float);
    const HostIn in[6] = {{cur, strip * cb},        {cur_hits, strip * sizeof(rt_hit)}, {prev_hits, frame * sizeof(rt_hit)},
                          {prev_value, frame * cb}, {prev_moments, frame * 8},          {prev_len, frame * 4}};
    const HostOut out[5] = {{out_value, strip * cb}, {out_moments, strip * 8}, {out_len, strip * 4}, {out_variance, strip * 4},
                            {out_flags, strip}};
    return staged_call(device, in, 6, out, 5, 0, kernel_ms, [&](void *const *d_in, void *const *d_out, void *) {
        const Buffers b{d_in[0], d_in[1], d_in[2], d_in[3], d_in[4], d_in[5], d_out[0], d_out[1], d_out[2], d_out[3], d_out[4]};
        return enqueue(pr, cam_prev, cam, W, H, x0, x1, b, nullptr, true);
    });
}

int rt_temporal_accumulate_device(int device, const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam,
                                  int W, int H, int x0, int x1, const void *d_cur, const void *d_cur_hits, const void *d_prev_hits,
                                  const void *d_prev_value, const void *d_prev_moments, const void *d_prev_len, void *d_out_value,
                                  void *d_out_moments, void *d_out_len, void *d_out_variance, void *d_out_flags, void *hip_stream) {
    const Buffers b{d_cur, d_cur_hits, d_prev_hits, d_prev_value, d_prev_moments, d_prev_len, d_out_value, d_out_moments, d_out_len,
                    d_out_variance, d_out_flags};
    return accumulate_device(device, pr, cam_prev, cam, W, H, x0, x1, b, hip_stream, true);
}

#if RT_TEMPORAL_VARIANTS
/* development aid, not in the header: rt_temporal_accumulate_device with the variant named (staged 0 / 1), for the comparison
 * recorded in profiles/temporal_experiments.txt */
int rt_internal_temporal_variant(int device, const rt_temporal_params *pr, const rt_camera_desc *cam_prev, const rt_camera_desc *cam,
                                 int W, int H, int x0, int x1, const void *d_cur, const void *d_cur_hits, const void *d_prev_hits,
                                 const void *d_prev_value, const void *d_prev_moments, const void *d_prev_len, void *d_out_value,
                                 void *d_out_moments, void *d_out_len, void *d_out_variance, void *d_out_flags, void *hip_stream,
                                 int staged) {
    const Buffers b{d_cur, d_cur_hits, d_prev_hits, d_prev_value, d_prev_moments, d_prev_len, d_out_value, d_out_moments, d_out_len,
                    d_out_variance, d_out_flags};
    return accumulate_device(device, pr, cam_prev, cam, W, H, x0, x1, b, hip_stream, staged != 0);
}
#endif

} // extern "C"
