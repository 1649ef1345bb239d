"""What profiles/temporal_experiments.txt records (include/rt_temporal.h): at 4096 x 4096, depth 4, on the built-in scene and
the 1024-sphere grid, three channels -- the accumulation kernel against a device copy of the bytes it moves, for equal cameras
(the identity path) and for a camera trucked by 0.3 units along its horizontal vector (reprojection, four taps); the kernel as
it is against the variant that stages the current records through LDS; and the mean variance over live pixels after 1, 4 and 16
accumulated frames of rt_indirect_diffuse at n = 1 under equal cameras.  Every time is device time between events around device
calls on one stream, the median of REPS interleaved repetitions after a warm-up; one process, nothing downloaded inside a timed
window.  The comparison needs both variants, which only a build with -DRT_TEMPORAL_VARIANTS=1 has:

    make -C tilecoderaytracer_amd/csrc variant NAME=temporal_variants DEFS=-DRT_TEMPORAL_VARIANTS=1
    TCRT_LIBRARY=tilecoderaytracer_amd/lib/variants/libtcrt_temporal_variants.so \
    timeout 600 python scripts/temporal_experiments.py [--size 4096] [--reps 7] > profiles/temporal_experiments.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tilecoderaytracer_amd import HostScene, Renderer, TemporalHistory, capi  # noqa: E402
from tilecoderaytracer_amd.renderer import temporal_params  # noqa: E402


def interleaved(fns, reps, warmup=2):
    """{name: (median, min, max)} of each fn's device time, one repetition of each in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def fmt(t):
    return f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def trucked(cam, distance):
    """the camera moved by `distance` along its horizontal vector: eye and screen alike"""
    out = capi.RtCameraDesc()
    C.memmove(C.byref(out), C.byref(cam), C.sizeof(out))
    h = list(cam.vector_horizontal)
    norm = sum(v * v for v in h) ** 0.5
    for k in range(3):
        out.eye_origin[k] = cam.eye_origin[k] + distance * h[k] / norm
        out.screen_origin[k] = cam.screen_origin[k] + distance * h[k] / norm
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--depth", type=int, default=4)
    args = ap.parse_args()
    W = H = args.size
    N = W * H
    lib = capi.load_library()
    if not hasattr(lib, "rt_internal_temporal_variant"):
        sys.exit("this library has one variant: build with -DRT_TEMPORAL_VARIANTS=1 and name it in TCRT_LIBRARY")
    lib.rt_internal_temporal_variant.argtypes = lib.rt_temporal_accumulate_device.argtypes + [C.c_int]
    lib.rt_internal_temporal_variant.restype = C.c_int
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# temporal accumulation, {W} x {H}, depth {args.depth}, 3 channels, {torch.cuda.get_device_name(0)}; device time "
          f"between events, median of {args.reps} interleaved repetitions")
    params = temporal_params(3, False, 32, 0.9, 0.05, 0.0, 0.0)
    new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
    for scene in ("builtin", "grid32"):
        host = HostScene.named(scene)
        r = Renderer(host)
        cam = capi.RtCameraDesc()
        C.memmove(C.byref(cam), host.camera, C.sizeof(cam))
        cams = {"equal cameras": cam, "truck 0.3": trucked(cam, -0.3)}          # the PREVIOUS camera of each case
        colours, records = new(N * 3), new(N * 12, torch.int32)
        prev_records = {}
        own = r._cam
        for name, c in cams.items():
            prev_records[name] = new(N * 12, torch.int32)
            r._cam = C.pointer(c)
            r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), prev_records[name].data_ptr(), stream)
        r._cam = own
        r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)
        prev = [torch.rand((N * k,), dtype=torch.float32, device="cuda") for k in (3, 2, 1)]
        prev[2].mul_(5.0).add_(1.0)
        out = [new(N * 3), new(N * 2), new(N), new(N), new(N, torch.uint8)]
        # records, sample, the previous frame's records and history words once each, the five outputs
        traffic = (48 + 12 + 48 + 12 + 8 + 4 + 12 + 8 + 4 + 4 + 1) * N
        half, half2 = new(traffic // 8, torch.int32), new(traffic // 8, torch.int32)
        print(f"\n== {scene} {W}x{H} depth {args.depth}: the kernel's traffic {traffic / 1e6:.1f} MB (161 bytes a pixel: 48 + 12 current, "
              f"48 + 24 previous, 29 out); the copy moves the same ({traffic / 2e6:.1f} MB read, as many written)")

        # ---- 1. and 2. the kernel and its variant against the copy -----------------------------------------------------------
        fns = {"copy": lambda: half2.copy_(half)}
        for name, c in cams.items():
            for staged in (0, 1):
                fns[f"{name:14s} staged={staged}"] = (lambda c=c, name=name, staged=staged: capi.check(lib.rt_internal_temporal_variant(
                    0, C.byref(params), C.byref(c), C.byref(cam), W, H, 0, W, colours.data_ptr(), records.data_ptr(),
                    prev_records[name].data_ptr(), prev[0].data_ptr(), prev[1].data_ptr(), prev[2].data_ptr(),
                    *[t.data_ptr() for t in out], stream, staged)))
        res = interleaved(fns, args.reps)
        for k, t in res.items():
            print(f"   {k:36s} {fmt(t)}  {traffic / 1e6 / t[0]:8.1f} GB/s  {t[0] / res['copy'][0]:5.2f} x the copy")
        for name, c in cams.items():
            fns[f"{name:14s} staged=0"]()
            torch.cuda.synchronize()
            without = int(out[4].sum())
            print(f"   {name}: {without} of {N} pixels without history ({100.0 * without / N:.2f} %)")
        del half, half2, prev, out, prev_records
        torch.cuda.empty_cache()

        # ---- 3. the variance of one-sample indirect light as frames accumulate -----------------------------------------------
        history = TemporalHistory(W, H, 3, max_history=32)
        live = None
        print("   rt_indirect_diffuse n = 1, gather depth 1, equal cameras, seed = frame index, max_history 32, alpha 0:")
        for k in range(16):
            r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)
            r.indirect_diffuse_device(N, records.data_ptr(), colours.data_ptr(), colours.data_ptr(), stream, samples=1, seed=k)
            value, variance, flags = history.push_device(colours, records, cam)
            if live is None:
                rec = records.view(N, 12)
                live = (rec[:, 0] >= 0) & ((rec[:, 11] & 2) == 0)
            if k + 1 in (1, 4, 16):
                torch.cuda.synchronize()
                v = variance[live].double()
                print(f"   after {k + 1:2d} frame(s): mean variance of luminance over {int(live.sum())} live pixels {float(v.mean()):.6e}, "
                      f"of the mean's (variance / frames) {float(v.mean()) / (k + 1):.6e}; pixels with variance > 0: {int((v > 0).sum())}")
        del history, colours, records, live
        r.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
