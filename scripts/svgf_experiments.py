"""What profiles/svgf_experiments.txt records (include/rt_svgf.h): at 4096 x 4096, depth 4, on the built-in scene and the
1024-sphere grid, one and three channels, iterations 1..5 -- rt_svgf_filter_device over a history of six noisy frames under equal
cameras (every live pixel on the temporal path at min_history 4) against rt_denoise_device at the same iteration count on the same
frame in the same run (three channels: rt_denoise has no other) and against a device copy of the bytes the call moves; and the
estimate pass, the one-iteration call over that long history against the same call on a first frame, where every live pixel walks
the (2r+1)^2 window.  Every time is device time between events around device calls on one stream, the median of REPS interleaved
repetitions after a warm-up; one process, nothing downloaded inside a timed window.  The frames are the G-buffer's colours plus
Gaussian noise of sigma 0.05, another draw each frame.

    timeout 900 python scripts/svgf_experiments.py [--size 4096] [--reps 7] [--label TEXT] > profiles/svgf_experiments.txt

The choices that were measured and not kept are build switches of csrc/rt_svgf.hip; the profile is this script's output for the
library followed by its output for each of

    make -C tilecoderaytracer_amd/csrc variant NAME=svgf_pass DEFS=-DRT_SVGF_FUSED_PREFILTER=0       (--vf pass)
    make -C tilecoderaytracer_amd/csrc variant NAME=svgf_fused DEFS=-DRT_SVGF_FUSED_PREFILTER=1      (--vf kernel)
    make -C tilecoderaytracer_amd/csrc variant NAME=svgf_pixels8 DEFS=-DRT_SVGF_PIXELS=8
    make -C tilecoderaytracer_amd/csrc variant NAME=svgf_varplane DEFS=-DRT_SVGF_VAR_PLANE=1
    make -C tilecoderaytracer_amd/csrc variant NAME=svgf_lds DEFS=-DRT_SVGF_ESTIMATE_LDS=1
    TCRT_LIBRARY=tilecoderaytracer_amd/lib/variants/libtcrt_svgf_NAME.so python scripts/svgf_experiments.py --label NAME [--vf ...]

Counters, in runs of their own and with nothing else collected: --pmc makes one render, a history and REPS calls each of the
filter and of rt_denoise at three iterations on the built-in scene, three channels, and nothing else; --counters CSV sums a
rocprofv3 counter file per kernel.

    rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -d DIR --output-format csv -- python scripts/svgf_experiments.py --pmc --reps 3
    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY -d DIR2 --output-format csv -- ...
    python scripts/svgf_experiments.py --counters DIR/*/*_counter_collection.csv
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tilecoderaytracer_amd import HostScene, Renderer, TemporalHistory, capi  # noqa: E402
from tilecoderaytracer_amd.renderer import svgf_params  # noqa: E402


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
    return f"{t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"


def svgf_bytes(channels, iterations, vf="kept"):
    """the bytes a pixel the call moves, every plane counted once a pass that reads or writes it: the pack (48 in, 32 out), the
    estimate (value, moments, length and aux in, a cell and the estimate's float out -- the window's taps not counted), and per
    iteration the kernel (key, aux and a cell in, a cell out) and, where vf is made by a pass of its own (one channel in the
    library as kept), that pass (a cell in, 4 out) and the kernel's 4 more in"""
    cell = 16 if channels == 3 else 8
    own_pass = vf == "pass" or (vf == "kept" and channels == 1)
    return 80 + (4 * channels + 8 + 4 + 16 + cell) + iterations * ((cell + 4 + 4 if own_pass else 0) + 32 + cell + cell)


def sum_counters(path):
    import csv
    total = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            key = (row["Kernel_Name"].split("(")[0], row["Counter_Name"])
            n, v = total.get(key, (0, 0.0))
            total[key] = (n + 1, v + float(row["Counter_Value"]))
    for (kernel, counter), (n, v) in sorted(total.items()):
        if "svgf" in kernel or "denoise" in kernel:
            print(f"{kernel:64s} {counter:18s} dispatches {n:4d} sum {v:.6g} per dispatch {v / n:.6g}")


def counter_run(args):
    """--pmc: the calls whose kernels a counter run reads, and nothing else"""
    W = H = args.size
    N = W * H
    lib = capi.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    host = HostScene.named("builtin")
    r = Renderer(host)
    cam = capi.RtCameraDesc()
    C.memmove(C.byref(cam), host.camera, C.sizeof(cam))
    new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
    colours, records = new(N * 3), new(N * 12, torch.int32)
    r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)
    gen = torch.Generator(device="cuda").manual_seed(1)
    history = TemporalHistory(W, H, 3, max_history=32)
    for _ in range(args.frames):
        history.push_device(colours + 0.05 * torch.randn(colours.shape, generator=gen, device="cuda"), records, cam)
    p, dn = svgf_params(3, 3), capi.RtDenoiseParams(3, 3, 0.2)
    out, var = new(N * 3), new(N)
    scratch = new(int(lib.rt_svgf_scratch_bytes(C.byref(p), W, H)), torch.uint8)
    dn_scratch = new(int(lib.rt_denoise_scratch_bytes(C.byref(dn), W, H)), torch.uint8)
    s = history._sets[history.frames % 2]
    for _ in range(args.reps):
        capi.check(lib.rt_svgf_filter_device(0, C.byref(p), W, H, s["value"].data_ptr(), s["hits"].data_ptr(), s["moments"].data_ptr(),
                                             s["length"].data_ptr(), out.data_ptr(), var.data_ptr(), None, scratch.data_ptr(), stream))
        capi.check(lib.rt_denoise_device(0, C.byref(dn), W, H, s["value"].data_ptr(), records.data_ptr(), out.data_ptr(),
                                         dn_scratch.data_ptr(), stream))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--frames", type=int, default=6)
    ap.add_argument("--label", default="the library as built")
    ap.add_argument("--vf", default="kept", choices=("kept", "pass", "kernel"), help="who makes vf in the measured build")
    ap.add_argument("--pmc", action="store_true", help="only the calls a counter run reads")
    ap.add_argument("--counters", help="sum this rocprofv3 counter CSV per kernel and exit")
    args = ap.parse_args()
    if args.counters:
        return sum_counters(args.counters)
    if args.pmc:
        return counter_run(args)
    W = H = args.size
    N = W * H
    lib = capi.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# rt_svgf_filter_device, {W} x {H}, depth {args.depth}, {torch.cuda.get_device_name(0)}, {args.label}; device time "
          f"between events, median of {args.reps} interleaved repetitions; sigma_l 2, min_history 4, radius 3, 3 squarings, "
          f"match_color 1, no plane term")
    new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
    for scene in ("builtin", "grid32"):
        host = HostScene.named(scene)
        r = Renderer(host)
        cam = capi.RtCameraDesc()
        C.memmove(C.byref(cam), host.camera, C.sizeof(cam))
        colours, records = new(N * 3), new(N * 12, torch.int32)
        r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)
        gen = torch.Generator(device="cuda").manual_seed(1)
        print(f"\n== {scene} {W}x{H} depth {args.depth}")
        for channels in (3, 1):
            clean = colours if channels == 3 else (colours.view(N, 3) * torch.tensor([0.25, 0.5, 0.25], device="cuda")).sum(dim=1)
            noisy = lambda: clean + 0.05 * torch.randn(clean.shape, generator=gen, device="cuda")
            long, first = TemporalHistory(W, H, channels, max_history=32), TemporalHistory(W, H, channels, max_history=32)
            for k in range(args.frames):
                long.push_device(noisy(), records, cam)
            first.push_device(noisy(), records, cam)
            torch.cuda.synchronize()
            out, var, est = new(N * channels), new(N), new(N)
            biggest = svgf_params(channels, 5)
            scratch = new(int(lib.rt_svgf_scratch_bytes(C.byref(biggest), W, H)), torch.uint8)
            dn_scratch = dn_out = None
            if channels == 3:
                dn = capi.RtDenoiseParams(5, 3, 0.2)
                dn_scratch, dn_out = new(int(lib.rt_denoise_scratch_bytes(C.byref(dn), W, H)), torch.uint8), new(N * 3)

            def svgf(history, iterations, sigma_l=2.0):
                p = svgf_params(channels, iterations, sigma_l)
                s = history._sets[history.frames % 2]
                capi.check(lib.rt_svgf_filter_device(0, C.byref(p), W, H, s["value"].data_ptr(), s["hits"].data_ptr(),
                                                     s["moments"].data_ptr(), s["length"].data_ptr(), out.data_ptr(), var.data_ptr(),
                                                     est.data_ptr(), scratch.data_ptr(), stream))

            def denoise(iterations):
                p = capi.RtDenoiseParams(iterations, 3, 0.2)
                capi.check(lib.rt_denoise_device(0, C.byref(p), W, H, long._sets[long.frames % 2]["value"].data_ptr(),
                                                 records.data_ptr(), dn_out.data_ptr(), dn_scratch.data_ptr(), stream))

            print(f"-- {channels} channel(s): a history of {args.frames} frames, equal cameras")
            for iterations in range(1, 6):
                traffic = svgf_bytes(channels, iterations, args.vf) * N
                half, half2 = new(traffic // 8, torch.int32), new(traffic // 8, torch.int32)
                fns = {"svgf": lambda: svgf(long, iterations), "svgf sigma_l 0": lambda: svgf(long, iterations, 0.0),
                       "copy": lambda: half2.copy_(half)}
                if channels == 3:
                    fns["rt_denoise"] = lambda: denoise(iterations)
                res = interleaved(fns, args.reps)
                line = (f"   iterations {iterations}: svgf {fmt(res['svgf'])}, {svgf_bytes(channels, iterations, args.vf)} B/pixel, "
                        f"{res['svgf'][0] / res['copy'][0]:5.2f} x their copy ({res['copy'][0]:.3f} ms); without the luminance term "
                        f"{res['svgf sigma_l 0'][0]:.3f} ms")
                if channels == 3:
                    # rt_denoise: its pack (48 + 12 in, 48 out), an iteration 48 in and 16 out
                    line += (f"; rt_denoise {fmt(res['rt_denoise'])}, {108 + 64 * iterations} B/pixel: svgf is "
                             f"{res['svgf'][0] / res['rt_denoise'][0]:5.2f} x its time for "
                             f"{svgf_bytes(channels, iterations, args.vf) / (108 + 64 * iterations):5.2f} x its bytes")
                print(line)
                del half, half2
            res = interleaved({"long": lambda: svgf(long, 1), "first": lambda: svgf(first, 1)}, args.reps)
            svgf(first, 1)
            torch.cuda.synchronize()
            rec = records.view(N, 12)
            live = (rec[:, 0] >= 0) & ((rec[:, 11] & 2) == 0)
            print(f"   the estimate pass, one iteration: long history (no pixel takes the window) {fmt(res['long'])}; first frame "
                  f"({int(live.sum())} of {N} pixels take the 7 x 7 window) {fmt(res['first'])}: the window costs "
                  f"{res['first'][0] - res['long'][0]:.3f} ms; mean estimate over live pixels {float(est[live].double().mean()):.3e}")
            del long, first, out, var, est, scratch, dn_scratch, dn_out
            torch.cuda.empty_cache()
        r.close()
        del colours, records
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
