"""What profiles/upsample_experiments.txt records (include/rt_capi_upsample.h): at 4096 x 4096, depth 4, on the built-in scene
and the 1024-sphere grid -- the two tap-loading variants of the upsample kernel against a device copy of the same traffic, the
subsample kernel, frames with an AO plane or one diffuse bounce gathered at scale 1 (the full-resolution path), 2 and 4, the share
of holes, and what `refine` adds.  Every figure is device time between events around device calls on one stream, the median of
REPS interleaved repetitions after a warm-up; nothing is downloaded inside a timed window except refine's flags.
The frames are composed here from the device calls Renderer.render_indirect(scale=) and render_ao(scale=) make (their small
allocations inside the window, their download left out): device-side figures, not timings of those Python calls.  The kernel
comparison needs both tap-loading variants, which only a build with -DRT_UPSAMPLE_VARIANTS=1 has:

    make -C tilecoderaytracer_amd/csrc variant NAME=upsample_variants DEFS=-DRT_UPSAMPLE_VARIANTS=1
    TCRT_LIBRARY=tilecoderaytracer_amd/lib/variants/libtcrt_upsample_variants.so \
    python scripts/upsample_experiments.py [--size 4096] [--reps 7] > profiles/upsample_experiments.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tilecoderaytracer_amd import HostScene, Renderer, capi  # noqa: E402
from tilecoderaytracer_amd.renderer import upsample_params  # noqa: E402


def timed(fn, reps, warmup=2):
    """median, min, max of fn()'s device time in ms"""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def interleaved(fns, reps, warmup=1):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--depth", type=int, default=4)
    args = ap.parse_args()
    W = H = args.size
    N = W * H
    lib = capi.load_library()
    if not hasattr(lib, "rt_internal_upsample_variant"):
        sys.exit("this library has one tap-loading variant: build with -DRT_UPSAMPLE_VARIANTS=1 and name it in TCRT_LIBRARY")
    vp = C.c_void_p
    lib.rt_internal_upsample_variant.argtypes = [C.c_int, C.POINTER(capi.RtUpsampleParams), C.c_int, C.c_int, vp, vp, vp, vp, vp, vp,
                                                 C.c_int]
    lib.rt_internal_upsample_variant.restype = C.c_int
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# guided upsampling, {W} x {H}, depth {args.depth}, {torch.cuda.get_device_name(0)}; device time between events, "
          f"median of {args.reps} interleaved repetitions")
    for scene in ("builtin", "grid32"):
        r = Renderer(HostScene.named(scene))
        colours = torch.empty((N, 3), dtype=torch.float32, device="cuda")
        records = torch.empty((N * 12,), dtype=torch.int32, device="cuda")
        out = torch.empty((N, 3), dtype=torch.float32, device="cuda")
        flags = torch.empty((N,), dtype=torch.uint8, device="cuda")
        gbuffer = lambda: r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)
        print(f"\n== {scene} {W}x{H} depth {args.depth}: rt_render_gbuffer_device alone {fmt(timed(gbuffer, args.reps))}")

        # ---- 1. the kernels on their own -----------------------------------------------------------------------------------
        for s in (2, 4):
            Wl, Hl = -(-W // s), -(-H // s)
            cells = torch.empty((Wl * Hl * 12,), dtype=torch.int32, device="cuda")
            lo = torch.rand((Wl * Hl, 3), dtype=torch.float32, device="cuda")
            sub = lambda: capi.check(lib.rt_subsample_hits_device(0, s, 1, W, H, records.data_ptr(), cells.data_ptr(), stream))
            traffic = 48 * N + 12 * N + 12 * N + 12 * Wl * Hl            # records, base, out, values; the shared taps once
            half = torch.empty((traffic // 8,), dtype=torch.int32, device="cuda")
            half2 = torch.empty_like(half)
            fns = {"subsample": sub, "copy": lambda: half2.copy_(half)}
            for lds in (0, 1):
                for plane in (0.0, 0.05):
                    p = upsample_params(s, 3, 3, False, True, plane, 0.0)
                    fns[f"upsample lds={lds} sigma_plane={plane}"] = (
                        lambda p=p, lds=lds: capi.check(lib.rt_internal_upsample_variant(
                            0, C.byref(p), W, H, records.data_ptr(), lo.data_ptr(), colours.data_ptr(), out.data_ptr(),
                            flags.data_ptr(), stream, lds)))
            res = interleaved(fns, args.reps)
            print(f"-- scale {s}: {Wl} x {Hl} cells; the upsample's traffic {traffic / 1e6:.1f} MB (48 N records + 12 N base + 12 N out "
                  f"+ values), the copy moves the same ({traffic / 2e6:.1f} MB read, as many written)")
            for k, t in res.items():
                extra = f"  {traffic / 1e6 / t[0]:8.1f} GB/s" if k != "subsample" else ""
                print(f"   {k:36s} {fmt(t)}{extra}")
            torch.cuda.synchronize()
            print(f"   holes: {int(flags.sum())} of {N} pixels ({100.0 * int(flags.sum()) / N:.3f} %) at sigma_plane 0.05")
            p0 = upsample_params(s, 3, 3, False, True, 0.0, 0.0)
            capi.check(lib.rt_upsample_guided_device(0, C.byref(p0), W, H, records.data_ptr(), lo.data_ptr(), None, out.data_ptr(),
                                                     flags.data_ptr(), stream))
            torch.cuda.synchronize()
            print(f"   holes: {int(flags.sum())} of {N} pixels ({100.0 * int(flags.sum()) / N:.3f} %) without the plane term")
            del cells, lo, half, half2

        # ---- 2. frames -------------------------------------------------------------------------------------------------------
        def indirect_frame(n, s, refine=False):
            kw = dict(samples=n, gather_depth=1, gain=1.0, seed=0)
            gbuffer()
            if s == 1:
                r.indirect_diffuse_device(N, records.data_ptr(), colours.data_ptr(), colours.data_ptr(), stream, **kw)
                return
            st = torch.cuda.current_stream()
            cells, Wl, Hl = r._subsample_device(s, W, H, records, st)
            lo = torch.empty((Wl * Hl, 3), dtype=torch.float32, device="cuda")
            r.indirect_diffuse_device(Wl * Hl, cells.data_ptr(), 0, lo.data_ptr(), stream, **kw)
            up = upsample_params(s, 3, 3, False, True, 0.05, 0.0)
            if not refine:
                r._upsample_device(up, W, H, records, lo, colours, colours, None, st)
                return
            r._upsample_device(up, W, H, records, lo, None, out, flags, st)
            idx = torch.nonzero(flags).reshape(-1)
            if idx.numel():
                holes = records.view(N, 12)[idx].contiguous()
                fine = torch.empty((idx.numel(), 3), dtype=torch.float32, device="cuda")
                r.indirect_diffuse_device(idx.numel(), holes.data_ptr(), 0, fine.data_ptr(), stream, **dict(kw, key0=0x80000000))
                out[idx] = fine
            torch.add(colours, out, out=out)

        def ao_frame(n, s):
            kw = dict(samples=n, radius=1.0, seed=0, channels=1)
            r.render_gbuffer_device(W, H, 0, 0, W, colours.data_ptr(), records.data_ptr(), stream)
            plane = out.view(-1)[:N]
            if s == 1:
                r.ambient_occlusion_device(N, H, records.data_ptr(), plane.data_ptr(), stream=stream, **kw)
                return
            st = torch.cuda.current_stream()
            cells, Wl, Hl = r._subsample_device(s, W, H, records, st)
            lo = torch.empty((Wl * Hl,), dtype=torch.float32, device="cuda")
            r.ambient_occlusion_device(Wl * Hl, Hl, cells.data_ptr(), lo.data_ptr(), stream=stream, **kw)
            r._upsample_device(upsample_params(s, 1, 3, False, False, 0.05, 1.0), W, H, records, lo, None, plane, None, st)

        for n in (2, 4):
            fns = {f"indirect n={n} scale {s}": (lambda n=n, s=s: indirect_frame(n, s)) for s in (1, 2, 4)}
            fns.update({f"indirect n={n} scale {s} refine": (lambda n=n, s=s: indirect_frame(n, s, True)) for s in (2, 4)})
            fns.update({f"ao       n={n} scale {s}": (lambda n=n, s=s: ao_frame(n, s)) for s in (1, 2, 4)})
            res = interleaved(fns, args.reps)
            print(f"-- frames, n = {n} (G-buffer pass included; scale 1 is the full-resolution path)")
            for k, t in res.items():
                print(f"   {k:36s} {fmt(t)}")
        r.close()
        del colours, records, out, flags
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
