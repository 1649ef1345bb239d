"""What profiles/mirror_experiments.txt records (include/rt_mirror.h): at 4096 x 4096 pixel rays (rt_lens_rays at one sample,
aperture 0, focus 1) on the built-in scene and on the mirror room of tests/mirror_scenes.py --
  1. rt_mirror_records_device at max_bounces 1, 4 and 8 against max_bounces + 1 runs of rt_intersect_rays_device on the same
     rays in the same run (the excess is the step kernels and the degenerate rays), with and without out_guide;
  2. the call's step_ms (rt_mirror_info) against a device copy of the bytes its step kernels move, counted from the shares of
     rays alive at each bounce;
  3. the two ways of reading the 48-byte records (three 16-byte loads a lane; through LDS), which needs a build with both:
         make -C tilecoderaytracer_amd/csrc variant NAME=mirror_variants DEFS=-DRT_MIRROR_VARIANTS=1
         TCRT_LIBRARY=tilecoderaytracer_amd/lib/variants/libtcrt_mirror_variants.so python scripts/mirror_experiments.py
  4. the share of rays still alive at each bounce (what a compacting variant would save);
and, with --deviation, on the CPU alone (tests/mirror_ref.py, 96 x 80 and 256 x 256): the share of pixels whose terminal object
changes when the chain follows normalize(r), as calculatePixel's Ray(P, r) does, and not normalize((P + r) - P).
Every time is device time between events around one device call, the median, minimum and maximum of --reps interleaved
repetitions after a warm-up; one process, nothing downloaded inside a timed window.

    timeout 900 python scripts/mirror_experiments.py [--size 4096] [--reps 11] >> profiles/mirror_experiments.txt
    python scripts/mirror_experiments.py --deviation >> profiles/mirror_experiments.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BOUNCES = (1, 4, 8)
FLOORS = {"builtin": 0.5, "room": 1.0}           # the built-in scene's half-mirror floor is followed: chains of every length


def deviation():
    import mirror_ref
    import mirror_scenes
    print("# the header's stated deviation (tests/mirror_ref.py on the CPU): pixels whose terminal object differs when ray k + 1 "
          "follows normalize(r) and not normalize((P + r) - P); max_bounces 8")
    for key in ("builtin", "room"):
        for W, H in ((96, 80), (256, 256)):
            rays = mirror_scenes.pixel_rays(key, W, H)
            for floor in (1.0, 0.5):
                own = mirror_ref.records(mirror_scenes.ref_scene(key), rays, 8, floor)
                other = mirror_ref.records(mirror_scenes.ref_scene(key), rays, 8, floor, follow_r=True)
                followed = mirror_ref.unpack(own[3])[0] >= 1
                differ = own[0]["object"] != other[0]["object"]
                bits = (own[0]["point"].view(np.uint32) != other[0]["point"].view(np.uint32)).any(-1)
                print(f"   {key:8s} {W:3d} x {H:3d} min_reflective {floor}: {int(followed.sum()):6d} of {W * H} pixels follow a mirror; "
                      f"terminal object differs at {int(differ.sum())} ({100.0 * differ.sum() / (W * H):.3f} % of the frame), "
                      f"terminal point differs in some bit at {int(bits.sum())}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--deviation", action="store_true")
    args = ap.parse_args()
    if args.deviation:
        return deviation()
    import torch
    import mirror_scenes
    from temporal_experiments import fmt, interleaved
    from tilecoderaytracer_amd import Renderer, capi
    from tilecoderaytracer_amd.renderer import lens_params

    W = H = args.size
    N = W * H
    lib = capi.load_library()
    variants = hasattr(lib, "rt_internal_mirror_variant")
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# mirror records, {W} x {H} pixel rays, {torch.cuda.get_device_name(0)}; device time between events, median (min, max) "
          f"of {args.reps} interleaved repetitions; " +
          ("both record loads" if variants else "the library's own record load only (no -DRT_MIRROR_VARIANTS=1 build)"))
    new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
    for key in ("builtin", "room"):
        r = Renderer(mirror_scenes.host_scene(key))
        floor = FLOORS[key]
        rays, plain = new(N * 6), new(N * 12, torch.int32)
        hits, guide, weight, path = new(N * 12, torch.int32), new(N * 12, torch.int32), new(N * 3), new(N, torch.int32)
        lens = lens_params(1, 0.0, 1.0, 0)
        capi.check(lib.rt_lens_rays_device(r._cam, W, H, 0, W, C.byref(lens), 0, rays.data_ptr(), stream))

        def mirror(bounces, with_guide=True):
            return lambda: r.mirror_records_device(N, H, rays.data_ptr(), hits.data_ptr(), guide.data_ptr() if with_guide else 0,
                                                   weight.data_ptr(), path.data_ptr(), stream, max_bounces=bounces,
                                                   min_reflective=floor)

        def queries(count):
            def run():
                for _ in range(count):
                    r.intersect_rays_device(N, H, rays.data_ptr(), plain.data_ptr(), stream)
            return run

        # ---- 4. the rays alive at each bounce (first: the traffic below is counted from it) ------------------------------------
        mirror(8)()
        torch.cuda.synchronize()
        k = path & 0xff
        alive = [int((k >= b).sum()) for b in range(10)]
        cut = int(((path >> 8) & 1).sum())
        print(f"\n== {key} {W}x{H}, min_reflective {floor}: rays alive at bounce 0..8 (max_bounces 8): " +
              " ".join(f"{100.0 * a / N:.2f}%" for a in alive[:9]) + f"; cut at 8: {100.0 * cut / N:.3f}%")

        # ---- 1. the call against max_bounces + 1 queries ----------------------------------------------------------------------
        fns = {"   the same without out_guide": mirror(BOUNCES[0], False)}
        for b in BOUNCES:
            fns[f"rt_mirror_records_device max_bounces {b}"] = mirror(b)
            fns[f"{b + 1} x rt_intersect_rays_device"] = queries(b + 1)
        res = interleaved(fns, args.reps)
        for b in BOUNCES:
            t, q = res[f"rt_mirror_records_device max_bounces {b}"], res[f"{b + 1} x rt_intersect_rays_device"]
            print(f"   max_bounces {b}: the call {fmt(t)};  {b + 1} queries of the pixel rays {fmt(q)};  {t[0] / q[0]:5.3f} x")
        print(f"   max_bounces {BOUNCES[0]} without out_guide: {fmt(res['   the same without out_guide'])}")

        # ---- 2. step_ms and query_ms, and the copy of the steps' bytes -----------------------------------------------------------
        for b in BOUNCES:
            for with_guide in (True, False):
                # a ray alive at bounce s reads its record, its ray and (s > 0) its state; one that goes on writes its ray and
                # state, one that ends writes its outputs and, before the last bounce, its zero ray and word; a retired ray's
                # lane reads its word
                state = 56 if with_guide else 16
                out = 48 + 12 + 4 + (48 if with_guide else 0)
                a = [int((k >= s).sum()) for s in range(b + 2)]
                a[b + 1] = 0                                                     # (nobody goes on from the last bounce)
                traffic = 0
                for s in range(b + 1):
                    traffic += a[s] * (48 + 24 + (state if s else 0)) + (N - a[s]) * 4
                    traffic += a[s + 1] * (24 + state) + (a[s] - a[s + 1]) * (out + (28 if s < b else 0))
                half, half2 = new(traffic // 8, torch.int32), new(traffic // 8, torch.int32)
                steps, qs = [], []
                fn = mirror(b, with_guide)
                fn()
                copy = interleaved({"copy": lambda: half2.copy_(half)}, args.reps)["copy"]
                for _ in range(args.reps):
                    fn()
                    info = r.mirror_info()
                    steps.append(info.step_ms), qs.append(info.query_ms)
                print(f"   max_bounces {b} {'with   ' if with_guide else 'without'} out_guide: step_ms {statistics.median(steps):8.3f} "
                      f"(min {min(steps):.3f}, max {max(steps):.3f}), query_ms {statistics.median(qs):8.3f}; the steps move "
                      f"{traffic / 1e6:8.1f} MB, a device copy of as many bytes {fmt(copy)}: {statistics.median(steps) / copy[0]:5.2f} x")
                del half, half2

        # ---- 3. the two record loads ---------------------------------------------------------------------------------------------
        if variants:
            lib.rt_internal_mirror_variant.argtypes = [C.c_int]

            def variant(stage, bounces, with_guide):
                fn = mirror(bounces, with_guide)

                def run():
                    lib.rt_internal_mirror_variant(stage)
                    fn()
                    return r.mirror_info().step_ms
                return run

            own = lib.rt_internal_mirror_variant(0)
            cases = {(stage, g): variant(stage, 4, g) for g in (True, False) for stage in (0, 1)}
            times = {c: [] for c in cases}
            for c, fn in cases.items():
                fn()
            for _ in range(args.reps):
                for c, fn in cases.items():
                    times[c].append(fn())
            lib.rt_internal_mirror_variant(own)
            for (stage, g), v in times.items():
                print(f"   max_bounces 4, {'with   ' if g else 'without'} out_guide, records {'through LDS      ' if stage else 'as 3 x 16-byte loads'}: "
                      f"step_ms {statistics.median(v):8.3f} (min {min(v):.3f}, max {max(v):.3f})")
        r.close()
        del rays, plain, hits, guide, weight, path
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
