"""What profiles/mirror_compact_experiments.txt records (include/rt_mirror_compact.h): at 4096 x 4096 pixel rays (rt_lens_rays
at one sample, aperture 0, focus 1) on the built-in scene (min_reflective 0.5) and on the mirror room of tests/mirror_scenes.py
(1.0), at max_bounces 1, 4 and 8, with and without out_guide --
  1. rt_mirror_records_compact_device against rt_mirror_records_device, one repetition of each in turn in the same run:
     WALL time, from the call to a drained stream (the compact call waits for its stream once a bounce, and that costs host time
     no event shows), and DEVICE time, the sum of the two stage times of the call's info struct;
  2. the compact call's alive[], rays_queried, queries, syncs and chunks;
  3. its query_ms against rays_queried / n times one query of the pixel rays (what the queries would cost if a query of a dense
     list cost what a query of the pixel rays costs per ray);
  4. the two calls' outputs compared word for word;
  5. the two calls in chunks of the same size, the compact call's default (it is the smaller one: 217 bytes a ray against 128);
  6. the two ways of laying a dense list out for its query (flat; the caller's rows scaled), which needs a build with both:
         make -C tilecoderaytracer_amd/csrc variant NAME=mirror_compact_variants DEFS=-DRT_MIRROR_COMPACT_VARIANTS=1
         TCRT_LIBRARY=tilecoderaytracer_amd/lib/variants/libtcrt_mirror_compact_variants.so python scripts/mirror_compact_experiments.py
One process, nothing downloaded inside a timed window, medians with minimum and maximum of --reps repetitions after a warm-up.
The resource lines of the kernels are the compiler's, made without a GPU (--resources):

    timeout 900 python scripts/mirror_compact_experiments.py [--size 4096] [--reps 11] >> profiles/mirror_compact_experiments.txt
    python scripts/mirror_compact_experiments.py --resources >> profiles/mirror_compact_experiments.txt
"""
import argparse
import ctypes as C
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BOUNCES = (1, 4, 8)
COMPACT_CHUNK = (256 << 20) // 217                # the compact call's default chunk (include/rt_mirror_compact.h)
FLOORS = {"builtin": 0.5, "room": 1.0}           # the built-in scene's half-mirror floor is followed: chains of every length


def resources():
    """the register, LDS and scratch figures of both mirror units' kernels from -Rpass-analysis=kernel-resource-usage, with the
    Makefile's own flags"""
    csrc = os.path.join(ROOT, "tilecoderaytracer_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*:=(.*?)\n\S", mk, flags=re.S | re.M).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    print("# kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, the Makefile's flags, gfx950); in place = rt_mirror.hip's "
          "instantiations of rt_mirror_body.h's step kernel (template arguments FIRST, GUIDE, STAGE, COMPACT), which "
          "profiles/mirror_experiments.txt has at 44 / 38 / 63 / 40 VGPRs, no LDS, no scratch")
    for unit in ("rt_mirror", "rt_mirror_compact"):
        r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull,
                                              unit + ".hip"], cwd=csrc, capture_output=True, text=True, check=True)
        name = None
        for line in r.stderr.splitlines():
            m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                          r"LDS Size \[bytes/block\]): (\S+)", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                if name:
                    print(f"   {unit + '.hip':22s} {name:46s} " + ", ".join(f"{k} {v}" for k, v in got.items()))
                demangled = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip() or m.group(2)
                name, got = re.sub(r"^void |\(.*$", "", demangled), {}
            else:
                got[{"TotalSGPRs": "SGPRs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "waves/SIMD",
                     "LDS Size [bytes/block]": "LDS"}.get(m.group(1), m.group(1))] = m.group(2)
        if name:
            print(f"   {unit + '.hip':22s} {name:46s} " + ", ".join(f"{k} {v}" for k, v in got.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--resources", action="store_true")
    args = ap.parse_args()
    if args.resources:
        return resources()
    import torch
    import mirror_scenes
    from tilecoderaytracer_amd import Renderer, capi
    from tilecoderaytracer_amd.renderer import lens_params

    W = H = args.size
    N = W * H
    lib = capi.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    med = lambda v: f"{statistics.median(v):8.3f} ms (min {min(v):.3f}, max {max(v):.3f})"
    print(f"# compact mirror records against rt_mirror_records_device, {W} x {H} pixel rays, {torch.cuda.get_device_name(0)}; "
          f"median (min, max) of {args.reps} repetitions, one of each call in turn; wall = from the call to a drained stream, "
          f"device = query_ms + step_ms of the call's info struct")
    new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
    for key in ("builtin", "room"):
        r = Renderer(mirror_scenes.host_scene(key))
        floor = FLOORS[key]
        rays, plain = new(N * 6), new(N * 12, torch.int32)
        outs = [[new(N * 12, torch.int32), new(N * 12, torch.int32), new(N * 3), new(N, torch.int32)] for _ in range(2)]
        lens = lens_params(1, 0.0, 1.0, 0)
        capi.check(lib.rt_lens_rays_device(r._cam, W, H, 0, W, C.byref(lens), 0, rays.data_ptr(), stream))

        def mirror(bounces, with_guide, compact, chunk=0):
            hits, guide, weight, path = outs[compact]
            return lambda: r.mirror_records_device(N, H, rays.data_ptr(), hits.data_ptr(), guide.data_ptr() if with_guide else 0,
                                                   weight.data_ptr(), path.data_ptr(), stream, max_bounces=bounces,
                                                   min_reflective=floor, chunk_rays=chunk, compact=bool(compact))

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        # one query of the pixel rays, device time
        one = []
        for rep in range(args.reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            r.intersect_rays_device(N, H, rays.data_ptr(), plain.data_ptr(), stream)
            b.record()
            torch.cuda.synchronize()
            if rep >= 2:
                one.append(a.elapsed_time(b))
        print(f"\n== {key} {W}x{H}, min_reflective {floor}: one rt_intersect_rays_device of the pixel rays {med(one)}")
        for bounces in BOUNCES:
            for with_guide in (True, False):
                fns = [mirror(bounces, with_guide, 0), mirror(bounces, with_guide, 1)]
                for fn in fns:                                                 # warm-up: scratch grown, pinned word made
                    fn(), fn()
                walls, devs, parts = ([], []), ([], []), ([], [])
                for _ in range(args.reps):
                    for c, fn in enumerate(fns):
                        walls[c].append(wall(fn))
                        info = r.mirror_compact_info() if c else r.mirror_info()
                        devs[c].append(info.query_ms + info.step_ms)
                        parts[c].append((info.query_ms, info.step_ms))
                same = all(bool(torch.equal(x, y)) for x, y, keep in zip(outs[0], outs[1], (1, with_guide, 1, 1)) if keep)
                info = r.mirror_compact_info()
                alive = list(info.alive)[:bounces + 1]
                model = info.rays_queried / N * statistics.median(one)
                q = [statistics.median([p[0] for p in parts[c]]) for c in (0, 1)]
                s = [statistics.median([p[1] for p in parts[c]]) for c in (0, 1)]
                print(f"   max_bounces {bounces} {'with   ' if with_guide else 'without'} out_guide: outputs {'identical' if same else 'DIFFER'}")
                print(f"      wall    existing {med(walls[0])}   compact {med(walls[1])}   existing / compact "
                      f"{statistics.median(walls[0]) / statistics.median(walls[1]):5.2f} x")
                print(f"      device  existing {med(devs[0])}   compact {med(devs[1])}   existing / compact "
                      f"{statistics.median(devs[0]) / statistics.median(devs[1]):5.2f} x")
                print(f"      existing: query_ms {q[0]:.3f}, step_ms {s[0]:.3f}, queries {r.mirror_info().queries}, chunks "
                      f"{r.mirror_info().chunks};  compact: query_ms {q[1]:.3f}, step_ms {s[1]:.3f} (count, scan and step), queries "
                      f"{info.queries}, syncs {info.syncs}, chunks {info.chunks}")
                print(f"      alive[0..{bounces}] " + " ".join(f"{100.0 * a / N:.2f}%" for a in alive) +
                      f";  rays_queried / n = {info.rays_queried / N:.3f} (the existing call: {bounces + 1});  "
                      f"query_ms {q[1]:.3f} against {info.rays_queried / N:.3f} x one query = {model:.3f} ms: {q[1] / model:4.2f} x;  "
                      f"wall - device = {statistics.median(walls[1]) - statistics.median(devs[1]):.3f} ms over {info.syncs} waits")
        # ---- the two calls in chunks of the same size -----------------------------------------------------------------------------
        for bounces in BOUNCES:
            fns = [mirror(bounces, True, 0, COMPACT_CHUNK), mirror(bounces, True, 1, COMPACT_CHUNK)]
            for fn in fns:
                fn()
            walls = ([], [])
            for _ in range(args.reps):
                for c, fn in enumerate(fns):
                    walls[c].append(wall(fn))
            print(f"   max_bounces {bounces} with out_guide, both calls with chunk_rays {COMPACT_CHUNK} ({r.mirror_info().chunks} chunks): "
                  f"wall existing {med(walls[0])}   compact {med(walls[1])}   existing / compact "
                  f"{statistics.median(walls[0]) / statistics.median(walls[1]):5.2f} x")

        # ---- the two layouts of a dense list's query ---------------------------------------------------------------------------
        if hasattr(lib, "rt_internal_mirror_compact_variant"):
            lib.rt_internal_mirror_compact_variant.argtypes = [C.c_int]
            own = lib.rt_internal_mirror_compact_variant(0)
            for bounces in BOUNCES:
                fn = mirror(bounces, True, 1)
                times = {0: [], 1: []}
                for v in (0, 1):
                    lib.rt_internal_mirror_compact_variant(v)
                    fn()
                for _ in range(args.reps):
                    for v in (0, 1):
                        lib.rt_internal_mirror_compact_variant(v)
                        w = wall(fn)
                        times[v].append((w, r.mirror_compact_info().query_ms))
                mirror(bounces, True, 0)()                                     # the existing call's words, to compare with
                torch.cuda.synchronize()
                same = all(bool(torch.equal(x, y)) for x, y in zip(outs[0], outs[1]))
                for v, name in ((0, "flat (rows = the list's length)"), (1, "the caller's rows scaled by the share alive")):
                    print(f"   max_bounces {bounces} with out_guide, dense lists queried {name:44s}: wall {med([t[0] for t in times[v]])}, "
                          f"query_ms {med([t[1] for t in times[v]])}" + ("" if same else "  OUTPUTS DIFFER"))
            lib.rt_internal_mirror_compact_variant(own)
        r.close()
        del rays, plain, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
