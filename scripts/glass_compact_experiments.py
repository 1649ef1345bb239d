"""What profiles/glass_compact_experiments.txt records (include/rt_glass_compact.h): at 4096 x 4096 pixel rays (rt_lens_rays at
one sample, aperture 0, focus 1) on the glass room of tests/glass_scenes.py (min_reflective 1.0, min_transmissive 0.5) and on the
built-in scene with its half-mirror floor followed (min_reflective 0.5; it has no glass: the mirror chain through this call), at
max_bounces 1, 4 and 8 with every output --
  1. rt_glass_records_compact_device against rt_glass_records_device, one repetition of each in turn in the same run:
     WALL time, from the call to a drained stream (the compact call waits for its stream once a bounce, and that costs host time
     no event shows), and DEVICE time, the sum of the two stage times of the call's info struct;
  2. the compact call's alive[], rays_queried against (max_bounces + 1) n, queries, syncs and chunks;
  3. the two calls' outputs compared word for word;
  4. each stream wait's cost: (wall - device) / syncs;
  5. the two calls in chunks of the same size, the compact call's default (it is the smaller one: 217 bytes a ray against 128);
  6. a device-to-device copy of 72 bytes per counted entry (the cache lines the count kernel can touch: an entry's 48-byte record
     and a candidate's 24-byte ray), timed by two events: what the count kernel's traffic is worth;
  7. (--kernels) the kernels' own times, from a child process of this script under rocprofv3 --kernel-trace --stats: the count
     kernel against that copy, the scan, the step, the hit queries.
One process, nothing downloaded inside a timed window, medians with the interquartile range of --reps repetitions after a warm-up.
The resource lines of the kernels are the compiler's, made without a GPU (--resources):

    timeout 900 python scripts/glass_compact_experiments.py [--size 4096] [--reps 11] >> profiles/glass_compact_experiments.txt
    timeout 600 python scripts/glass_compact_experiments.py --kernels >> profiles/glass_compact_experiments.txt
    python scripts/glass_compact_experiments.py --resources >> profiles/glass_compact_experiments.txt
"""
import argparse
import ctypes as C
import csv
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BOUNCES = (1, 4, 8)
COMPACT_CHUNK = (256 << 20) // 217                # the compact call's default chunk (include/rt_glass_compact.h)
SCENES = {"glass": (1.0, 0.5), "builtin": (0.5, 0.5)}     # key: (min_reflective, min_transmissive)
COUNTED_BYTES = 72                                # an entry's record and its ray


def resources():
    """the register, LDS and scratch figures of both glass units' kernels from -Rpass-analysis=kernel-resource-usage, with the
    Makefile's own flags"""
    csrc = os.path.join(ROOT, "tilecoderaytracer_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^HIPFLAGS\s*:=(.*?)\n\S", mk, flags=re.S | re.M).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    print("# kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, the Makefile's flags, gfx950); template arguments "
          "FIRST, GUIDE; the LDS of the new kernels is rt_scan_rank's four words")
    for unit in ("rt_glass", "rt_glass_compact"):
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


def renderer_of(key):
    import glass_scenes
    import mirror_scenes
    from tilecoderaytracer_amd import Renderer
    if key == "builtin":
        return Renderer(mirror_scenes.host_scene("builtin"))
    from test_refract_gpu import make
    from test_texture_gpu import Desc
    host, refr = glass_scenes.host_scene(key)
    return make(Desc(host), refractive=refr)


def kernels(args):
    """the kernels' own times: this script's --plain mode (the compact call alone, the glass room, max_bounces 8, three times
    after a warm-up) as a child process under rocprofv3 --kernel-trace --stats"""
    with tempfile.TemporaryDirectory() as out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "--output-format", "csv", "--", sys.executable,
               os.path.abspath(__file__), "--plain", "--size", str(args.size)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        found = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not found:
            print(f"# --kernels: not measured (rocprofv3 exit {r.returncode}, {len(found)} stats files)\n" + r.stderr[-600:])
            return
        print(f"# the kernels of rt_glass_records_compact_device on the glass room, {args.size} x {args.size}, max_bounces 8, with "
              f"out_guide; rocprofv3 --kernel-trace --stats over 1 warm-up and 3 timed calls (4 calls in all): calls, total ms, "
              f"average us\n" + "".join("#   " + line + "\n" for line in r.stdout.splitlines() if line.startswith("plain:")), end="")
        for row in csv.DictReader(open(found[0])):
            name = row.get("Name", "")
            if re.search(r"glass_compact|rt_scan_|hits|copy|Copy", name):
                short = re.sub(r"\(.*$", "", name)[:70]
                print(f"   {short:70s} calls {row.get('Calls'):>5s}  total {float(row.get('TotalDurationNs', 0)) / 1e6:9.3f} ms  "
                      f"average {float(row.get('AverageNs', 0)) / 1e3:9.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--plain", action="store_true")
    args = ap.parse_args()
    if args.resources:
        return resources()
    if args.kernels:
        return kernels(args)
    import torch
    from tilecoderaytracer_amd import capi
    from tilecoderaytracer_amd.renderer import lens_params

    W = H = args.size
    N = W * H
    lib = capi.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    quart = lambda v: statistics.quantiles(v, n=4) if len(v) >= 2 else [v[0]] * 3
    med = lambda v: f"{statistics.median(v):8.3f} ms (IQR {quart(v)[0]:.3f} .. {quart(v)[2]:.3f})"
    new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
    lens = lens_params(1, 0.0, 1.0, 0)

    if args.plain:                                                            # --kernels' child: the compact call alone
        r = renderer_of("glass")
        rays = new(N * 6)
        hits, guide, weight, path = new(N * 12, torch.int32), new(N * 12, torch.int32), new(N * 3), new(N, torch.int32)
        capi.check(lib.rt_lens_rays_device(r._cam, W, H, 0, W, C.byref(lens), 0, rays.data_ptr(), stream))
        for _ in range(4):
            r.glass_records_device(N, H, rays.data_ptr(), hits.data_ptr(), guide.data_ptr(), weight.data_ptr(), path.data_ptr(), stream,
                                   max_bounces=8, min_reflective=1.0, min_transmissive=0.5, compact=True)
            torch.cuda.synchronize()
        info = r.glass_compact_info()
        counted = sum(list(info.alive)[:8])
        src, dst = new(counted * COUNTED_BYTES // 4, torch.int32), new(counted * COUNTED_BYTES // 4, torch.int32)
        for _ in range(4):
            dst.copy_(src)
        torch.cuda.synchronize()
        print(f"plain: alive {list(info.alive)[:9]}, entries counted per call {counted}; the copy kernel below moves "
              f"{counted * COUNTED_BYTES / 1e6:.1f} MB, 4 times")
        r.close()
        return

    print(f"# compact glass records against rt_glass_records_device, {W} x {H} pixel rays, {torch.cuda.get_device_name(0)}; "
          f"median (interquartile range) of {args.reps} repetitions, one of each call in turn; wall = from the call to a drained "
          f"stream, device = query_ms + step_ms of the call's info struct; every ratio is against the in-place call of this run")
    for key, (floor, look) in SCENES.items():
        r = renderer_of(key)
        rays = new(N * 6)
        outs = [[new(N * 12, torch.int32), new(N * 12, torch.int32), new(N * 3), new(N, torch.int32)] for _ in range(2)]
        capi.check(lib.rt_lens_rays_device(r._cam, W, H, 0, W, C.byref(lens), 0, rays.data_ptr(), stream))

        def glass(bounces, compact, chunk=0):
            hits, guide, weight, path = outs[compact]
            return lambda: r.glass_records_device(N, H, rays.data_ptr(), hits.data_ptr(), guide.data_ptr(), weight.data_ptr(),
                                                  path.data_ptr(), stream, max_bounces=bounces, min_reflective=floor,
                                                  min_transmissive=look, chunk_rays=chunk, compact=bool(compact))

        def wall(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        print(f"\n== {key} {W}x{H}, min_reflective {floor}, min_transmissive {look}")
        for bounces in BOUNCES:
            fns = [glass(bounces, 0), glass(bounces, 1)]
            for fn in fns:                                                     # warm-up: scratch grown, pinned word made
                fn(), fn()
            walls, devs, parts = ([], []), ([], []), ([], [])
            for _ in range(args.reps):
                for c, fn in enumerate(fns):
                    walls[c].append(wall(fn))
                    info = r.glass_compact_info() if c else r.glass_info()
                    devs[c].append(info.query_ms + info.step_ms)
                    parts[c].append((info.query_ms, info.step_ms))
            same = all(bool(torch.equal(x, y)) for x, y in zip(outs[0], outs[1]))
            info = r.glass_compact_info()
            alive = list(info.alive)[:bounces + 1]
            q = [statistics.median([p[0] for p in parts[c]]) for c in (0, 1)]
            s = [statistics.median([p[1] for p in parts[c]]) for c in (0, 1)]
            w, d = [statistics.median(walls[c]) for c in (0, 1)], [statistics.median(devs[c]) for c in (0, 1)]
            lost = "   THE COMPACT CALL LOSES HERE" if w[1] > w[0] else ""
            print(f"   max_bounces {bounces}: outputs {'identical' if same else 'DIFFER'}{lost}")
            print(f"      wall    in place {med(walls[0])}   compact {med(walls[1])}   in place / compact {w[0] / w[1]:5.2f} x")
            print(f"      device  in place {med(devs[0])}   compact {med(devs[1])}   in place / compact {d[0] / d[1]:5.2f} x")
            print(f"      in place: query_ms {q[0]:.3f}, step_ms {s[0]:.3f}, queries {r.glass_info().queries}, chunks "
                  f"{r.glass_info().chunks};  compact: query_ms {q[1]:.3f}, step_ms {s[1]:.3f} (count, scan and step), queries "
                  f"{info.queries}, syncs {info.syncs}, chunks {info.chunks}")
            print(f"      alive[0..{bounces}] " + " ".join(f"{100.0 * a / N:.2f}%" for a in alive) +
                  f";  rays_queried {info.rays_queried} = {info.rays_queried / N:.3f} n against ({bounces} + 1) n = "
                  f"{(bounces + 1) * N};  wall - device = {w[1] - d[1]:.3f} ms over {info.syncs} waits = "
                  f"{(w[1] - d[1]) / max(info.syncs, 1):.3f} ms a wait")
            counted = sum(alive[:bounces])
            src, dst = new(counted * COUNTED_BYTES // 4, torch.int32), new(counted * COUNTED_BYTES // 4, torch.int32)
            copies = []
            for rep in range(args.reps + 2):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                dst.copy_(src)
                b.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    copies.append(a.elapsed_time(b))
            print(f"      the count pass ran over {counted} entries; a device copy of {COUNTED_BYTES} bytes an entry "
                  f"({counted * COUNTED_BYTES / 1e6:.1f} MB read and as many written): {med(copies)};  compact step_ms - in-place "
                  f"step_ms = {s[1] - s[0]:.3f} ms")
            del src, dst
        # ---- the two calls in chunks of the same size ---------------------------------------------------------------------------
        for bounces in BOUNCES:
            fns = [glass(bounces, 0, COMPACT_CHUNK), glass(bounces, 1, COMPACT_CHUNK)]
            for fn in fns:
                fn()
            walls = ([], [])
            for _ in range(args.reps):
                for c, fn in enumerate(fns):
                    walls[c].append(wall(fn))
            print(f"   max_bounces {bounces}, both calls with chunk_rays {COMPACT_CHUNK} ({r.glass_info().chunks} chunks): "
                  f"wall in place {med(walls[0])}   compact {med(walls[1])}   in place / compact "
                  f"{statistics.median(walls[0]) / statistics.median(walls[1]):5.2f} x")
        r.close()
        del rays, outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
