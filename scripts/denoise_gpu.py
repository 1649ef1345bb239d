"""Cost and gain of the denoiser (include/rt_capi_denoise.h) on the built-in scene, both lights area lights of radius 1.0
(include/rt_capi_soft.h), W x W at depth `depth`:

  time (default)  kernel ms of the G-buffer render at n = 1, 2, 4, 8 samples a side (rt_get_timing, median of `reps` launches
                  after a warm-up); ms of rt_denoise_device at iterations 1..4 on the n = 1 frame (device events around the
                  call, median of `reps`), with the algorithmic bytes per iteration -- 12 B read + 32 B of packed guide + 12 B
                  written per pixel -- over that time as a share of 6.3 TB/s; PSNR against the n = 8 frame (seed 2; the others
                  seed 1) of every n, unfiltered and filtered at iterations 1..4.  Writes the table as JSON to `out`.
  pmc             one render and `reps` filters of `iterations` iterations and nothing else, for a counter run of its own:
                  rocprofv3 --pmc FETCH_SIZE -- python scripts/denoise_gpu.py mode=pmc   (and WRITE_SIZE in another run)
  counters        sum a rocprofv3 counter CSV (csv=...) per kernel name

usage: denoise_gpu.py [mode=time] [W=4096] [depth=4] [reps=15] [iterations=3] [sigma=1.0] [squarings=3] [out=FILE] [csv=FILE]"""
import csv
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
mode = opts.get("mode", "time")

if mode == "counters":
    total = {}
    with open(opts["csv"]) as f:
        for row in csv.DictReader(f):
            key = (row["Kernel_Name"].split("(")[0], row["Counter_Name"])
            n, v = total.get(key, (0, 0.0))
            total[key] = (n + 1, v + float(row["Counter_Value"]))
    for (kernel, counter), (n, v) in sorted(total.items()):
        print(f"{kernel:60s} {counter:12s} dispatches {n:4d} sum {v:.6g} per dispatch {v / n:.6g}")
    sys.exit(0)

import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer, capi  # noqa: E402

W, depth, reps = int(opts.get("W", 4096)), int(opts.get("depth", 4)), int(opts.get("reps", 15))
sigma, squarings = float(opts.get("sigma", 1.0)), int(opts.get("squarings", 3))
lib = capi.load_library()
stream = torch.cuda.current_stream().cuda_stream
pixels = W * W


def renderer(n, seed):
    host = HostScene.builtin()
    d = host.desc.contents
    for k in range(d.n_objects):
        if d.objects[k].is_light:
            host.set_area_light(k, n, 1.0)
    r = Renderer(host)
    r.set_shadow_seed(seed)
    return r


def filter_device(iterations, d_rgb, d_hits, d_out, d_scratch):
    params = capi.RtDenoiseParams(iterations, squarings, sigma)
    capi.check(lib.rt_denoise_device(0, C.byref(params), W, W, d_rgb.data_ptr(), d_hits.data_ptr(), d_out.data_ptr(),
                                     d_scratch.data_ptr(), stream))


def psnr(a, b):
    return float(10.0 * torch.log10(1.0 / torch.mean((a.double() - b.double()) ** 2)))


d_hits = torch.empty((pixels * 12,), dtype=torch.int32, device="cuda")
d_out = torch.empty((W, W, 3), dtype=torch.float32, device="cuda")
nbytes = lib.rt_denoise_scratch_bytes(C.byref(capi.RtDenoiseParams(5, squarings, sigma)), W, W)
d_scratch = torch.empty((nbytes // 4 + 4,), dtype=torch.int32, device="cuda")

if mode == "pmc":
    iterations = int(opts.get("iterations", 3))
    d_rgb = torch.empty((W, W, 3), dtype=torch.float32, device="cuda")
    renderer(1, 1).render_gbuffer_device(W, W, depth, 0, W, d_rgb.data_ptr(), d_hits.data_ptr(), stream)
    for _ in range(reps):
        filter_device(iterations, d_rgb, d_hits, d_out, d_scratch)
    torch.cuda.synchronize()
    sys.exit(0)

result = {"W": W, "depth": depth, "radius": 1.0, "sigma_color": sigma, "normal_squarings": squarings, "reps": reps,
          "device": torch.cuda.get_device_name(0), "render_ms": {}, "denoise_ms": {}, "psnr_db": {}}
frames = {}
for n, seed in ((1, 1), (2, 1), (4, 1), (8, 2)):
    r = renderer(n, seed)
    frames[n] = torch.empty((W, W, 3), dtype=torch.float32, device="cuda")
    times = []
    for k in range(2 + (reps if n < 8 else max(reps // 5, 2))):          # two warm-up frames; the 64-sample frame is long
        r.render_gbuffer_device(W, W, depth, 0, W, frames[n].data_ptr(), d_hits.data_ptr(), stream)
        torch.cuda.synchronize()
        if k >= 2:
            times.append(r.timing().last_kernel_ms)
    result["render_ms"][n] = {"median": statistics.median(times), "min": min(times), "max": max(times), "launches": len(times),
                              "kernel": r.kernel_name()}
    print(f"render n={n}: {result['render_ms'][n]}", flush=True)
    assert bool(torch.isfinite(frames[n]).all())

# (d_hits: the camera rays' records, the same for every n)
for iterations in (1, 2, 3, 4):
    times = []
    for k in range(3 + reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        filter_device(iterations, frames[1], d_hits, d_out, d_scratch)
        stop.record()
        torch.cuda.synchronize()
        if k >= 3:
            times.append(start.elapsed_time(stop))
    med = statistics.median(times)
    algorithmic = pixels * (48 + 32) + iterations * pixels * (12 + 32 + 12)          # the pack, then each iteration
    result["denoise_ms"][iterations] = {"median": med, "min": min(times), "max": max(times), "launches": len(times),
                                        "algorithmic_bytes": algorithmic,
                                        "share_of_6.3TBps": algorithmic / (med * 1e-3) / 6.3e12}
    print(f"denoise iterations={iterations}: {result['denoise_ms'][iterations]}", flush=True)

for n in (1, 2, 4):
    row = {"unfiltered": psnr(frames[n], frames[8])}
    for iterations in (1, 2, 3, 4):
        filter_device(iterations, frames[n], d_hits, d_out, d_scratch)
        torch.cuda.synchronize()
        row[f"iterations_{iterations}"] = psnr(d_out, frames[8])
    result["psnr_db"][n] = row
    print(f"PSNR against n=8, n={n}: {row}", flush=True)
row = {}
for iterations in (1, 2, 3, 4):                       # the filter's own bias: the 64-sample frame against itself filtered
    filter_device(iterations, frames[8], d_hits, d_out, d_scratch)
    torch.cuda.synchronize()
    row[f"iterations_{iterations}"] = psnr(d_out, frames[8])
result["psnr_db"]["8_filtered_against_8"] = row
print(f"PSNR of the filtered n=8 frame against itself: {row}", flush=True)
if "out" in opts:
    with open(opts["out"], "w") as f:
        json.dump(result, f, indent=1)
