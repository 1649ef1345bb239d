"""Cost of the thin-lens camera (include/rt_capi_lens.h) against rt_render_ssaa at the same sample count, W x W frames of the
built-in scene and of the 1024-sphere grid at depth `depth`.

Every call is a device call on the current torch stream, timed by device events around it and a synchronise after it; the calls of
a workload are interleaved -- one round runs each of them once, `warm` rounds first, then `reps` rounds whose medians are printed
-- so that a drift of the machine falls on all of them alike.  Per workload and n = 2, 4:
  ssaa                    rt_render_ssaa_device: the yardstick -- the same sample count, averaged inside the render kernel, no
                          scratch traffic
  pinhole                 rt_render_lens_device at aperture 0, focus 1: the same rays by the batch route
  lens                    rt_render_lens_device at the workload's test aperture and focus (the focal plane among the objects, the
                          lens radius 1 / 20 of its distance, as the tests choose them): the samples of a pixel diverge
with the three stage times of rt_get_lens_info for the two lens calls.

The batch's layout is the library's (RT_LENS_PLANES, csrc/rt_lens.hip): run once with the product library and once with
TCRT_LIBRARY naming a variant built with -DRT_LENS_PLANES=0 (make variant), and pass layout=planes|list to label the output.

usage: lens_gpu.py [W=4096] [depth=4] [reps=7] [warm=2] [workloads=builtin,grid32] [layout=planes] [out=FILE]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)

import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer, capi  # noqa: E402

W, depth = int(opts.get("W", 4096)), int(opts.get("depth", 4))
reps, warm = int(opts.get("reps", 7)), int(opts.get("warm", 2))
workloads = opts.get("workloads", "builtin,grid32").split(",")
layout = opts.get("layout", "planes")
stream = torch.cuda.current_stream().cuda_stream
out = torch.empty((W, W, 3), dtype=torch.float32, device="cuda")
STAGES = ("raygen_ms", "trace_ms", "resolve_ms")
# (aperture, focus): the focal plane through the built-in scene's anchor (0, 1, 1), and 8 screen distances into the sphere grid
LENS = {"builtin": (0.3672383, 7.3447666), "grid32": (0.4, 8.0)}


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def med(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


result = {"W": W, "depth": depth, "reps": reps, "warm": warm, "device": torch.cuda.get_device_name(0),
          "library": capi.library_path(), "layout": layout, "workloads": {}}
for name in workloads:
    r = Renderer(HostScene.named(name))
    aperture, focus = LENS.get(name, (0.4, 8.0))
    calls = {}
    for n in (2, 4):
        calls[f"ssaa{n}"] = lambda n=n: r.render_ssaa_device(W, W, depth, n, 0, W, out.data_ptr(), stream)
        calls[f"pinhole{n}"] = lambda n=n: r.render_lens_device(W, W, depth, 0, W, out.data_ptr(), stream, samples=n)
        calls[f"lens{n}"] = lambda n=n: r.render_lens_device(W, W, depth, 0, W, out.data_ptr(), stream, samples=n,
                                                             aperture=aperture, focus=focus)
    frame = {c: [] for c in calls}
    stages = {c: {s: [] for s in STAGES} for c in calls if not c.startswith("ssaa")}
    chunks = {}
    for rep in range(warm + reps):
        for c, fn in calls.items():
            ms = timed(fn)
            if c in stages:
                i = r.lens_info()
                chunks[c] = int(i.chunks)
                if rep >= warm:
                    for s in STAGES:
                        stages[c][s].append(getattr(i, s))
            if rep >= warm:
                frame[c].append(ms)
    w = {"frame_ms": {c: med(v) for c, v in frame.items()}, "lens": {}, "aperture": aperture, "focus": focus}
    print(f"== {name} {W}x{W} depth {depth}, layout {layout}, aperture {aperture}, focus {focus}", flush=True)
    for n in (2, 4):
        ssaa = w["frame_ms"][f"ssaa{n}"]["median"]
        row = {"ssaa_ms": ssaa}
        for c in (f"pinhole{n}", f"lens{n}"):
            st = {s: statistics.median(stages[c][s]) for s in STAGES}
            row[c] = {"frame_ms": w["frame_ms"][c]["median"], "over_ssaa": w["frame_ms"][c]["median"] / ssaa, "chunks": chunks[c],
                      "stages_ms": st, "trace_over_ssaa": st["trace_ms"] / ssaa}
            print(f"n={n} {c:9s}: frame {row[c]['frame_ms']:9.3f} ms = {row[c]['over_ssaa']:.3f} x ssaa ({ssaa:.3f} ms), "
                  f"{chunks[c]} chunk(s), stages " + ", ".join(f"{s[:-3]} {st[s]:.3f}" for s in STAGES)
                  + f" | trace alone {row[c]['trace_over_ssaa']:.3f} x ssaa", flush=True)
        w["lens"][n] = row
    result["workloads"][name] = w
    del r
if "out" in opts:
    with open(opts["out"], "w") as f:
        json.dump(result, f, indent=1)
