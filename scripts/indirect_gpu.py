"""Cost of one diffuse bounce (include/rt_capi_indirect.h) over the direct frame, W x W frames of the built-in scene and of the
1024-sphere grid at depth `depth`, and each of its stages against the floor it cannot beat.

Every call is a device call on the current torch stream, timed by device events around it and a synchronise after it; the calls of
a workload are interleaved -- one round runs each of them once, `warm` rounds first, then `reps` rounds whose medians are printed
-- so that a drift of the machine falls on all of them alike.  Per workload:
  gbuffer                 rt_render_gbuffer_device alone: the direct frame and its records, what a bounce is added to
and per n = 2, 4:
  lens raygen / resolve   rt_lens_rays_device of the whole frame (the same ray count, 24 bytes a ray and no record to read) and the
                          resolve stage of rt_render_lens_device at aperture 0 (rt_get_lens_info)
  rays                    rt_indirect_rays_device of the whole frame's records: this unit's ray generation in one launch
and per gather depth 1, 2 and emitters 0, 1:
  indirect                rt_indirect_diffuse_device on the frame's records, the frame's colours the base, with the four stage times
                          of rt_get_indirect_info
  floor                   rt_trace_rays_device of the same rays (those `rays` left in its buffer), called directly in chunks of
                          the size the call used: what the trace stage cannot beat

usage: indirect_gpu.py [W=4096] [depth=4] [reps=5] [warm=2] [workloads=builtin,grid32] [out=FILE]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)

import ctypes as C  # noqa: E402

import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer, capi  # noqa: E402
from tilecoderaytracer_amd.renderer import indirect_params, lens_params  # noqa: E402

W, depth = int(opts.get("W", 4096)), int(opts.get("depth", 4))
reps, warm = int(opts.get("reps", 5)), int(opts.get("warm", 2))
workloads = opts.get("workloads", "builtin,grid32").split(",")
NS, DEPTHS, EMITTERS = (2, 4), (1, 2), (0, 1)
N = W * W
lib = capi.load_library()
stream = torch.cuda.current_stream().cuda_stream
colours = torch.empty((W, W, 3), dtype=torch.float32, device="cuda")
records = torch.empty((N * 12,), dtype=torch.int32, device="cuda")
out = torch.empty((W, W, 3), dtype=torch.float32, device="cuda")
rays = torch.empty((N * max(NS) ** 2 * 6,), dtype=torch.float32, device="cuda")
STAGES = ("raygen_ms", "trace_ms", "query_ms", "resolve_ms")


def default_chunk(n, emitters):
    """the library's default chunk_records (include/rt_capi_indirect.h, SCRATCH)"""
    return max(1, (256 << 20) // (n * n * (36 if emitters else 84)))


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def med(values):
    return statistics.median(values)


result = {"W": W, "depth": depth, "reps": reps, "warm": warm, "device": torch.cuda.get_device_name(0), "workloads": {}}
for name in workloads:
    host = HostScene.named(name)
    r = Renderer(host)
    sample_colours = torch.empty((default_chunk(min(NS), 1) * min(NS) ** 2 * 3,), dtype=torch.float32, device="cuda")

    def gbuffer():
        r.render_gbuffer_device(W, W, depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)

    def own_rays(n):
        p = indirect_params(n)
        capi.check(lib.rt_indirect_rays_device(C.byref(p), N, records.data_ptr(), 0, rays.data_ptr(), stream))

    def lens_rays(n):
        p = lens_params(n)
        capi.check(lib.rt_lens_rays_device(host.camera, W, W, 0, W, C.byref(p), 0, rays.data_ptr(), stream))

    def indirect(n, gd, em):
        r.indirect_diffuse_device(N, records.data_ptr(), colours.data_ptr(), out.data_ptr(), stream, samples=n, gather_depth=gd,
                                  emitters=bool(em))

    def floor(n, gd, em):
        S, chunk = n * n, default_chunk(n, em)
        for i0 in range(0, N, chunk):
            m = min(chunk, N - i0) * S
            r.trace_rays_device(m, m, rays.data_ptr() + i0 * S * 24, gd, sample_colours.data_ptr(), stream)

    t = {"gbuffer": [], **{f"{k}{n}": [] for n in NS for k in ("rays", "lens_rays", "lens_resolve")}}
    cfg = [(n, gd, em) for n in NS for gd in DEPTHS for em in EMITTERS]
    t.update({f"indirect{c}": [] for c in cfg})
    t.update({f"floor{c}": [] for c in cfg})
    stages = {c: {s: [] for s in STAGES} for c in cfg}
    chunks = {}
    for rep in range(warm + reps):
        keep = rep >= warm
        ms = timed(gbuffer)
        if keep:
            t["gbuffer"].append(ms)
        for n in NS:
            timed(lambda: r.render_lens_device(W, W, depth, 0, W, out.data_ptr(), stream, samples=n))
            resolve_ms = r.lens_info().resolve_ms
            lens_ms = timed(lambda: lens_rays(n))
            own_ms = timed(lambda: own_rays(n))                     # (last: the floor traces what it left in `rays`)
            if keep:
                t[f"lens_resolve{n}"].append(resolve_ms), t[f"lens_rays{n}"].append(lens_ms), t[f"rays{n}"].append(own_ms)
            for c in (c for c in cfg if c[0] == n):
                ms = timed(lambda: indirect(*c))
                info = r.indirect_info()
                chunks[c] = int(info.chunks)
                assert chunks[c] == -(-N // default_chunk(n, c[2])), (c, chunks[c])
                floor_ms = timed(lambda: floor(*c))
                if keep:
                    t[f"indirect{c}"].append(ms), t[f"floor{c}"].append(floor_ms)
                    for s in STAGES:
                        stages[c][s].append(getattr(info, s))
    g = med(t["gbuffer"])
    w = {"gbuffer_ms": g, "n": {}}
    print(f"== {name} {W}x{W} depth {depth}: rt_render_gbuffer_device alone {g:.3f} ms "
          f"(min {min(t['gbuffer']):.3f}, max {max(t['gbuffer']):.3f})", flush=True)
    for n in NS:
        own, lens, lres = med(t[f"rays{n}"]), med(t[f"lens_rays{n}"]), med(t[f"lens_resolve{n}"])
        traffic = (24 + 48 / (n * n)) / 24
        print(f"n={n} ray generation, whole frame in one launch: rt_indirect_rays_device {own:.3f} ms, rt_lens_rays_device {lens:.3f} ms: "
              f"{own / lens:.3f} x (traffic {traffic:.3f} x); rt_render_lens_device's resolve stage {lres:.3f} ms", flush=True)
        w["n"][n] = {"rays_ms": own, "lens_rays_ms": lens, "lens_resolve_ms": lres, "traffic_ratio": traffic, "configs": {}}
        for c in (c for c in cfg if c[0] == n):
            st = {s: med(stages[c][s]) for s in STAGES}
            frame, fl = med(t[f"indirect{c}"]), med(t[f"floor{c}"])
            row = {"frame_ms": frame, "over_gbuffer": frame / g, "chunks": chunks[c], "stages_ms": st, "floor_ms": fl,
                   "trace_over_floor": st["trace_ms"] / fl, "floor_min_max": [min(t[f"floor{c}"]), max(t[f"floor{c}"])],
                   "raygen_over_lens": st["raygen_ms"] / lens, "resolve_over_lens": st["resolve_ms"] / lres,
                   "query_over_trace": st["query_ms"] / st["trace_ms"]}
            print(f"n={n} gather_depth={c[1]} emitters={c[2]}: {frame:9.3f} ms = {row['over_gbuffer']:.2f} x gbuffer, {chunks[c]} chunk(s), "
                  + ", ".join(f"{s[:-3]} {st[s]:.3f}" for s in STAGES)
                  + f" | trace {row['trace_over_floor']:.3f} x floor ({fl:.3f} ms, {row['floor_min_max'][0]:.3f} .. {row['floor_min_max'][1]:.3f})"
                  + f" | raygen {row['raygen_over_lens']:.3f} x lens, resolve {row['resolve_over_lens']:.3f} x lens"
                  + (f" | query {row['query_over_trace']:.3f} x trace" if not c[2] else ""), flush=True)
            w["n"][n]["configs"][f"d{c[1]}e{c[2]}"] = row
    result["workloads"][name] = w
    del r
if "out" in opts:
    with open(opts["out"], "w") as f:
        json.dump(result, f, indent=1)
