"""Cost of the ray queries (include/rt_capi_query.h): rt_intersect_rays_device of a frame's own rays against
rt_trace_rays_device of the same rays at max_depth 0 (the same nearest-hit scan, plus the shading's shadow scans), and
rt_occluded_rays_device of the segments from the frame's hit points to light 0; interleaved, kernel time by HIP events
(rt_get_timing), median of `reps` launches each after a warm-up (development aid).

usage: query_gpu.py [reps=25] [only=builtin4096,grid32,grid16]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (before the library brings in the HIP runtime)
import numpy as np  # noqa: E402

import oracle_lib  # noqa: E402
from rays_ref import camera_rays  # noqa: E402
from tilecoderaytracer_amd import HostScene, Renderer  # noqa: E402

opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps = int(opts.get("reps", 25))
cases = [("builtin4096", "builtin", 4096, 4096), ("grid32", "grid32", 2048, 2048), ("grid16", "grid16", 2048, 2048)]
if "only" in opts:
    cases = [c for c in cases if c[0] in opts["only"].split(",")]
for label, name, W, H in cases:
    host = HostScene.named(name)
    r = Renderer(host)
    st = torch.cuda.current_stream().cuda_stream
    rays_np = camera_rays(r._cam, W, H)
    rays = torch.from_numpy(rays_np).to("cuda:0")
    rgb = torch.empty((W, H, 3), dtype=torch.float32, device="cuda:0")
    hits = torch.empty((W * H * 12,), dtype=torch.float32, device="cuda:0")
    blocked = torch.empty((W * H,), dtype=torch.uint8, device="cuda:0")
    r.intersect_rays_device(W * H, H, rays.data_ptr(), hits.data_ptr(), st)
    torch.cuda.synchronize()
    o = oracle_lib.OracleScene.named(name)
    L = next(np.array(o.get_object(i).origin.tuple(), dtype=np.float32) for i in range(o.object_count) if o.get_object(i).is_light)
    segs = torch.empty((W * H, 6), dtype=torch.float32, device="cuda:0")
    segs[:, :3] = hits.reshape(-1, 12)[:, 2:5]
    segs[:, 3:] = torch.from_numpy(L).to("cuda:0")

    runs = (("trace_d0", lambda: r.trace_rays_device(W * H, H, rays.data_ptr(), 0, rgb.data_ptr(), st)),
            ("intersect", lambda: r.intersect_rays_device(W * H, H, rays.data_ptr(), hits.data_ptr(), st)),
            ("occluded", lambda: r.occluded_rays_device(W * H, H, segs.data_ptr(), blocked.data_ptr(), st)))
    for _ in range(5):                 # clocks still rising in the first frames of a process
        for _, fn in runs:
            fn()
    torch.cuda.synchronize()
    times = {tag: [] for tag, _ in runs}
    kernels = {}
    for _ in range(reps):
        for tag, fn in runs:
            fn()
            torch.cuda.synchronize()
            times[tag].append(r.timing().last_kernel_ms)
            kernels[tag] = r.launch_info().kernel.decode()
    t, i, s = (statistics.median(times[k]) for k in ("trace_d0", "intersect", "occluded"))
    print(f"{label:12s} {name} {W}x{H}: rt_trace_rays d0 {t:8.3f} ms [{kernels['trace_d0']}]  "
          f"rt_intersect_rays {i:8.3f} ms [{kernels['intersect']}] ratio {i / t:6.3f}  "
          f"rt_occluded_rays (hit points -> light 0) {s:8.3f} ms [{kernels['occluded']}]  "
          f"(min {min(times['trace_d0']):.3f} / {min(times['intersect']):.3f} / {min(times['occluded']):.3f}, n={reps})",
          flush=True)
