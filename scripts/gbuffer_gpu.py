"""Cost of a G-buffer frame (include/rt_capi_gbuffer.h): rt_render_gbuffer_device against rt_render_device of the same frame,
and against the two passes it replaces -- rt_render_device plus rt_intersect_rays_device of the frame's own rays, the rays
already on the device; interleaved, kernel time by HIP events (rt_get_timing), median of `reps` launches each after a
warm-up.  Checks once that the fused call's colours and records equal the two passes' (development aid; TCRT_LIBRARY names a
variant build, e.g. make variant NAME=late DEFS=-DRT_GBUFFER_STORE_LATE=1).

usage: gbuffer_gpu.py [reps=25] [only=builtin4096,grid32,grid16]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (before the library brings in the HIP runtime)

from rays_ref import camera_rays  # noqa: E402
from tilecoderaytracer_amd import HostScene, Renderer  # noqa: E402

opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps = int(opts.get("reps", 25))
cases = [("builtin4096", "builtin", 4096, 4096, 4), ("grid32", "grid32", 2048, 2048, 4), ("grid16", "grid16", 2048, 2048, 8)]
if "only" in opts:
    cases = [c for c in cases if c[0] in opts["only"].split(",")]
for label, name, W, H, depth in cases:
    r = Renderer(HostScene.named(name))
    st = torch.cuda.current_stream().cuda_stream
    rays = torch.from_numpy(camera_rays(r._cam, W, H)).to("cuda:0")
    rgb = torch.empty((W, H, 3), dtype=torch.float32, device="cuda:0")
    rgb2 = torch.empty_like(rgb)
    hits = torch.empty((W * H * 12,), dtype=torch.float32, device="cuda:0")
    hits2 = torch.empty_like(hits)

    runs = (("render", lambda: r.render_device(W, H, depth, 0, W, rgb.data_ptr(), st)),
            ("gbuffer", lambda: r.render_gbuffer_device(W, H, depth, 0, W, rgb2.data_ptr(), hits2.data_ptr(), st)),
            ("intersect", lambda: r.intersect_rays_device(W * H, H, rays.data_ptr(), hits.data_ptr(), st)))
    for _ in range(5):                 # clocks still rising in the first frames of a process
        for _, fn in runs:
            fn()
    torch.cuda.synchronize()
    same = torch.equal(rgb.view(torch.int32), rgb2.view(torch.int32)) and torch.equal(hits.view(torch.int32), hits2.view(torch.int32))
    times = {tag: [] for tag, _ in runs}
    kernels = {}
    for _ in range(reps):
        for tag, fn in runs:
            fn()
            torch.cuda.synchronize()
            times[tag].append(r.timing().last_kernel_ms)
            kernels[tag] = r.launch_info().kernel.decode()
    t_r, t_g, t_i = (statistics.median(times[k]) for k in ("render", "gbuffer", "intersect"))
    print(f"{label:12s} {name} {W}x{H} d{depth}: rt_render {t_r:8.3f} ms [{kernels['render']}]  "
          f"rt_render_gbuffer {t_g:8.3f} ms [{kernels['gbuffer']}] ratio {t_g / t_r:6.3f}  "
          f"rt_render + rt_intersect_rays {t_r + t_i:8.3f} ms (intersect {t_i:.3f}) [{kernels['intersect']}]  "
          f"fused / two passes {t_g / (t_r + t_i):6.3f}  "
          f"(min {min(times['render']):.3f} / {min(times['gbuffer']):.3f} / {min(times['intersect']):.3f}, n={reps})  "
          f"outputs {'equal' if same else 'DIFFER'}", flush=True)
