"""Cost of tracing caller-supplied rays (include/rt_capi_rays.h): rt_trace_rays_device of a frame's own rays in the frame's
order (rows = H) against rt_render_device of the frame -- the same rays, read from memory instead of made by the camera -- and
of the same rays shuffled; interleaved, kernel time by HIP events (rt_get_timing), median of `reps` launches each after a
warm-up (development aid).  "row 0": rt_render_device with option first_row = 0, the tile order a ray batch always has (no
camera, no horizon to start from), which tells the order's share of the difference from the rest.

usage: rays_gpu.py [reps=25] [only=builtin4096,grid32,grid16d8]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (before the library brings in the HIP runtime)
import numpy as np  # noqa: E402

from rays_ref import camera_rays  # noqa: E402
from tilecoderaytracer_amd import HostScene, Renderer  # noqa: E402

opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps = int(opts.get("reps", 25))
cases = [("builtin4096", "builtin", 4096, 4096, 4), ("grid32", "grid32", 2048, 2048, 4), ("grid16d8", "grid16", 2048, 2048, 8)]
if "only" in opts:
    cases = [c for c in cases if c[0] in opts["only"].split(",")]
for label, name, W, H, depth in cases:
    r = Renderer(HostScene.named(name))
    st = torch.cuda.current_stream().cuda_stream
    rays = camera_rays(r._cam, W, H)
    ordered = torch.from_numpy(rays).to("cuda:0")
    perm = torch.from_numpy(np.random.default_rng(1).permutation(W * H)).to("cuda:0")
    shuffled = ordered.reshape(-1, 6)[perm].contiguous()
    out = torch.empty((W, H, 3), dtype=torch.float32, device="cuda:0")

    def plain():
        r.set_option("first_row", -1)
        r.render_device(W, H, depth, 0, W, out.data_ptr(), st)

    def row0():
        r.set_option("first_row", 0)
        r.render_device(W, H, depth, 0, W, out.data_ptr(), st)
        r.set_option("first_row", -1)

    def traced():
        r.trace_rays_device(W * H, H, ordered.data_ptr(), depth, out.data_ptr(), st)

    def shuffle():
        r.trace_rays_device(W * H, H, shuffled.data_ptr(), depth, out.data_ptr(), st)

    runs = (("render", plain), ("row0", row0), ("rays", traced), ("shuffled", shuffle))
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
    p, p0, t, s = (statistics.median(times[k]) for k in ("render", "row0", "rays", "shuffled"))
    print(f"{label:12s} {name} {W}x{H} d{depth}: rt_render {p:8.3f} ms [{kernels['render']}]  row 0 {p0:8.3f} ms  "
          f"rt_trace_rays {t:8.3f} ms [{kernels['rays']}] ratio {t / p:6.4f}  "
          f"shuffled {s:8.3f} ms ratio {s / p:6.3f} ({W * H / (s * 1e3):8.1f} Mrays/s)  "
          f"(min {min(times['render']):.3f} / {min(times['rays']):.3f} / {min(times['shuffled']):.3f}, n={reps})", flush=True)
