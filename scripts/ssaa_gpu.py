"""Cost of supersampling (include/rt_capi_ssaa.h): rt_render_ssaa_device(W, H, k) against rt_render_device(kW, kH) -- the same
rays, one store per k x k samples instead of one per sample -- interleaved, kernel time by HIP events (rt_get_timing), median
of `reps` launches each after a warm-up (development aid).

usage: ssaa_gpu.py [reps=25] [only=builtin2048,grid32,builtin500]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer  # noqa: E402

opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps = int(opts.get("reps", 25))
cases = [("builtin2048", "builtin", 2048, 2048, 2, 4), ("grid32", "grid32", 1024, 1024, 4, 4),
         ("builtin500", "builtin", 500, 504, 4, 50)]
if "only" in opts:
    cases = [c for c in cases if c[0] in opts["only"].split(",")]
for label, name, W, H, k, depth in cases:
    r = Renderer(HostScene.named(name))
    st = torch.cuda.current_stream().cuda_stream
    virtual = torch.empty((k * W, k * H, 3), dtype=torch.float32, device="cuda:0")
    out = torch.empty((W, H, 3), dtype=torch.float32, device="cuda:0")

    def plain():
        r.render_device(k * W, k * H, depth, 0, k * W, virtual.data_ptr(), st)

    def ssaa():
        r.render_ssaa_device(W, H, depth, k, 0, W, out.data_ptr(), st)

    for _ in range(5):                 # clocks still rising in the first frames of a process
        plain(); ssaa()
    torch.cuda.synchronize()
    times = {"plain": [], "ssaa": []}
    kernels = {}
    for _ in range(reps):
        for tag, fn in (("plain", plain), ("ssaa", ssaa)):
            fn()
            torch.cuda.synchronize()
            times[tag].append(r.timing().last_kernel_ms)
            kernels[tag] = r.launch_info().kernel.decode()
    p, s = statistics.median(times["plain"]), statistics.median(times["ssaa"])
    print(f"{label:12s} {name} {W}x{H} k{k} d{depth}: rt_render({k * W}x{k * H}) {p:9.3f} ms [{kernels['plain']}]  "
          f"rt_render_ssaa {s:9.3f} ms [{kernels['ssaa']}]  ratio {s / p:6.4f}  "
          f"(min {min(times['plain']):.3f} / {min(times['ssaa']):.3f}, n={reps})", flush=True)
