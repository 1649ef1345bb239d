"""Cost of soft shadows (include/rt_capi_soft.h): the built-in 4096^2 depth-4 frame and the grid-32 frame, as is (hard shadows)
and with every light an area light of n x n samples, n = 1, 2, 4 (radius: the built-in lights' own 0.15, grid-32's 0.5) --
the *_soft kernels.  rt_render_device, interleaved, kernel time by HIP events (rt_get_timing), median of `reps` launches each
after a warm-up.

usage: soft_gpu.py [reps=25] [W=4096] [depth=4] [grid=32] [gW=2048] [gdepth=8]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer, capi  # noqa: E402


def renderer(host, area=None):
    d = host.desc.contents
    objs = (capi.RtObjectDesc * d.n_objects)()
    for i in range(d.n_objects):
        objs[i] = d.objects[i]
    texs = (capi.RtTextureDesc * max(d.n_textures, 1))()
    for i in range(d.n_textures):
        texs[i] = d.textures[i]
    cam = capi.RtCameraDesc()
    C.memmove(C.byref(cam), host.camera, C.sizeof(capi.RtCameraDesc))
    desc = capi.RtSceneDesc(d.n_objects, objs, d.n_textures, texs, d.shadow_begin, d.shadow_end, d.null_color)
    return Renderer.from_desc(desc, cam, keepalive=(host, objs, texs, desc, cam), area_lights=area)


def measure(label, host, radius, W, depth, reps):
    d = host.desc.contents
    lights = [i for i in range(d.n_objects) if d.objects[i].is_light]
    variants = [("hard", renderer(host))] + [(f"n{n}", renderer(host, [(k, n, radius) for k in lights])) for n in (1, 2, 4)]
    st = torch.cuda.current_stream().cuda_stream
    outs = {tag: torch.empty((W, W, 3), dtype=torch.float32, device="cuda:0") for tag, _ in variants}
    runs = [(tag, (lambda r=r, o=outs[tag]: r.render_device(W, W, depth, 0, W, o.data_ptr(), st)), r) for tag, r in variants]
    for _ in range(3):                     # clocks still rising in the first frames of a process
        for _, fn, _ in runs:
            fn()
    torch.cuda.synchronize()
    times = {tag: [] for tag, _, _ in runs}
    kernels = {}
    for _ in range(reps):
        for tag, fn, r in runs:
            fn()
            torch.cuda.synchronize()
            times[tag].append(r.timing().last_kernel_ms)
            kernels[tag] = r.launch_info().kernel.decode()
    med = {k: statistics.median(v) for k, v in times.items()}
    base = med["hard"]
    for k in med:
        print(f"{label} {W}x{W} d{depth} r{radius} {k:5s} {med[k]:8.3f} ms x{med[k] / base:5.3f} [{kernels[k]}] "
              f"(min {min(times[k]):.3f}, max {max(times[k]):.3f}) n={reps}", flush=True)


opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps = int(opts.get("reps", 25))
measure("builtin", HostScene.builtin(), 0.15, int(opts.get("W", 4096)), int(opts.get("depth", 4)), reps)
g = int(opts.get("grid", 32))
measure(f"grid{g}", HostScene.grid(g), 0.5, int(opts.get("gW", 2048)), int(opts.get("gdepth", 8)), reps)
