"""Cost of refraction (include/rt_capi_refract.h) on the built-in 4096^2 depth-4 frame, three ways: (a) as is, (b) with the red
sphere (4) made one glass sphere (tf 0.9, ior 1.5, rf 0) -- the *_refract kernel -- and (c) that sphere also reflective (rf
0.5), so that its hits have both children.  rt_render_device, interleaved, kernel time by HIP events (rt_get_timing), median
of `reps` launches each after a warm-up.

usage: refract_gpu.py [reps=25] [W=4096] [depth=4]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer, capi  # noqa: E402


def renderer(host, refractive=None):
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
    return Renderer.from_desc(desc, cam, keepalive=(host, objs, texs, desc, cam), refractive=refractive)


opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps, W, depth = int(opts.get("reps", 25)), int(opts.get("W", 4096)), int(opts.get("depth", 4))
H = W
plain_host, mirror_host = HostScene.builtin(), HostScene.builtin()
mirror_host.set_reflective(4, 0.5)
variants = (("as_is", renderer(plain_host)), ("glass", renderer(plain_host, [(4, 0.9, 1.5)])),
            ("glass_rf0.5", renderer(mirror_host, [(4, 0.9, 1.5)])))
st = torch.cuda.current_stream().cuda_stream
outs = {tag: torch.empty((W, H, 3), dtype=torch.float32, device="cuda:0") for tag, _ in variants}
runs = [(tag, (lambda r=r, o=outs[tag]: r.render_device(W, H, depth, 0, W, o.data_ptr(), st)), r) for tag, r in variants]
for _ in range(5):                     # clocks still rising in the first frames of a process
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
base = med["as_is"]
for k in med:
    print(f"builtin {W}x{H} d{depth} {k:12s} {med[k]:8.3f} ms x{med[k] / base:5.3f} [{kernels[k]}] "
          f"(min {min(times[k]):.3f}, max {max(times[k]):.3f}) n={reps}", flush=True)
