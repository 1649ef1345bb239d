"""Cost of image textures (include/rt_capi_texture.h) on a frame whose floor is textured: (a) the plain checkerboard floor,
(b) the same floor as its 2 x 2 CHECKER image -- the *_image kernel, pixels equal to (a) -- and (c) a 1024^2 REPEAT image of
random texels on the floor (a divergent gather of texels from global memory on the floor rows).  rt_render_device,
interleaved, kernel time by HIP events (rt_get_timing), median of `reps` launches each after a warm-up.

usage: texture_gpu.py [reps=25] [only=builtin4096,grid32]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer, capi  # noqa: E402


def renderer(host, images_for_checkers=None):
    """host's scene; images_for_checkers(texture desc) -> image: every checkerboard-textured plane samples that image instead"""
    d = host.desc.contents
    objs = (capi.RtObjectDesc * d.n_objects)()
    for i in range(d.n_objects):
        objs[i] = d.objects[i]
    texs = (capi.RtTextureDesc * max(d.n_textures, 1))()
    for i in range(d.n_textures):
        texs[i] = d.textures[i]
    cam = capi.RtCameraDesc()
    C.memmove(C.byref(cam), host.camera, C.sizeof(capi.RtCameraDesc))
    images = None
    if images_for_checkers is not None:
        images = [images_for_checkers(texs[t]) for t in range(d.n_textures)]
        for i in range(d.n_objects):
            if objs[i].texture >= 0:
                objs[i].texture += d.n_textures
    desc = capi.RtSceneDesc(d.n_objects, objs, d.n_textures, texs, d.shadow_begin, d.shadow_end, d.null_color)
    return Renderer.from_desc(desc, cam, keepalive=(host, objs, texs, desc, cam), images=images)


def checker(x):
    t = np.array([[x.light, x.dark], [x.dark, x.light]], dtype=np.float32)
    return (t, x.width, x.height, 0)


def random_1024(x):
    t = np.random.RandomState(1).uniform(0, 1, (1024, 1024, 3)).astype(np.float32)
    return (t, x.width, x.height, 1)


opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps = int(opts.get("reps", 25))
cases = [("builtin4096", "builtin", 4096, 4096, 4), ("grid32", "grid32", 2048, 2048, 4)]
if "only" in opts:
    cases = [c for c in cases if c[0] in opts["only"].split(",")]
for label, name, W, H, depth in cases:
    host = HostScene.named(name)
    if host.desc.contents.n_textures == 0:
        print(f"{label}: no checkerboard to replace", flush=True)
        continue
    variants = (("checkerboard", renderer(host)), ("checker_image", renderer(host, checker)), ("image_1024", renderer(host, random_1024)))
    st = torch.cuda.current_stream().cuda_stream
    outs = {tag: torch.empty((W, H, 3), dtype=torch.float32, device="cuda:0") for tag, _ in variants}
    runs = [(tag, (lambda r=r, o=outs[tag]: r.render_device(W, H, depth, 0, W, o.data_ptr(), st)), r) for tag, r in variants]
    for _ in range(5):                 # clocks still rising in the first frames of a process
        for _, fn, _ in runs:
            fn()
    torch.cuda.synchronize()
    same = torch.equal(outs["checkerboard"].view(torch.int32), outs["checker_image"].view(torch.int32))
    times = {tag: [] for tag, _, _ in runs}
    kernels = {}
    for _ in range(reps):
        for tag, fn, r in runs:
            fn()
            torch.cuda.synchronize()
            times[tag].append(r.timing().last_kernel_ms)
            kernels[tag] = r.launch_info().kernel.decode()
    med = {k: statistics.median(v) for k, v in times.items()}
    base = med["checkerboard"]
    print(f"{label:12s} {name} {W}x{H} d{depth}: " + "  ".join(
        f"{k} {med[k]:8.3f} ms x{med[k] / base:5.3f} [{kernels[k]}] (min {min(times[k]):.3f})" for k in med) +
        f"  n={reps}  checker image pixels {'equal' if same else 'DIFFER'}", flush=True)
