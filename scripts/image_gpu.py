"""Cost of the image encoder (include/rt_capi_image.h) on the built-in scene, W x W at depth `depth`:

  time (default)  device-event ms of rt_encode_image_device with 3 and with 4 channels, and of a hipMemcpyAsync device-to-device
                  copy that moves the same total traffic -- (12 + C) / 2 bytes a pixel copied, i.e. (12 + C) bytes a pixel read
                  plus written -- taken interleaved, round by round, in this one process after a warm-up of each; the copy, not an
                  earlier run of the kernel, is the yardstick.  The same on a frame of uniform random colours (every search step
                  of every lane differs: the worst case for the threshold reads).  Then the host clock around rt_render's
                  download of the fp32 frame (12 bytes a pixel) against the download of the encoded bytes.  Writes the table as
                  JSON to `out`.
  pmc             one render and `reps` encodes with `channels` channels and nothing else, for a counter run of its own:
                  rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -- python scripts/image_gpu.py mode=pmc channels=3
  counters        sum a rocprofv3 counter CSV (csv=...) per kernel name

usage: image_gpu.py [mode=time] [W=4096] [depth=4] [reps=30] [channels=3] [out=FILE] [csv=FILE]"""
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

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
        print(f"{kernel:60s} {counter:24s} dispatches {n:4d} sum {v:.6g} per dispatch {v / n:.6g}")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer, capi  # noqa: E402
from tilecoderaytracer_amd.renderer import image_params  # noqa: E402

W, depth, reps = int(opts.get("W", 4096)), int(opts.get("depth", 4)), int(opts.get("reps", 30))
lib = capi.load_library()
stream = torch.cuda.current_stream().cuda_stream
pixels = W * W
r = Renderer(HostScene.builtin())
d_rgb = torch.empty((W, W, 3), dtype=torch.float32, device="cuda")
d_out = torch.empty((pixels * 4,), dtype=torch.uint8, device="cuda")
r.render_device(W, W, depth, 0, W, d_rgb.data_ptr(), stream)
torch.cuda.synchronize()


def encode(channels, src):
    params, _ = image_params(channels=channels)
    capi.check(lib.rt_encode_image_device(0, C.byref(params), W, W, src.data_ptr(), d_out.data_ptr(), W * channels, stream))


if mode == "pmc":
    for _ in range(reps):
        encode(int(opts.get("channels", 3)), d_rgb)
    torch.cuda.synchronize()
    sys.exit(0)

d_random = torch.empty_like(d_rgb).uniform_(-0.1, 1.2)
copy_src = torch.empty((pixels * 8,), dtype=torch.uint8, device="cuda").random_(0, 256)
copy_dst = torch.empty_like(copy_src)


def copy(channels):
    n = pixels * (12 + channels) // 2
    copy_dst[:n].copy_(copy_src[:n], non_blocking=True)       # (hipMemcpyAsync device to device on the current stream)


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


arms = {"encode_c3": lambda: encode(3, d_rgb), "copy_c3": lambda: copy(3), "encode_c4": lambda: encode(4, d_rgb),
        "copy_c4": lambda: copy(4), "encode_c3_random": lambda: encode(3, d_random), "encode_c4_random": lambda: encode(4, d_random)}
times = {k: [] for k in arms}
for k in range(3 + reps):                                 # three warm-up rounds; the arms alternate within every round
    for name, fn in arms.items():
        ms = timed(fn)
        if k >= 3:
            times[name].append(ms)
result = {"W": W, "depth": depth, "reps": reps, "device": torch.cuda.get_device_name(0), "ms": {}, "ratio_to_copy": {},
          "download": {}}
for name, t in times.items():
    channels = 3 if "c3" in name else 4
    traffic = pixels * (12 + channels)
    med = statistics.median(t)
    result["ms"][name] = {"median": med, "min": min(t), "max": max(t), "launches": len(t), "bytes_read_plus_written": traffic,
                          "TBps": traffic / (med * 1e-3) / 1e12}
    print(f"{name}: {result['ms'][name]}", flush=True)
for channels in (3, 4):
    for suffix in ("", "_random"):
        result["ratio_to_copy"][f"c{channels}{suffix}"] = (result["ms"][f"encode_c{channels}{suffix}"]["median"]
                                                           / result["ms"][f"copy_c{channels}"]["median"])
print(f"encode / copy: {result['ratio_to_copy']}", flush=True)

# the downloads: rt_render's 12 bytes a pixel (its own timing's last_download_ms) against the encoded bytes, by the host clock
frame = np.empty((W, W, 3), dtype=np.float32)
downloads = {"rt_render_fp32": [], "encoded_c3": [], "encoded_c4": []}
host_out = {c: torch.empty((pixels * c,), dtype=torch.uint8) for c in (3, 4)}          # (pageable, like rt_render's frame)
for k in range(2 + 5):
    capi.check(lib.rt_render(r._scene, r._cam, W, W, 0, W, depth, frame.ctypes.data))
    if k >= 2:
        downloads["rt_render_fp32"].append(r.timing().last_download_ms)
    for c in (3, 4):
        encode(c, d_rgb)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_out[c].copy_(d_out[:pixels * c])
        torch.cuda.synchronize()
        if k >= 2:
            downloads[f"encoded_c{c}"].append((time.perf_counter() - t0) * 1e3)
for name, t in downloads.items():
    nbytes = pixels * {"rt_render_fp32": 12, "encoded_c3": 3, "encoded_c4": 4}[name]
    result["download"][name] = {"median_ms": statistics.median(t), "min_ms": min(t), "bytes": nbytes}
    print(f"download {name}: {result['download'][name]}", flush=True)
if "out" in opts:
    with open(opts["out"], "w") as f:
        json.dump(result, f, indent=1)
