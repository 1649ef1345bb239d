"""Cost of rt_ambient_occlusion_device (include/rt_capi_ao.h) against what a caller could do without it: the sum of the kernel
times of the n x n rt_occluded_rays_device launches over the same segments, which are generated on the device beforehand and
not timed (nor are their 24 n^2 bytes per record of writes).  4096 x 4096 records of a depth-0 G-buffer, n = 4, R = 2.0, the
built-in scene and the 1 028-object grid; the two interleaved, kernel time by HIP events (rt_get_timing), medians and spread
of `reps` runs each after a warm-up (development aid).  mode=pmc: only `reps` AO launches, for a rocprofv3 --pmc run of its own.

usage: ao_gpu.py [reps=7] [only=builtin,grid32] [side=4096] [n=4] [radius=2.0] [mode=time|pmc]"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer  # noqa: E402

opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)
reps, side, n, R = int(opts.get("reps", 7)), int(opts.get("side", 4096)), int(opts.get("n", 4)), float(opts.get("radius", 2.0))
mode = opts.get("mode", "time")
names = opts.get("only", "builtin,grid32").split(",")
SEED = 1
M32 = 0xFFFFFFFF
GOLDEN = 0x9E3779B9


def H(x):
    """lowbias32 on int64 tensors holding uint32 values"""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M32
    return x ^ (x >> 16)


def segments(records, s):
    """sample s's segments {P, Q} of the header's definition for every record (float32 (N, 12) view of the rt_hit records):
    float32 (N, 6) on the device, one torch operation per rounding (the records that are no hits get a harmless segment)"""
    N_ = records.shape[0]
    ints = records.view(torch.int32)
    live = (ints[:, 0] >= 0) & ((ints[:, 11] & 2) == 0)
    P = records[:, 2:5]
    Nn = torch.where(((ints[:, 11] & 1) != 0)[:, None], -records[:, 5:8], records[:, 5:8])
    one, zero = torch.ones_like(Nn[:, 0]), torch.zeros_like(Nn[:, 0])
    first = Nn[:, 0].abs() < 0.5
    A = torch.stack([torch.where(first, one, zero), torch.where(first, zero, one), zero], dim=1)

    def cross(a, b):
        return torch.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                            a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], dim=1)

    U = cross(A, Nn)
    U = U / torch.sqrt((U[:, 0] * U[:, 0] + U[:, 1] * U[:, 1]) + U[:, 2] * U[:, 2])[:, None]
    V = cross(Nn, U)
    key = torch.arange(N_, dtype=torch.int64, device=records.device) & M32
    g = H(H(torch.tensor((SEED ^ GOLDEN) & M32, dtype=torch.int64, device=records.device)) ^ key)
    i, j = divmod(s, n)
    hs = H(g ^ s)
    xi1 = (hs >> 8).to(torch.float32) * 2.0 ** -24
    xi2 = (H(hs ^ GOLDEN) >> 8).to(torch.float32) * 2.0 ** -24
    step = torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    a = (xi1 + float(i)) * step.item() - 1.0
    b = (xi2 + float(j)) * step.item() - 1.0
    dx = a * torch.sqrt(1.0 - (b * b) * 0.5)
    dy = b * torch.sqrt(1.0 - (a * a) * 0.5)
    w = (1.0 - dx * dx) - dy * dy
    dz = torch.where(w > 0, torch.sqrt(w.clamp_min(0.0)), torch.zeros_like(w))
    D = (U * dx[:, None] + V * dy[:, None]) + Nn * dz[:, None]
    Q = P + D * R
    segs = torch.cat([P, Q], dim=1)
    segs[~live] = 0.0
    return segs.contiguous(), live


for name in names:
    r = Renderer(HostScene.named(name))
    st = torch.cuda.current_stream().cuda_stream
    W = Hh = side
    count = W * Hh
    colours = torch.empty((count * 3,), dtype=torch.float32, device="cuda:0")
    records = torch.empty((count, 12), dtype=torch.float32, device="cuda:0")
    ao = torch.empty((count,), dtype=torch.float32, device="cuda:0")
    r.render_gbuffer_device(W, Hh, 0, 0, W, colours.data_ptr(), records.data_ptr(), st)
    torch.cuda.synchronize()
    del colours

    def fused():
        r.ambient_occlusion_device(count, Hh, records.data_ptr(), ao.data_ptr(), samples=n, radius=R, seed=SEED, stream=st)
        torch.cuda.synchronize()
        return r.timing().last_kernel_ms

    if mode == "pmc":
        for _ in range(reps):
            fused()
        print(f"{name}: {reps} launches of {r.kernel_name()}", flush=True)
        continue

    segs, live = [], None
    for s in range(n * n):
        sg, live = segments(records, s)
        segs.append(sg)
    blocked = [torch.empty((count,), dtype=torch.uint8, device="cuda:0") for _ in range(n * n)]
    torch.cuda.synchronize()

    def baseline():
        total = 0.0
        for s in range(n * n):
            r.occluded_rays_device(count, Hh, segs[s].data_ptr(), blocked[s].data_ptr(), st)
            torch.cuda.synchronize()
            total += r.timing().last_kernel_ms
        return total

    for _ in range(2):                 # clocks still rising in the first launches of a process
        fused()
        kernel = r.kernel_name()
        baseline()
        base_kernel = r.kernel_name()
    # what the two compute: the same numbers, if torch rounds the segments as the kernel does
    open_ = sum((1 - b.to(torch.int32)) for b in blocked)
    from_query = torch.where(live, open_.to(torch.float32) / float(n * n), torch.ones_like(ao))
    differing = int((from_query != ao).sum())
    partial = float(((ao > 0) & (ao < 1)).float().mean())
    tf, tb = [], []
    for _ in range(reps):
        tf.append(fused())
        tb.append(baseline())
    mf, mb = statistics.median(tf), statistics.median(tb)
    print(f"{name} {W}x{Hh} n={n} R={R}: fused {mf:.3f} ms [{kernel}] (min {min(tf):.3f} max {max(tf):.3f})  "
          f"{n * n} x rt_occluded_rays_device {mb:.3f} ms [{base_kernel}] (min {min(tb):.3f} max {max(tb):.3f})  "
          f"ratio fused / baseline {mf / mb:.3f}  reps {reps}  records with 0 < ao < 1: {100 * partial:.1f} %  "
          f"records where the torch-made segments' verdicts give another value: {differing}", flush=True)
    del segs, blocked, records, ao
    r.close()
    torch.cuda.empty_cache()
