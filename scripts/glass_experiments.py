"""What profiles/glass_experiments.txt records (include/rt_glass.h): at 4096 x 4096 pixel rays (rt_lens_rays at one sample,
aperture 0, focus 1; a hit query has no depth), max_bounces 1, 4 and 8 --
  a. the cost of the glass step when nothing is glass: rt_glass_records_device with min_transmissive = +inf against
     rt_mirror_records_device in the same run, on the mirror room (tests/mirror_scenes.py) and the built-in scene.  The mirror
     call's step kernel is the one the library had before rt_glass.h (rt_mirror_body.h's kernel is unchanged, and so are its
     registers).  Both medians and the run's own spread: the interquartile range of the repetitions;
  b. the glass room (tests/glass_scenes.py): the call against max_bounces + 1 hit queries of the pixel rays (the floor), and the
     step kernels' share of the call's device time (rt_glass_info);
  c. divergence: the step kernels' time on the glass room with its two spheres in the refractive list and without them (the
     same geometry and rays; only the sphere branch -- four sqrtf and the divides, on a minority of lanes -- goes away, and the
     chains behind the spheres with it).
Every call is timed two ways over --reps interleaved repetitions after a warm-up, in one process with nothing downloaded inside
a timed window: device time between HIP events around the call, and wall time from before the call until the stream has
drained.  Median, interquartile range, minimum and maximum of each.

    timeout 300 python scripts/glass_experiments.py --part a >> profiles/glass_experiments.txt     (likewise b, c)
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BOUNCES = (1, 4, 8)
INF = float("inf")


def spread(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[2] - q[0], min(v), max(v)


def fmt(t):
    return f"{t[0]:8.3f} ms (iqr {t[1]:.3f}, min {t[2]:.3f}, max {t[3]:.3f})"


def interleaved(fns, reps, after=None, warmup=2):
    """{name: (device-time spread, wall-time spread, [after()'s value per repetition])}, one repetition of each fn in turn"""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    device, wall, extra = ({k: [] for k in fns} for _ in range(3))
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            device[k].append(a.elapsed_time(b))
            if after:
                extra[k].append(after(k))
    return {k: (spread(device[k]), spread(wall[k]), extra[k]) for k in fns}


class Frame:
    """a Renderer's pixel rays and outputs on the device"""

    def __init__(self, r, W, H):
        import torch
        from tilecoderaytracer_amd import capi
        from tilecoderaytracer_amd.renderer import lens_params
        self.r, self.N, self.H = r, W * H, H
        new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
        self.rays, self.plain = new(self.N * 6), new(self.N * 12, torch.int32)
        self.out = [new(self.N * 12, torch.int32), new(self.N * 12, torch.int32), new(self.N * 3), new(self.N, torch.int32)]
        self.stream = torch.cuda.current_stream().cuda_stream
        lens = lens_params(1, 0.0, 1.0, 0)
        capi.check(capi.load_library().rt_lens_rays_device(r._cam, W, H, 0, W, C.byref(lens), 0, self.rays.data_ptr(), self.stream))

    def glass(self, bounces, floor, look):
        return lambda: self.r.glass_records_device(self.N, self.H, self.rays.data_ptr(), *[o.data_ptr() for o in self.out],
                                                   stream=self.stream, max_bounces=bounces, min_reflective=floor,
                                                   min_transmissive=look)

    def mirror(self, bounces, floor):
        return lambda: self.r.mirror_records_device(self.N, self.H, self.rays.data_ptr(), *[o.data_ptr() for o in self.out],
                                                    stream=self.stream, max_bounces=bounces, min_reflective=floor)

    def queries(self, count):
        def run():
            for _ in range(count):
                self.r.intersect_rays_device(self.N, self.H, self.rays.data_ptr(), self.plain.data_ptr(), self.stream)
        return run

    def close(self):
        import torch
        self.r.close()
        del self.rays, self.plain, self.out
        torch.cuda.empty_cache()


def glass_renderer(without_spheres=False):
    import glass_scenes
    from test_refract_gpu import make
    from test_texture_gpu import Desc
    host, refr = glass_scenes.host_scene("glass")
    if without_spheres:
        refr = [e for e in refr if e[0] == glass_scenes.PANE]
    return make(Desc(host), refractive=refr)


def part_a(args):
    import mirror_scenes
    from tilecoderaytracer_amd import Renderer
    for key, floor in (("room", 1.0), ("builtin", 0.5)):
        f = Frame(Renderer(mirror_scenes.host_scene(key)), args.size, args.size)
        fns = {}
        for b in BOUNCES:
            fns[("glass", b)] = f.glass(b, floor, INF)
            fns[("mirror", b)] = f.mirror(b, floor)
        step = lambda k: (f.r.glass_info() if k[0] == "glass" else f.r.mirror_info()).step_ms
        res = interleaved(fns, args.reps, after=step)
        print(f"\n== a. nothing is glass: {key} {args.size}x{args.size}, min_reflective {floor}, min_transmissive inf")
        for b in BOUNCES:
            g, m = res[("glass", b)], res[("mirror", b)]
            inside = abs(g[0][0] - m[0][0]) <= max(g[0][1], m[0][1])
            print(f"   max_bounces {b}: rt_glass_records_device  device {fmt(g[0])}  wall {fmt(g[1])}  step_ms {statistics.median(g[2]):.3f}")
            print(f"                  rt_mirror_records_device device {fmt(m[0])}  wall {fmt(m[1])}  step_ms {statistics.median(m[2]):.3f}")
            print(f"                  glass - mirror {g[0][0] - m[0][0]:+.3f} ms ({100.0 * (g[0][0] / m[0][0] - 1.0):+.2f} %): "
                  f"{'within' if inside else 'OUTSIDE'} the larger interquartile range ({max(g[0][1], m[0][1]):.3f} ms)")
        f.close()


def part_b(args):
    f = Frame(glass_renderer(), args.size, args.size)
    f.glass(8, 1.0, 0.5)()
    import torch
    torch.cuda.synchronize()
    path = f.out[3]
    k = path & 0xff
    alive = [int((k >= b).sum()) for b in range(9)]
    print(f"\n== b. the glass room {args.size}x{args.size}, min_reflective 1.0, min_transmissive 0.5: rays alive at bounce 0..8 "
          f"(max_bounces 8): " + " ".join(f"{100.0 * a / f.N:.2f}%" for a in alive) +
          f"; looked through glass: {100.0 * int(((path >> 10) & 1).sum()) / f.N:.2f}%; cut at 8: {100.0 * int(((path >> 8) & 1).sum()) / f.N:.3f}%")
    fns = {}
    for b in BOUNCES:
        fns[("glass", b)] = f.glass(b, 1.0, 0.5)
        fns[("queries", b)] = f.queries(b + 1)
    info = lambda key: (f.r.glass_info().step_ms, f.r.glass_info().query_ms) if key[0] == "glass" else (0.0, 0.0)
    res = interleaved(fns, args.reps, after=info)
    for b in BOUNCES:
        g, q = res[("glass", b)], res[("queries", b)]
        step, query = statistics.median(v[0] for v in g[2]), statistics.median(v[1] for v in g[2])
        print(f"   max_bounces {b}: the call device {fmt(g[0])}  wall {fmt(g[1])}")
        print(f"                  {b + 1} queries of the pixel rays device {fmt(q[0])}  wall {fmt(q[1])};  the call is {g[0][0] / q[0][0]:5.3f} x")
        print(f"                  step_ms {step:.3f}, query_ms {query:.3f}: the steps are {100.0 * step / (step + query):.1f} % of the call's stages")
    f.close()


def part_c(args):
    frames = {"spheres in the refractive list": Frame(glass_renderer(), args.size, args.size),
              "the pane alone": Frame(glass_renderer(without_spheres=True), args.size, args.size)}
    fns = {(name, b): f.glass(b, 1.0, 0.5) for name, f in frames.items() for b in BOUNCES}
    info = lambda key: (frames[key[0]].r.glass_info().step_ms, frames[key[0]].r.glass_info().query_ms)
    res = interleaved(fns, args.reps, after=info)
    print(f"\n== c. divergence: the glass room {args.size}x{args.size}, min_reflective 1.0, min_transmissive 0.5; step_ms and "
          f"query_ms of rt_glass_info, medians of {args.reps}")
    for b in BOUNCES:
        for name in frames:
            v = res[(name, b)][2]
            steps = spread([x[0] for x in v])
            print(f"   max_bounces {b}, {name:31s}: step_ms {fmt(steps)}, query_ms {statistics.median(x[1] for x in v):8.3f}, "
                  f"the call device {fmt(res[(name, b)][0])}")
    for f in frames.values():
        f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--part", choices=("a", "b", "c"), required=True)
    args = ap.parse_args()
    import torch
    print(f"# glass records, part {args.part}: {args.size} x {args.size} pixel rays, {torch.cuda.get_device_name(0)}; "
          f"median (interquartile range, min, max) of {args.reps} interleaved repetitions")
    {"a": part_a, "b": part_b, "c": part_c}[args.part](args)


if __name__ == "__main__":
    main()
