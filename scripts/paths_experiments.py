"""What profiles/paths_experiments.txt records (include/rt_paths.h): at 4096 x 4096 records (rt_render_gbuffer_device at depth 4),
gather depth 1, emitters 0, n = 2 and 4, on the built-in scene and on the sphere grid --
  1. rt_indirect_paths_device at B = 1, 2, 3, 4 against rt_indirect_diffuse_device in the same run (B = 1 is the same launches
     with another resolve and one step kernel more), and each B against B times the one-bounce call;
  2. the stage times of rt_get_paths_info;
  3. step_ms against a device copy of the bytes the step kernels move, counted from alive[]: a lane reads its T (12 bytes; the
     first step the record's two words, 8) and, alive, the colour (12), the record (48; the last step its flags word, 4) and acc
     (12, not the first step), and writes acc (12) and, before the last step, T (12) and the ray (24);
  4. alive[] as shares of alive[0]: the case for or against a compacting variant.
Every time of 1. is device time between events around one device call, the median, minimum and maximum of --reps interleaved
repetitions after a warm-up; one process, nothing downloaded inside a timed window.

    timeout 900 python scripts/paths_experiments.py [--size 4096] [--reps 7] >> profiles/paths_experiments.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BOUNCES = (1, 2, 3, 4)


def step_bytes(alive, total, B):
    """the bytes the B step kernels of a call move, from the paths alive at each bounce"""
    moved = 0
    for b in range(B):
        first, last = b == 0, b == B - 1
        moved += total * (8 if first else 12)
        moved += alive[b] * (12 + (4 if last else 48) + (0 if first else 12) + 12)
        if not last:
            moved += alive[b] * (12 + 24)
        if first:
            moved += (total - alive[0]) * (12 + (0 if last else 12))
    return moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--depth", type=int, default=4)
    args = ap.parse_args()
    import torch
    from temporal_experiments import fmt, interleaved
    from tilecoderaytracer_amd import HostScene, Renderer

    W = H = args.size
    N = W * H
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# diffuse paths, {W} x {H} records at depth {args.depth}, gather depth 1, emitters 0, {torch.cuda.get_device_name(0)}; "
          f"device time between events, median (min, max) of {args.reps} interleaved repetitions")
    for key in ("builtin", "grid32"):
        r = Renderer(HostScene.named(key))
        colours = torch.empty((N * 3,), dtype=torch.float32, device="cuda")
        records = torch.empty((N * 12,), dtype=torch.int32, device="cuda")
        out = torch.empty((N * 3,), dtype=torch.float32, device="cuda")
        r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)
        torch.cuda.synchronize()
        for n in (2, 4):
            kw = dict(samples=n, gather_depth=1, seed=0)
            total = N * n * n

            def paths(B):
                return lambda: r.indirect_paths_device(N, records.data_ptr(), colours.data_ptr(), out.data_ptr(), stream, bounces=B, **kw)

            fns = {"diffuse": lambda: r.indirect_diffuse_device(N, records.data_ptr(), colours.data_ptr(), out.data_ptr(), stream, **kw)}
            for B in BOUNCES:
                fns[f"paths {B}"] = paths(B)
            res = interleaved(fns, args.reps)
            one = res["diffuse"]
            print(f"\n== {key} {W}x{H} n={n}: rt_indirect_diffuse_device {fmt(one)}")
            for B in BOUNCES:
                t = res[f"paths {B}"]
                print(f"   rt_indirect_paths_device B={B}: {fmt(t)}  = {t[0] / one[0]:6.3f} x the one-bounce call, "
                      f"{t[0] / (B * one[0]):6.3f} x B times it")
            for B in BOUNCES:
                stages = []
                fn = paths(B)
                for _ in range(args.reps):
                    fn()
                    i = r.paths_info()
                    stages.append((i.raygen_ms, i.trace_ms, i.query_ms, i.step_ms, i.resolve_ms))
                med = [statistics.median(s[k] for s in stages) for k in range(5)]
                alive = [int(v) for v in i.alive[:B]]
                moved = step_bytes(alive, total, B)
                a, b = (torch.empty((moved // 8,), dtype=torch.int32, device="cuda") for _ in range(2))
                copy = interleaved({"copy": lambda: b.copy_(a)}, args.reps)["copy"]
                del a, b
                print(f"   B={B}: {i.chunks} chunk(s), {i.rays} rays; raygen {med[0]:.3f}, trace {med[1]:.3f}, query {med[2]:.3f}, "
                      f"step {med[3]:.3f}, resolve {med[4]:.3f} ms | the steps move {moved / 1e6:.1f} MB, a device copy of as many "
                      f"bytes {fmt(copy)}: {med[3] / copy[0]:5.2f} x | alive " +
                      " ".join(f"{100.0 * v / max(alive[0], 1):.2f}%" for v in alive) + f" of {alive[0]} ({100.0 * alive[0] / total:.2f}% of the paths)")
        r.close()
        del colours, records, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
