"""What profiles/paths_compact_experiments.txt records (include/rt_paths_compact.h): at 4096 x 4096 records
(rt_render_gbuffer_device at depth 4), gather depth 1, emitters 0, n = 2 and 4, B = 1, 2, 3, 4, 8, on the built-in scene and on the
sphere grid, rt_indirect_paths_compact_device against rt_indirect_paths_device in the same run --
  1. wall time from the call to a drained stream, and device time, the sum of the call's five stage times (the time the device
     stands idle while the host reads a total is in neither stage and so only in the wall time);
  2. rays traced against records * S * B, traces, queries, syncs, and (wall - device) per sync: what a wait costs;
  3. trace_ms of both calls, and the compact call's trace_ms per bounce as the difference from B to the next B, beside alive[b];
  4. step_ms (the count, scan and step kernels) against a device copy of the bytes they move, counted from alive[]: per entry the
     count reads 20 bytes of the record, T (12) and the slot (4) (bounce 0: the record's two liveness words, 8, and no T or slot);
     the step reads the slot (4), T (12), the colour (12), the record (48; the last step its flags, 4) and acc (12) (bounce 0: 8
     liveness bytes, no slot, T or acc) and writes acc (12) and, for a path that goes on, T (12), the ray (24) and the slot (4).
Every figure is the median of --reps interleaved repetitions (one of each call in turn) after a warm-up; one process, nothing
downloaded inside a timed window.  Both chunk settings are run: each call's default chunk, and the compact call's default (the
smaller) given to both.  --budget stops the script before a setting it has no time left for, and says so.

    timeout 900 python scripts/paths_compact_experiments.py [--size 4096] [--reps 11] [--samples 2,4] >> profiles/paths_compact_experiments.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUNCES = (1, 2, 3, 4, 8)
PATH_BYTES = 141                                   # include/rt_paths_compact.h: a path's scratch
CHUNK_BYTES = 256 << 20


def moved_bytes(alive, total, B):
    """the bytes the count and step kernels of a compact call move, from the paths alive at each bounce (alive[0]: the live
    records' paths; bounce 0's list is all `total` paths)"""
    moved = 0
    for b in range(B):
        first, last = b == 0, b == B - 1
        entries = total if first else alive[b]
        live = alive[b]
        on = 0 if last else (alive[b + 1] if b + 1 < len(alive) else 0)
        if not last:
            moved += entries * 8 if first else entries * 16                     # count: liveness, or T and the slot
            moved += live * 20                                                   # count: the record's words
        moved += entries * 8 if first else entries * (4 + 12 + 12)             # step: liveness, or the slot, T and acc
        moved += live * (12 + (4 if last else 48)) + entries * 12               # step: colour, record; acc written
        moved += on * (12 + 24 + 4)                                              # step: T, the ray and the slot of a path that goes on
    return moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--samples", default="2,4")
    ap.add_argument("--scenes", default="builtin,grid32")
    ap.add_argument("--budget", type=float, default=0.0, help="seconds after which no further setting is started (0: none)")
    args = ap.parse_args()
    import torch
    from tilecoderaytracer_amd import HostScene, Renderer

    started = time.perf_counter()
    W = H = args.size
    N = W * H
    stream = torch.cuda.current_stream().cuda_stream
    med = statistics.median
    print(f"# diffuse paths over the live paths alone, {W} x {H} records at depth {args.depth}, gather depth 1, emitters 0, "
          f"{torch.cuda.get_device_name(0)}; medians of {args.reps} interleaved repetitions; wall: from the call to a drained "
          f"stream; device: the sum of the five stage times", flush=True)
    for key in args.scenes.split(","):
        r = Renderer(HostScene.named(key))
        colours = torch.empty((N * 3,), dtype=torch.float32, device="cuda")
        records = torch.empty((N * 12,), dtype=torch.int32, device="cuda")
        out = torch.empty((N * 3,), dtype=torch.float32, device="cuda")
        r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)
        torch.cuda.synchronize()
        for n in (int(v) for v in args.samples.split(",")):
            S, total = n * n, N * n * n
            compact_chunk = max(1, CHUNK_BYTES // (PATH_BYTES * S))
            for chunk, what in ((0, "each call's default chunk"), (compact_chunk, f"chunk_records {compact_chunk} for both")):
                if args.budget and time.perf_counter() - started > args.budget:
                    print(f"\n== {key} n={n}, {what}: NOT MEASURED (the run's time budget of {args.budget:g} s was used up)", flush=True)
                    continue
                print(f"\n== {key} {W}x{H} n={n}, {what}", flush=True)
                before = None
                for B in BOUNCES:
                    kw = dict(samples=n, gather_depth=1, seed=0, bounces=B, chunk_records=chunk)
                    calls = {False: lambda: r.indirect_paths_device(N, records.data_ptr(), colours.data_ptr(), out.data_ptr(), stream, **kw),
                             True: lambda: r.indirect_paths_device(N, records.data_ptr(), colours.data_ptr(), out.data_ptr(), stream,
                                                                   compact=True, **kw)}
                    rows = {False: [], True: []}
                    for rep in range(args.reps + 1):                         # (the first repetition is the warm-up)
                        for compact, fn in calls.items():
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            fn()
                            torch.cuda.synchronize()
                            wall = (time.perf_counter() - t0) * 1e3
                            i = r.paths_compact_info() if compact else r.paths_info()
                            if rep:
                                rows[compact].append((wall, i.raygen_ms, i.trace_ms, i.query_ms, i.step_ms, i.resolve_ms))
                            if compact:
                                ci = i
                            else:
                                pi = i
                    m = {c: [med(row[k] for row in rows[c]) for k in range(6)] for c in rows}
                    dev = {c: sum(m[c][1:]) for c in m}
                    alive = [int(v) for v in ci.alive[:B]]
                    assert alive == [int(v) for v in pi.alive[:B]], (alive, list(pi.alive[:B]))
                    moved = moved_bytes(alive, total, B)
                    a, b = (torch.empty((max(moved // 8, 1),), dtype=torch.int32, device="cuda") for _ in range(2))
                    copies = []
                    for rep in range(args.reps + 1):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        b.copy_(a)
                        e1.record()
                        torch.cuda.synchronize()
                        if rep:
                            copies.append(e0.elapsed_time(e1))
                    del a, b
                    copy = med(copies)
                    verdict = "" if m[True][0] < m[False][0] else "  THE COMPACT CALL LOSES (wall)"
                    print(f"   B={B}: rt_indirect_paths_device wall {m[False][0]:9.3f} device {dev[False]:9.3f} (trace {m[False][2]:9.3f}, query "
                          f"{m[False][3]:8.3f}, step {m[False][4]:7.3f}) ms, {pi.chunks} chunk(s), {pi.rays} rays", flush=True)
                    print(f"        rt_indirect_paths_compact_device wall {m[True][0]:9.3f} device {dev[True]:9.3f} (trace {m[True][2]:9.3f}, "
                          f"query {m[True][3]:8.3f}, step {m[True][4]:7.3f}) ms, {ci.chunks} chunk(s), {ci.rays} rays = "
                          f"{100.0 * ci.rays / (total * B):.1f}% of records*S*B, {ci.traces} traces, {ci.queries} queries, {ci.syncs} syncs, "
                          f"(wall - device) / sync {(m[True][0] - dev[True]) / max(ci.syncs, 1):.3f} ms{verdict}", flush=True)
                    print(f"        wall {m[True][0] / m[False][0]:.3f} x, device {dev[True] / dev[False]:.3f} x, trace "
                          f"{m[True][2] / m[False][2]:.3f} x the in-place call's | count+scan+step move {moved / 1e6:.1f} MB, a device copy "
                          f"of as many bytes {copy:.3f} ms: {m[True][4] / copy:5.2f} x | alive " +
                          " ".join(f"{100.0 * v / total:.1f}%" for v in alive) + " of the paths", flush=True)
                    if before is not None and B - before[0] > 0:
                        span = f"{before[0]}..{B - 1}"
                        print(f"        compact trace_ms of bounces {span}: {m[True][2] - before[1]:.3f} ms for "
                              f"{sum(alive[before[0]:B])} rays; in place {m[False][2] - before[2]:.3f} ms for {total * (B - before[0])}", flush=True)
                    before = (B, m[True][2], m[False][2])
        r.close()
        del colours, records, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
