"""Cost of adaptive supersampling (include/rt_capi_adaptive.h) against rt_render and rt_render_ssaa, W x W frames of the built-in
scene and of the 1024-sphere grid at depth `depth`, at the suggested thresholds (colour 1/32, normal cosine 0.9).

Every call is a device call on the current torch stream, timed by device events around it and a synchronise after it; the calls of
a workload are interleaved -- one round runs each of them once, `warm` rounds first, then `reps` rounds whose medians are printed
-- so that a drift of the machine falls on all of them alike.  Per workload and k = 2, 4:
  render, ssaa            rt_render_device and rt_render_ssaa_device (code older than the adaptive call)
  adaptive                rt_render_adaptive_device: the frame time (events around the call: the host's wait for the flagged
                          count is inside), the flagged share, the four stage times of rt_get_adaptive_info and their sum
  flag_all                the same with flag_all = 1: every pixel refined.  trace_ms / ssaa_ms is the cost of a refined sample
                          over one of rt_render_ssaa's; break_even_share is the flagged share at which the adaptive frame would
                          take as long as rt_render_ssaa's: (ssaa - first pass - flags) / (flag_all trace + resolve)
  copy                    the flag stage (flag, scan, list kernels) and flag_all's resolve stage against a device-to-device copy
                          that moves the same algorithmic bytes (flag stage: 12 + 16 B read and 12 + 1 B written a pixel by the
                          flag kernel -- no 12 B written when the first pass rendered into the output --, 1 B read a pixel and 4 B
                          written a flagged pixel by the list kernel; resolve: 12 k^2 + 4 B read and 12 B written a flagged pixel).
                          A record's 16 bytes lie in words 0 and 5..7 of its 48, so the memory system fetches every record
                          whole: the flag stage is also set against a copy of the bytes with 48 B a record

first=copied: the library under test (TCRT_LIBRARY) was built with RT_ADAPTIVE_DIRECT_FIRST=0, so its flag kernel writes 12 B a
pixel more.

usage: adaptive_gpu.py [W=4096] [depth=4] [reps=9] [warm=2] [workloads=builtin,grid32] [first=direct|copied] [out=FILE]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
opts = dict(a.split("=") for a in sys.argv[1:] if "=" in a)

import torch  # noqa: E402  (before the library brings in the HIP runtime)

from tilecoderaytracer_amd import HostScene, Renderer, capi  # noqa: E402

W, depth = int(opts.get("W", 4096)), int(opts.get("depth", 4))
reps, warm = int(opts.get("reps", 9)), int(opts.get("warm", 2))
workloads = opts.get("workloads", "builtin,grid32").split(",")
stream = torch.cuda.current_stream().cuda_stream
pixels = W * W
out = torch.empty((W, W, 3), dtype=torch.float32, device="cuda")
flags = torch.empty((W, W), dtype=torch.uint8, device="cuda")
STAGES = ("first_pass_ms", "flag_ms", "trace_ms", "resolve_ms")


def timed(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def copy_ms(nbytes):
    """a device-to-device copy that moves nbytes in all (half read, half written), median of 9 after a warm-up"""
    n = max(nbytes // 2, 4)
    src = torch.empty((n,), dtype=torch.uint8, device="cuda")
    dst = torch.empty((n,), dtype=torch.uint8, device="cuda")
    times = [timed(lambda: dst.copy_(src)) for _ in range(11)][2:]
    return statistics.median(times)


def med(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


result = {"W": W, "depth": depth, "reps": reps, "warm": warm, "device": torch.cuda.get_device_name(0),
          "library": capi.library_path(), "workloads": {}}
for name in workloads:
    r = Renderer(HostScene.named(name))
    calls = {"render": lambda: r.render_device(W, W, depth, 0, W, out.data_ptr(), stream)}
    for k in (2, 4):
        calls[f"ssaa{k}"] = lambda k=k: r.render_ssaa_device(W, W, depth, k, 0, W, out.data_ptr(), stream)
        calls[f"adaptive{k}"] = lambda k=k: r.render_adaptive_device(W, W, depth, 0, W, out.data_ptr(), flags.data_ptr(), stream,
                                                                     samples=k)
        calls[f"flag_all{k}"] = lambda k=k: r.render_adaptive_device(W, W, depth, 0, W, out.data_ptr(), flags.data_ptr(), stream,
                                                                     samples=k, flag_all=True)
    frame = {c: [] for c in calls}
    stages = {c: {s: [] for s in STAGES} for c in calls if c.startswith(("adaptive", "flag_all"))}
    info = {}
    for rep in range(warm + reps):
        for c, fn in calls.items():
            ms = timed(fn)
            if c in stages:
                i = r.adaptive_info()
                info[c] = i
                if rep >= warm:
                    for s in STAGES:
                        stages[c][s].append(getattr(i, s))
            if rep >= warm:
                frame[c].append(ms)
    w = {"frame_ms": {c: med(v) for c, v in frame.items()}, "adaptive": {}}
    print(f"== {name} {W}x{W} depth {depth}: render {w['frame_ms']['render']['median']:.3f} ms", flush=True)
    for k in (2, 4):
        ssaa = w["frame_ms"][f"ssaa{k}"]["median"]
        a, fa = f"adaptive{k}", f"flag_all{k}"
        st = {c: {s: statistics.median(stages[c][s]) for s in STAGES} for c in (a, fa)}
        flagged = int(info[a].flagged)
        share = flagged / pixels
        ratio = st[fa]["trace_ms"] / ssaa
        break_even = (ssaa - st[a]["first_pass_ms"] - st[a]["flag_ms"]) / (st[fa]["trace_ms"] + st[fa]["resolve_ms"])
        direct = opts.get("first", "direct") == "direct"
        flag_bytes = pixels * (12 + 16 + 1 + (0 if direct else 12)) + pixels * 1 + flagged * 4
        fetched_bytes = flag_bytes + pixels * (48 - 16)
        resolve_bytes = pixels * (12 * k * k + 4 + 12)
        row = {"ssaa_ms": ssaa, "adaptive_frame_ms": w["frame_ms"][a]["median"], "flagged": flagged, "share": share,
               "chunks": int(info[a].chunks), "stages_ms": st[a], "stages_sum_ms": sum(st[a].values()),
               "adaptive_over_ssaa": w["frame_ms"][a]["median"] / ssaa,
               "flag_all_frame_ms": w["frame_ms"][fa]["median"], "flag_all_stages_ms": st[fa],
               "flag_all_chunks": int(info[fa].chunks), "refined_sample_cost_over_ssaa_sample": ratio,
               "break_even_share": break_even,
               "flag_stage_bytes": flag_bytes, "flag_stage_copy_ms": copy_ms(flag_bytes),
               "flag_stage_fetched_bytes": fetched_bytes, "flag_stage_fetched_copy_ms": copy_ms(fetched_bytes),
               "resolve_bytes_flag_all": resolve_bytes, "resolve_copy_ms": copy_ms(resolve_bytes)}
        w["adaptive"][k] = row
        print(f"k={k}: ssaa {ssaa:.3f} ms | adaptive frame {row['adaptive_frame_ms']:.3f} ms = {row['adaptive_over_ssaa']:.3f} x ssaa, "
              f"flagged {flagged} = {100 * share:.2f} %, {row['chunks']} chunk(s), stages "
              + ", ".join(f"{s[:-3]} {st[a][s]:.3f}" for s in STAGES) + f" (sum {row['stages_sum_ms']:.3f})", flush=True)
        print(f"     flag_all frame {row['flag_all_frame_ms']:.3f} ms in {row['flag_all_chunks']} chunk(s), stages "
              + ", ".join(f"{s[:-3]} {st[fa][s]:.3f}" for s in STAGES)
              + f" | a refined sample costs {ratio:.3f} x one of rt_render_ssaa's; break-even share {100 * break_even:.2f} %", flush=True)
        print(f"     flag stage {st[a]['flag_ms']:.3f} ms for {flag_bytes / 1e6:.0f} MB, a copy of as many bytes {row['flag_stage_copy_ms']:.3f} ms"
              f" ({fetched_bytes / 1e6:.0f} MB with whole records: {row['flag_stage_fetched_copy_ms']:.3f} ms)"
              f" | flag_all resolve {st[fa]['resolve_ms']:.3f} ms for {resolve_bytes / 1e6:.0f} MB, a copy {row['resolve_copy_ms']:.3f} ms",
              flush=True)
    result["workloads"][name] = w
    del r
if "out" in opts:
    with open(opts["out"], "w") as f:
        json.dump(result, f, indent=1)
