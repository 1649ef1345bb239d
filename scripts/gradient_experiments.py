"""What profiles/gradient_experiments.txt records (include/rt_gradient.h).

On the GPU: at 4096 x 4096, depth 4, one and three channels, on the motion tests' scene (tests/motion_scenes.py, pose REST then
SHIFTED) -- the stale-frame setting scripts/clamp_experiments.py measures the clamp on: eight frames of the previous pose
accumulated with match_color, then the current pose pushed with its motion table under equal cameras, so that the history is
stale where shadows and reflections moved.  The two cell frames are the G-buffer's colours of both poses at 1/s^2 density under
that camera, their records the two G-buffers'.  Timed on that frame: rt_gradient_reweight_device for scale 2 / 4 x radius 0, 1, 2
-- both forms of the window's reads where the library has them -- against a device copy of the bytes the call must move at full
resolution (117 a pixel with three channels: the record 48, cur 12, value 12, moments 8, length 4 in; value 12, moments 8, length
4, variance 4, lambda 4, flags 1 out; 93 with one; the cells add (96 + 8 channels) / s^2) and against rt_history_clamp_device with
the extremes box at r = 1.  Every time is device time between events around one device call, the median, minimum and maximum of
REPS interleaved repetitions after a warm-up; one process, nothing downloaded inside a timed window.  Each setting's shares of
pixels re-blended (flag 1) and restarted (flag 3) are read after the timing.  The comparison of the kernel forms needs both, which
only a build with -DRT_GRADIENT_VARIANTS=1 has; the two forms' outputs are compared word for word.  Last, what render_animated()
costs per frame with gradient= against without: five frames of the two poses, term "direct", the whole call between two events
(its one download included in both), the difference divided by the four frames that have a gradient.

    make -C tilecoderaytracer_amd/csrc variant NAME=gradient_variants DEFS=-DRT_GRADIENT_VARIANTS=1
    TCRT_LIBRARY=tilecoderaytracer_amd/lib/variants/libtcrt_gradient_variants.so \\
    timeout 900 python scripts/gradient_experiments.py [--size 4096] [--reps 11] > profiles/gradient_experiments.txt

Without a GPU, from the tests' reference (tests/gradient_ref.py over tests/clamp_scenes.py):

    python scripts/gradient_experiments.py --cpu >> profiles/gradient_experiments.txt

the ghost-pixel error of two pose pairs at 192 x 128 for scales 2, 3, 4, radii 0, 1, 2 and gains 2 and 4, beside the clamp's, and
the unchanged static pixels whose weight is not 0."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F = np.float32
SETTINGS = [(scale, radius) for scale in (2, 4) for radius in (0, 1, 2)]
BYTES = {3: 117, 1: 93}


# ---- without a GPU: the reference's numbers ---------------------------------------------------------------------------------------

def cpu_tables():
    import clamp_ref
    from clamp_scenes import GHOST_KW, GHOST_PAIRS, ghost_error
    from test_gradient_cpu import ghost_reweight, gradient_setting
    print("\n# the tests' reference: the ghost pixels of two pose pairs of tests/motion_scenes.py under equal cameras at 192 x 128 -- 8"
          "\n# frames of the previous pose accumulated with match_color, one frame of the current pose pushed; the cell frames are the"
          "\n# oracle's colours of both poses at every s-th pixel, the cell records the two G-buffers'; error = mean over the ghost pixels"
          "\n# (static objects, with history, colour changed by more than 0.02) of max over channels |value - current colour|;"
          "\n# normal_cos 0.9, match_color 1, lambda_min 0, den_floor 1e-6")
    for name in GHOST_PAIRS:
        cur, hits, value, moments, length, ghost, unchanged = gradient_setting(name, 192, 128)[0]
        clamped = clamp_ref.clamp(cur, hits, value, moments, length, **GHOST_KW)
        print(f"{name}: {int(ghost.sum())} ghost pixels, {int(unchanged.sum())} unchanged static pixels with history; no call "
              f"{ghost_error(value, cur, ghost):.3f}, clamp extremes r=1 {ghost_error(clamped[0], cur, ghost):.3f}")
        for scale in (2, 3, 4):
            for radius in (0, 1, 2):
                for gain in (2.0, 4.0):
                    out, _ = ghost_reweight(name, scale, radius, gain)
                    touched = unchanged & (out[4] > 0)
                    kept = np.ascontiguousarray(out[0]).view(np.uint32)[touched].tobytes() == np.ascontiguousarray(value).view(np.uint32)[touched].tobytes()
                    print(f"   s={scale} r={radius} gain={gain:g}: ghost error {ghost_error(out[0], cur, ghost):.3f}; unchanged with lambda > 0: "
                          f"{int(touched.sum())} ({100.0 * touched.sum() / unchanged.sum():.1f} %), their values "
                          f"{'kept bit for bit' if kept else 'CHANGED'}; flags 1 / 2 / 3: "
                          f"{int((out[5] == 1).sum())} / {int((out[5] == 2).sum())} / {int((out[5] == 3).sum())}")


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------

def gpu_tables(args):
    import motion_scenes
    import torch
    from temporal_experiments import fmt, interleaved
    from tilecoderaytracer_amd import Renderer, TemporalHistory, capi, object_motions, render_animated
    from tilecoderaytracer_amd.renderer import clamp_params, gradient_params
    W = H = args.size
    N = W * H
    lib = capi.load_library()
    variants = hasattr(lib, "rt_internal_gradient_variant")
    if variants:
        lib.rt_internal_gradient_variant.argtypes, lib.rt_internal_gradient_variant.restype = [C.c_int], C.c_int
    forms = (("direct", 0), ("LDS", 1)) if variants else (("as built", None),)
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# rt_gradient_reweight_device, {W} x {H}, depth {args.depth}, {torch.cuda.get_device_name(0)}; device time between events, "
          f"median (min, max) of {args.reps} interleaved repetitions; match_color 1, normal_cos 0.9, gain 2, lambda_min 0, den_floor "
          f"1e-6, then_hits given; " + ("both forms of the window's reads" if variants else
                                        "the library's own form only (no -DRT_GRADIENT_VARIANTS=1 build)"))
    new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
    host_prev, host_cur = motion_scenes.host(motion_scenes.REST), motion_scenes.host(motion_scenes.SHIFTED)
    cam = motion_scenes.camera_pair("equal")[1]
    table = object_motions(host_prev.desc, host_cur.desc)
    renderers = [Renderer(host_prev), Renderer(host_cur)]
    frames, lows = [], {}
    for r in renderers:
        own, r._cam = r._cam, C.pointer(cam)
        colours, records = new(N * 3), new(N * 12, torch.int32)
        r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)
        frames.append((colours, records))
        for s in (2, 4):
            Wl, Hl = W // s, H // s
            lo = (new(Wl * Hl * 3), new(Wl * Hl * 12, torch.int32))
            r.render_gbuffer_device(Wl, Hl, args.depth, 0, Wl, lo[0].data_ptr(), lo[1].data_ptr(), stream)
            lows.setdefault(s, []).append(lo)
        torch.cuda.synchronize()
        r._cam = own
    d_table = torch.tensor(table.reshape(-1), device="cuda")
    print(f"\n== motion scene {W}x{H} depth {args.depth}: {table.shape[0]} objects")
    for channels in (3, 1):
        weights = torch.tensor([0.25, 0.5, 0.25], device="cuda")
        term = lambda c: c if channels == 3 else (c.view(-1, 3) * weights).sum(dim=1)
        before, cur = term(frames[0][0]), term(frames[1][0])
        cells = {s: (term(lows[s][1][0]), term(lows[s][0][0]), lows[s][1][1], lows[s][0][1]) for s in lows}     # now, then, lo_hits, then_hits
        history = TemporalHistory(W, H, channels, match_color=True)
        for _ in range(args.frames):
            history.push_device(before, frames[0][1], cam)
        history.push_device(cur, frames[1][1], cam, motions=d_table)
        torch.cuda.synchronize()
        st = history._sets[history.frames % 2]
        make = lambda: [new(N * channels), new(N * 2), new(N), new(N), new(N), new(N, torch.uint8)]
        out, other = make(), make()
        traffic = BYTES[channels] * N
        half, half2 = new(traffic // 8, torch.int32), new(traffic // 8, torch.int32)
        cp = clamp_params(channels, box=0, radius=1)

        def reweight(scale, radius, form, to=out):
            p = gradient_params(channels, scale=scale, radius=radius)
            now_lo, then_lo, lo_hits, then_hits = cells[scale]

            def call():
                if form is not None:
                    lib.rt_internal_gradient_variant(form)
                capi.check(lib.rt_gradient_reweight_device(0, C.byref(p), W, H, cur.data_ptr(), st["hits"].data_ptr(), st["value"].data_ptr(),
                                                           st["moments"].data_ptr(), st["length"].data_ptr(), now_lo.data_ptr(),
                                                           then_lo.data_ptr(), lo_hits.data_ptr(), then_hits.data_ptr(),
                                                           *[t.data_ptr() for t in to], stream))
            return call

        fns = {"copy": lambda: half2.copy_(half),
               "rt_history_clamp_device box 0 r 1": lambda: capi.check(lib.rt_history_clamp_device(
                   0, C.byref(cp), W, H, cur.data_ptr(), st["hits"].data_ptr(), st["value"].data_ptr(), st["moments"].data_ptr(),
                   st["length"].data_ptr(), *[t.data_ptr() for t in other[:4]], other[5].data_ptr(), stream))}
        for scale, radius in SETTINGS:
            for label, form in forms:
                fns[f"gradient s {scale} r {radius} {label}"] = reweight(scale, radius, form)
        res = interleaved(fns, args.reps)
        print(f"-- {channels} channel(s): a history of {args.frames} frames of the previous pose, then the moved frame; the call moves "
              f"{BYTES[channels]} bytes a pixel, {traffic / 1e6:.1f} MB, and its cells")
        clamp_ms = res["rt_history_clamp_device box 0 r 1"][0]
        for k, t in res.items():
            print(f"   {k:40s} {fmt(t)}  {t[0] / res['copy'][0]:5.2f} x the copy  {t[0] / clamp_ms:5.2f} x the clamp")
        for scale, radius in SETTINGS:
            reweight(scale, radius, forms[0][1])()
            torch.cuda.synchronize()
            flags = out[5]
            line = (f"   s {scale} r {radius}: re-blended {int((flags == 1).sum())} ({100.0 * float((flags == 1).sum()) / N:.3f} %), restarted "
                    f"{int((flags == 3).sum())} ({100.0 * float((flags == 3).sum()) / N:.3f} %), {int((flags == 2).sum())} left for no counted "
                    f"cell, of {N} pixels")
            if variants:
                reweight(scale, radius, 1, other)()
                torch.cuda.synchronize()
                same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(out, other))
                line += f"; the two forms' outputs are {'equal word for word' if same else 'DIFFERENT'}"
            print(line)
        del history, out, other, half, half2
        torch.cuda.empty_cache()
    del frames, lows
    torch.cuda.empty_cache()
    # render_animated with and without gradient=
    a, b = renderers
    sequence = [(a, cam, None), (a, cam, object_motions(host_prev.desc, host_prev.desc)), (b, cam, table),
                (b, cam, object_motions(host_cur.desc, host_cur.desc)), (a, cam, object_motions(host_cur.desc, host_prev.desc))]
    print(f"\n== render_animated(term=direct), {W}x{H} depth {args.depth}, {len(sequence)} frames of the two poses: the whole call between "
          f"two events, median (min, max) of {args.animated_reps} interleaved repetitions")
    settings = {"without": None}
    for s in (2, 4):
        settings[f"gradient s {s} r 1"] = dict(scale=s, radius=1)
    times = {k: [] for k in settings}
    for rep in range(args.animated_reps + 1):
        for k, g in settings.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            render_animated(sequence, W, H, args.depth, term="direct", match_color=True, gradient=g)
            e1.record()
            torch.cuda.synchronize()
            if rep:                                              # (the first round warms up)
                times[k].append(e0.elapsed_time(e1))
    base = statistics.median(times["without"])
    for k, v in times.items():
        med = statistics.median(v)
        extra = "" if k == "without" else f"  +{(med - base) / (len(sequence) - 1):.3f} ms per frame with a gradient ({100.0 * (med - base) / base:.1f} % of the call)"
        print(f"   {k:24s} {med:9.3f} ms (min {min(v):.3f}, max {max(v):.3f}), {med / len(sequence):.3f} ms a frame{extra}")
    for r in renderers:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--animated-reps", type=int, default=5)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--cpu", action="store_true", help="the reference's tables only; needs no GPU")
    args = ap.parse_args()
    return cpu_tables() if args.cpu else gpu_tables(args)


if __name__ == "__main__":
    main()
