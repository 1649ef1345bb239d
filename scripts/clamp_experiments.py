"""What profiles/clamp_experiments.txt records (include/rt_clamp.h).

On the GPU: at 4096 x 4096, depth 4, one and three channels, on the built-in scene and the 1024-sphere grid -- the current frame
rendered from a scene whose spheres stand 0.05 units further along x, as scripts/motion_experiments.py moves them -- and on the
motion tests' scene (tests/motion_scenes.py, pose REST then SHIFTED): eight frames of the previous pose accumulated with
match_color, then the current pose pushed with its motion table under equal cameras, so that the history is stale where shadows
and reflections moved.  Timed on that frame: rt_history_clamp_device for box 0 / 1 x radius 1, 2, 3 -- both forms of the window's
reads where the library has them -- against a device copy of the bytes the call must move (113 a pixel with three channels: the
record 48, cur 12, value 12, moments 8, length 4 in; value 12, moments 8, length 4, variance 4, flags 1 out; 89 with one), against
rt_motion_accumulate_device of the same frame and against a one-iteration rt_svgf_filter_device.  Every time is device time between
events around one device call, the median, minimum and maximum of REPS interleaved repetitions after a warm-up; one process,
nothing downloaded inside a timed window.  Each setting's share of pixels clipped is read after the timing.  The comparison of the
kernel forms needs both, which only a build with -DRT_CLAMP_VARIANTS=1 has; the two forms' outputs are compared word for word.

    make -C tilecoderaytracer_amd/csrc variant NAME=clamp_variants DEFS=-DRT_CLAMP_VARIANTS=1
    TCRT_LIBRARY=tilecoderaytracer_amd/lib/variants/libtcrt_clamp_variants.so \
    timeout 900 python scripts/clamp_experiments.py [--size 4096] [--reps 11] > profiles/clamp_experiments.txt

Without a GPU, from the tests' reference (tests/clamp_ref.py over tests/temporal_ref.py and tests/motion_ref.py):

    python scripts/clamp_experiments.py --cpu >> profiles/clamp_experiments.txt

the ghost-pixel error of two pose pairs at 96 x 64 and 192 x 128 for both boxes and every radius, the unchanged pixels each box
clips, and what the clamp costs where nothing moved: the RMSE against the clean signal of eight accumulated frames of a static
scene under Gaussian noise of sigma 0.2, the clamp applied after every frame."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F = np.float32
SETTINGS = [(box, radius) for box in (0, 1) for radius in (1, 2, 3)]
BYTES = {3: 113, 1: 89}


# ---- without a GPU: the reference's numbers ---------------------------------------------------------------------------------------

def cpu_tables():
    import clamp_ref
    import temporal_ref
    from clamp_scenes import GHOST_PAIRS, ghost_error, ghost_setting
    from test_temporal_cpu import pair_records
    print("\n# the tests' reference: the ghost pixels of two pose pairs of tests/motion_scenes.py under equal cameras -- 8 frames of the"
          "\n# previous pose accumulated with match_color, one frame of the current pose pushed; error = mean over the ghost pixels"
          "\n# (static objects, with history, colour changed by more than 0.02) of max over channels |value - current colour|;"
          "\n# min_taps 3, clip_history 4, normal_cos 0.9, match_color 1")
    for W, H in ((96, 64), (192, 128)):
        for name in GHOST_PAIRS:
            cur, hits, value, moments, length, ghost, unchanged = ghost_setting(name, W, H)
            line = f"{W}x{H} {name}: {int(ghost.sum())} ghost pixels, no clamp {ghost_error(value, cur, ghost):.3f}"
            untouched = f"   of {int(unchanged.sum())} unchanged static pixels with history, clipped:"
            for box, gamma in ((0, 1.0), (1, 1.0), (1, 2.0)):
                for radius in (1, 2, 3):
                    out = clamp_ref.clamp(cur, hits, value, moments, length, box=box, radius=radius, match_color=True, gamma=gamma)
                    label = f"extremes r={radius}" if box == 0 else f"moments gamma={gamma:g} r={radius}"
                    line += f" | {label} {ghost_error(out[0], cur, ghost):.3f}"
                    untouched += f" {label}: {int(((out[4] == 1) & unchanged).sum())};"
            print(line)
            print(untouched)
    print("\n# what the clamp costs where nothing moved: the built-in scene's records at 192 x 128 under one camera, the signal 0.5 *"
          "\n# albedo * a stripe pattern plus Gaussian noise of sigma 0.2 (tests/test_svgf_cpu.py's), 8 frames accumulated at"
          "\n# max_history 32, the clamp after every frame; RMSE of the last frame's value against the clean signal over live pixels")
    W, H = 192, 128
    _, cam, _, hits = pair_records("equal", W, H)
    x, z = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    truth = F(0.5) * hits["color"] * np.where(((x + z) // 8) % 2 == 1, F(0.3), F(1.0))[..., None].astype(F)
    live = ~temporal_ref.dead_records(hits)
    for label, kw in (("no clamp", None), ("extremes r=1", dict(box=0, radius=1)), ("moments r=3 gamma=1", dict(box=1, radius=3, gamma=1.0)),
                      ("moments r=3 gamma=2", dict(box=1, radius=3, gamma=2.0))):
        rng = np.random.default_rng(1)
        state, clipped = None, 0
        for _ in range(8):
            cur = (truth + rng.normal(0.0, 0.2, truth.shape)).astype(F)
            value, moments, length, _, _ = temporal_ref.accumulate(cur, hits, cam, state, max_history=32)
            if kw is not None:
                value, moments, length, _, flags = clamp_ref.clamp(cur, hits, value, moments, length, match_color=True, **kw)
                clipped += int((flags == 1).sum())
            state = (cam, hits, value, moments, length)
        d = (value.astype(np.float64) - truth)[live]
        print(f"   {label:22s} RMSE {np.sqrt(np.mean(d * d)):.4f}, mean length {float(length[live].mean()):.2f}, "
              f"{clipped} clips over the 8 frames of {int(live.sum())} live pixels")


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------

def scenes(shift):
    """(name, previous HostScene, current HostScene) of the three measured scenes"""
    import motion_scenes
    from tilecoderaytracer_amd import HostScene
    for name in ("builtin", "grid32"):
        prev, cur = HostScene.named(name), HostScene.named(name)
        desc = cur.desc.contents
        for k in range(desc.n_objects):
            if desc.objects[k].kind == 0 and not desc.objects[k].is_light:
                desc.objects[k].origin[0] = float(F(desc.objects[k].origin[0]) + F(shift))
        yield name, prev, cur, None
    yield ("motion scene", motion_scenes.host(motion_scenes.REST), motion_scenes.host(motion_scenes.SHIFTED),
           motion_scenes.camera_pair("equal")[1])


def gpu_tables(args):
    import torch
    from temporal_experiments import fmt, interleaved
    from tilecoderaytracer_amd import Renderer, TemporalHistory, capi, object_motions
    from tilecoderaytracer_amd.renderer import clamp_params, svgf_params, temporal_params
    W = H = args.size
    N = W * H
    lib = capi.load_library()
    variants = hasattr(lib, "rt_internal_clamp_variant")
    if variants:
        lib.rt_internal_clamp_variant.argtypes, lib.rt_internal_clamp_variant.restype = [C.c_int], C.c_int
    forms = (("direct", 0), ("LDS", 1)) if variants else (("as built", None),)
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# rt_history_clamp_device, {W} x {H}, depth {args.depth}, {torch.cuda.get_device_name(0)}; device time between events, "
          f"median (min, max) of {args.reps} interleaved repetitions; min_taps 3, clip_history 4, normal_cos 0.9, match_color 1, "
          f"gamma 1; " + ("both forms of the window's reads" if variants else "the library's own form only (no -DRT_CLAMP_VARIANTS=1 build)"))
    new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
    for name, host_prev, host_cur, camera in scenes(args.shift):
        table = object_motions(host_prev.desc, host_cur.desc)
        cam = capi.RtCameraDesc()
        C.memmove(C.byref(cam), C.byref(camera) if camera is not None else host_cur.camera, C.sizeof(cam))
        frames = []
        for host in (host_prev, host_cur):
            r = Renderer(host)
            own, r._cam = r._cam, C.pointer(cam)
            colours, records = new(N * 3), new(N * 12, torch.int32)
            r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), records.data_ptr(), stream)
            torch.cuda.synchronize()
            r._cam = own
            r.close()
            frames.append((colours, records))
        d_table = torch.tensor(table.reshape(-1), device="cuda")
        print(f"\n== {name} {W}x{H} depth {args.depth}: {table.shape[0]} objects, "
              f"{int((table != np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=F)).any(axis=1).sum())} of them moved")
        for channels in (3, 1):
            term = lambda c: c if channels == 3 else (c.view(N, 3) * torch.tensor([0.25, 0.5, 0.25], device="cuda")).sum(dim=1)
            before, cur = term(frames[0][0]), term(frames[1][0])
            history = TemporalHistory(W, H, channels, match_color=True)
            for _ in range(args.frames):
                history.push_device(before, frames[0][1], cam)
            history.push_device(cur, frames[1][1], cam, motions=d_table)
            torch.cuda.synchronize()
            s, old = history._sets[history.frames % 2], history._sets[(history.frames + 1) % 2]
            out = [new(N * channels), new(N * 2), new(N), new(N), new(N, torch.uint8)]
            other = [new(N * channels), new(N * 2), new(N), new(N), new(N, torch.uint8)]
            tp, sp = temporal_params(channels, match_color=True), svgf_params(channels, 1)
            scratch = new(int(lib.rt_svgf_scratch_bytes(C.byref(sp), W, H)), torch.uint8)
            traffic = BYTES[channels] * N
            half, half2 = new(traffic // 8, torch.int32), new(traffic // 8, torch.int32)

            def clamp(box, radius, form, to=out):
                p = clamp_params(channels, box=box, radius=radius)

                def call():
                    if form is not None:
                        lib.rt_internal_clamp_variant(form)
                    capi.check(lib.rt_history_clamp_device(0, C.byref(p), W, H, cur.data_ptr(), s["hits"].data_ptr(), s["value"].data_ptr(),
                                                           s["moments"].data_ptr(), s["length"].data_ptr(), *[t.data_ptr() for t in to],
                                                           stream))
                return call

            fns = {"copy": lambda: half2.copy_(half),
                   "rt_motion_accumulate_device": lambda: capi.check(lib.rt_motion_accumulate_device(
                       0, C.byref(tp), C.byref(cam), C.byref(cam), W, H, 0, W, d_table.data_ptr(), table.shape[0], cur.data_ptr(),
                       s["hits"].data_ptr(), old["hits"].data_ptr(), old["value"].data_ptr(), old["moments"].data_ptr(),
                       old["length"].data_ptr(), *[t.data_ptr() for t in other], stream)),
                   "rt_svgf_filter_device, 1 iteration": lambda: capi.check(lib.rt_svgf_filter_device(
                       0, C.byref(sp), W, H, s["value"].data_ptr(), s["hits"].data_ptr(), s["moments"].data_ptr(), s["length"].data_ptr(),
                       other[0].data_ptr(), other[3].data_ptr(), None, scratch.data_ptr(), stream))}
            for box, radius in SETTINGS:
                for label, form in forms:
                    fns[f"clamp box {box} r {radius} {label}"] = clamp(box, radius, form)
            res = interleaved(fns, args.reps)
            print(f"-- {channels} channel(s): a history of {args.frames} frames of the previous pose, then the moved frame; the call moves "
                  f"{BYTES[channels]} bytes a pixel, {traffic / 1e6:.1f} MB")
            for k, t in res.items():
                print(f"   {k:40s} {fmt(t)}  {t[0] / res['copy'][0]:5.2f} x the copy")
            rec = frames[1][1].view(N, 12)
            live = (rec[:, 0] >= 0) & ((rec[:, 11] & 2) == 0)
            for box, radius in SETTINGS:
                clamp(box, radius, forms[0][1])()
                torch.cuda.synchronize()
                flags = out[4]
                line = (f"   box {box} r {radius}: clipped {int((flags == 1).sum())} of {N} pixels ({100.0 * float((flags == 1).sum()) / N:.3f} %), "
                        f"{int((flags == 2).sum())} left for fewer than 3 taps; {int(live.sum())} live")
                if variants:
                    clamp(box, radius, 1, other)()
                    torch.cuda.synchronize()
                    same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(out, other))
                    line += f"; the two forms' outputs are {'equal word for word' if same else 'DIFFERENT'}"
                print(line)
            del history, out, other, scratch, half, half2
            torch.cuda.empty_cache()
        del frames
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--shift", type=float, default=0.05)
    ap.add_argument("--cpu", action="store_true", help="the reference's tables only; needs no GPU")
    args = ap.parse_args()
    return cpu_tables() if args.cpu else gpu_tables(args)


if __name__ == "__main__":
    main()
