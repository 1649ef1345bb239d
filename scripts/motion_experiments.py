"""What profiles/motion_experiments.txt records (include/rt_motion.h): at 4096 x 4096, depth 4, three channels, on the built-in
scene and the 1024-sphere grid, a history of six frames -- rt_motion_accumulate_device against rt_temporal_accumulate_device and
against a device copy of the bytes the kernel moves, under equal cameras (no table, n_motions 0, an all-identity table, every
sphere translated by 0.05 units) and under a camera trucked by 0.3 units (the existing call; the table of translated spheres);
and the two ways of reading the table, (a) global memory and (b) LDS, for tables on both sides of (b)'s limit of 170 entries.  The
moved frames are real ones: the current records are rendered from a scene whose spheres stand 0.05 units further along x, the
previous ones from the scene as it is, and the table is object_motions() of the two.  Every time is device time between events
around one device call, the median, minimum and maximum of REPS interleaved repetitions after a warm-up; one process, nothing
downloaded inside a timed window.  The comparison of the table paths needs both, which only a build with -DRT_MOTION_VARIANTS=1
has:

    make -C tilecoderaytracer_amd/csrc variant NAME=motion_variants DEFS=-DRT_MOTION_VARIANTS=1
    TCRT_LIBRARY=tilecoderaytracer_amd/lib/variants/libtcrt_motion_variants.so \
    timeout 900 python scripts/motion_experiments.py [--size 4096] [--reps 21] >> profiles/motion_experiments.txt
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from temporal_experiments import fmt, interleaved, trucked  # noqa: E402
from tilecoderaytracer_amd import HostScene, Renderer, capi, object_motions  # noqa: E402
from tilecoderaytracer_amd.renderer import temporal_params  # noqa: E402

GLOBAL, LDS, LDS_ENTRIES = 1, 2, 170
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--shift", type=float, default=0.05)
    args = ap.parse_args()
    W = H = args.size
    N = W * H
    lib = capi.load_library()
    variants = hasattr(lib, "rt_internal_motion_variant")
    if variants:
        lib.rt_internal_motion_variant.argtypes = lib.rt_motion_accumulate_device.argtypes + [C.c_int]
        lib.rt_internal_motion_variant.restype = C.c_int
    stream = torch.cuda.current_stream().cuda_stream
    print(f"# motion accumulation, {W} x {H}, depth {args.depth}, 3 channels, {torch.cuda.get_device_name(0)}; device time between "
          f"events, median (min, max) of {args.reps} interleaved repetitions; " +
          ("both table paths" if variants else "the library's own table path only (no -DRT_MOTION_VARIANTS=1 build)"))
    params = temporal_params(3, False, 32, 0.9, 0.05, 0.0, 0.0)
    new = lambda words, dtype=torch.float32: torch.empty((words,), dtype=dtype, device="cuda")
    for scene in ("builtin", "grid32"):
        host_prev, host_cur = HostScene.named(scene), HostScene.named(scene)
        desc = host_cur.desc.contents
        spheres = [k for k in range(desc.n_objects) if desc.objects[k].kind == 0 and not desc.objects[k].is_light]
        for k in spheres:                                        # the current pose: every sphere args.shift further along x
            desc.objects[k].origin[0] = float(np.float32(desc.objects[k].origin[0]) + np.float32(args.shift))
        table = object_motions(host_prev.desc, host_cur.desc)
        n_objects = table.shape[0]
        assert (table[spheres, 3] != 0).all() and (np.delete(table, spheres, axis=0) == IDENTITY).all()
        cam = capi.RtCameraDesc()
        C.memmove(C.byref(cam), host_cur.camera, C.sizeof(cam))
        cam_truck = trucked(cam, -0.3)                           # the PREVIOUS camera of the trucked cases
        r_prev, r_cur = Renderer(host_prev), Renderer(host_cur)
        colours = new(N * 3)

        def records(r, c):
            out = new(N * 12, torch.int32)
            own = r._cam
            r._cam = C.pointer(c)
            r.render_gbuffer_device(W, H, args.depth, 0, W, colours.data_ptr(), out.data_ptr(), stream)
            r._cam = own
            return out

        cur = records(r_cur, cam)                                # (colours: the current frame's, rendered last)
        prev_static = {"equal": cur, "truck": records(r_cur, cam_truck)}      # nothing moved between the frames
        prev_moved = {"equal": records(r_prev, cam), "truck": records(r_prev, cam_truck)}
        cur = records(r_cur, cam)
        prev = [torch.rand((N * k,), dtype=torch.float32, device="cuda") for k in (3, 2, 1)]
        prev[2].mul_(5.0).add_(1.0)                              # a history of up to six frames
        out = [new(N * 3), new(N * 2), new(N), new(N), new(N, torch.uint8)]
        pad = lambda t, n: np.concatenate([t, np.tile(IDENTITY, (max(n - len(t), 0), 1))])[:max(n, len(t))]
        d_table = lambda t: torch.tensor(np.ascontiguousarray(t).reshape(-1), device="cuda")
        tables = {"moved": d_table(table), "identity": d_table(np.tile(IDENTITY, (n_objects, 1)))}
        traffic = (48 + 12 + 48 + 12 + 8 + 4 + 12 + 8 + 4 + 4 + 1) * N
        half, half2 = new(traffic // 8, torch.int32), new(traffic // 8, torch.int32)
        print(f"\n== {scene} {W}x{H} depth {args.depth}: {n_objects} objects, {len(spheres)} spheres moved by {args.shift} along x; the "
              f"kernel's traffic without a table {traffic / 1e6:.1f} MB (161 bytes a pixel); the copy moves the same")

        def temporal(cams, prev_records):
            return lambda: capi.check(lib.rt_temporal_accumulate_device(
                0, C.byref(params), C.byref(cams), C.byref(cam), W, H, 0, W, colours.data_ptr(), cur.data_ptr(), prev_records.data_ptr(),
                prev[0].data_ptr(), prev[1].data_ptr(), prev[2].data_ptr(), *[t.data_ptr() for t in out], stream))

        def motion(cams, prev_records, t, n, path=None):
            head = (0, C.byref(params), C.byref(cams), C.byref(cam), W, H, 0, W, t.data_ptr() if t is not None else None, n,
                    colours.data_ptr(), cur.data_ptr(), prev_records.data_ptr(), prev[0].data_ptr(), prev[1].data_ptr(),
                    prev[2].data_ptr(), *[t_.data_ptr() for t_ in out], stream)
            if path is None:
                return lambda: capi.check(lib.rt_motion_accumulate_device(*head))
            return lambda: capi.check(lib.rt_internal_motion_variant(*head, path))

        # ---- 1. the static calls and the moved frame against the existing call and the copy ------------------------------------
        fns = {"copy": lambda: half2.copy_(half),
               "equal  rt_temporal_accumulate_device": temporal(cam, prev_static["equal"]),
               "equal  motion, n_motions 0": motion(cam, prev_static["equal"], None, 0),
               "equal  motion, all-identity table": motion(cam, prev_static["equal"], tables["identity"], n_objects),
               "equal  motion, spheres moved": motion(cam, prev_moved["equal"], tables["moved"], n_objects),
               "truck  rt_temporal_accumulate_device": temporal(cam_truck, prev_static["truck"]),
               "truck  motion, spheres moved": motion(cam_truck, prev_moved["truck"], tables["moved"], n_objects)}
        res = interleaved(fns, args.reps)
        base = {"equal": res["equal  rt_temporal_accumulate_device"][0], "truck": res["truck  rt_temporal_accumulate_device"][0]}
        for k, t in res.items():
            ratio = "" if k == "copy" else f"  {t[0] / base[k[:5]]:5.3f} x rt_temporal_accumulate_device"
            print(f"   {k:40s} {fmt(t)}  {t[0] / res['copy'][0]:5.2f} x the copy{ratio}")
        rec = cur.view(N, 12)
        live = (rec[:, 0] >= 0) & ((rec[:, 11] & 2) == 0)
        on_spheres = live & torch.isin(rec[:, 0], torch.tensor(spheres, dtype=torch.int32, device="cuda"))
        for k in ("equal  motion, all-identity table", "equal  motion, spheres moved", "truck  rt_temporal_accumulate_device",
                  "truck  motion, spheres moved"):
            fns[k]()
            torch.cuda.synchronize()
            lost = out[4].bool()
            print(f"   {k}: {int(on_spheres.sum())} of {N} pixels on moved spheres, {int((lost & on_spheres).sum())} of them and "
                  f"{int((lost & live & ~on_spheres).sum())} other live pixels without history")
        for name, cams in (("equal", cam), ("truck", cam_truck)):
            temporal(cams, prev_moved[name])()
            torch.cuda.synchronize()
            print(f"   {name}  the moved frame through rt_temporal_accumulate_device, as a caller without a table has it: "
                  f"{int((out[4].bool() & on_spheres).sum())} of the spheres' pixels without history")

        # ---- 2. the table paths: (a) global memory, (b) LDS -------------------------------------------------------------------
        if variants:
            fns = {"equal  rt_temporal_accumulate_device": temporal(cam, prev_static["equal"])}
            sizes = sorted({min(n_objects, LDS_ENTRIES), LDS_ENTRIES} | {LDS_ENTRIES + 1, 4096})
            for n in sizes:
                if n < n_objects and n <= LDS_ENTRIES:
                    continue                                     # (a table cut short of the scene's objects is another frame)
                t = d_table(pad(table, n))
                for cams, name in ((cam, "equal"), (cam_truck, "truck")):
                    fns[f"{name}  (a) global, n_motions {max(n, n_objects)}"] = motion(cams, prev_moved[name], t, max(n, n_objects), GLOBAL)
                    if max(n, n_objects) <= LDS_ENTRIES:
                        fns[f"{name}  (b) LDS,    n_motions {n}"] = motion(cams, prev_moved[name], t, n, LDS)
            res = interleaved(fns, args.reps)
            for k, t in res.items():
                print(f"   {k:40s} {fmt(t)}")
        del half, half2, prev, out, prev_static, prev_moved, cur, colours
        r_prev.close(), r_cur.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
