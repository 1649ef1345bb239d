#!/usr/bin/env python3
"""Regenerate the fixtures that the reference itself wrote: tests/golden/ref/ and the three survey frames tests/golden/*.f32.

Everything stored here is output of oracle/_ref/ref_harness, a build of the reference's own sources (`make -C oracle ref`),
or an input handed to it (scene files, rays, segments).  No oracle, query_ref or GPU result is ever written: the oracle is used
only to lay out inputs (where the spheres, planes and lights of a scene are).  Without the binary this script refuses to run.

  *.scene                 the scenes, as building verbs (tests/ref_lib.py)
  *.f32 (frames)          ref_lib.FRAMES: packed fp32 [x][z][3]
  NAME.rays.f32           ref_lib.BATCHES: 1 024 rays {E, T}; NAME.hits.bin the reference's getCollision records (rt_hit),
  NAME.colours.f32        its calculatePixel colours at depth 3; NAME.segs.f32 as many segments (from the reference's own hit
  NAME.verdicts.u8        points to the lights) with its inShadeCollisionDetection verdicts
  digests.json            SHA-256, NaN count and "FAILURE" diagnostic count of the reference's frame for every case of
                          ref_lib.sweep_cases(); a frame that holds a NaN is stored whole instead (shrunk until it fits)

A second run must leave `git diff` empty."""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_lib  # noqa: E402


def reference_twice(what, *args, **kw):
    """the reference's answer, asked twice: (array, failures), or raises ReferenceFailed (a crash, a timeout, or two answers)"""
    a, fa = ref_lib.run_reference(*args, **kw)
    b, fb = ref_lib.run_reference(*args, **kw)
    if a.tobytes() != b.tobytes() or fa != fb:
        raise ref_lib.ReferenceFailed(f"{what}: two runs of the reference gave different bytes")
    return a, fa


def write(path, data):
    assert len(data) <= ref_lib.MAX_FIXTURE_BYTES, (path, len(data))
    with open(path, "wb") as f:
        f.write(data)


def main():
    if not ref_lib.have_binary():
        sys.exit(f"{ref_lib.REF_BINARY} is missing: `make -C oracle ref` builds it from the reference's sources; "
                 "these fixtures are written by the reference and by nothing else")
    os.makedirs(ref_lib.GOLDEN_REF, exist_ok=True)

    # named frames (no exclusions allowed: a failure here stops the script)
    for key, (make, W, H, depth, _) in ref_lib.FRAMES.items():
        rec = make()
        rec.write(ref_lib.scene_path(key))
        frame, failures = reference_twice(key, ref_lib.scene_path(key), W, H, depth)
        write(ref_lib.frame_path(key), frame.tobytes())
        print(f"frame {key}: {W}x{H} d{depth} sha256 {hashlib.sha256(frame.tobytes()).hexdigest()[:12]} "
              f"nans {ref_lib.count_nans(frame)} failures {failures}")

    # ray and segment batches
    for seed, (name, key) in enumerate(ref_lib.BATCHES.items()):
        oscene = ref_lib.load_scene(ref_lib.scene_path(key))
        rays = ref_lib.batch_rays(name, oscene, 100 + seed)
        hits, _ = reference_twice(name, ref_lib.scene_path(key), mode="hits", rays=rays)
        colours, _ = reference_twice(name, ref_lib.scene_path(key), depth=ref_lib.BATCH_DEPTH, mode="trace", rays=rays)
        segs = ref_lib.batch_segments(name, oscene, hits, 200 + seed)
        verdicts, _ = reference_twice(name, ref_lib.scene_path(key), mode="occluded", rays=segs)
        write(ref_lib.batch_path(name, "rays.f32"), rays.tobytes())
        write(ref_lib.batch_path(name, "hits.bin"), hits.tobytes())
        write(ref_lib.batch_path(name, "colours.f32"), colours.tobytes())
        write(ref_lib.batch_path(name, "segs.f32"), segs.tobytes())
        write(ref_lib.batch_path(name, "verdicts.u8"), verdicts.astype(np.uint8).tobytes())
        print(f"batch {name}: {int((hits['object'] >= 0).sum())} hits, {int(verdicts.sum())} occluded of {len(rays)}")

    # the sweep
    cases, excluded = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        scene_file = os.path.join(tmp, "case.scene")
        for cid, make, W, H, depth, is_seed in ref_lib.sweep_cases():
            make().write(scene_file)
            try:
                frame, failures = reference_twice(cid, scene_file, W, H, depth)
            except ref_lib.ReferenceFailed as e:
                if not is_seed:
                    raise
                excluded[cid] = str(e).split(":")[0]
                continue
            entry = {"W": W, "H": H, "depth": depth, "nans": ref_lib.count_nans(frame), "failures": failures}
            if entry["nans"]:
                # NaN payload bits are not portable: no digest; the frame itself, at a size that fits
                while W * H * 12 > ref_lib.MAX_FIXTURE_BYTES:
                    W, H = max(W // 2, 1), max(H // 2, 1)
                frame, failures = reference_twice(cid, scene_file, W, H, depth)
                entry.update(W=W, H=H, nans=ref_lib.count_nans(frame), failures=failures, sha256=None, frame=f"sweep_{cid}.f32")
                write(os.path.join(ref_lib.GOLDEN_REF, entry["frame"]), frame.tobytes())
            else:
                entry["sha256"] = hashlib.sha256(frame.tobytes()).hexdigest()
            cases[cid] = entry
    assert len(excluded) <= ref_lib.MAX_EXCLUDED_SEEDS, excluded
    doc = {"_about": "Written by tests/golden/make_ref_pins.py from oracle/_ref/ref_harness, a build of the reference's own "
                     "sources: SHA-256 of its packed fp32 frame for every case of ref_lib.sweep_cases(), with the number of NaN "
                     "values in the frame and of the reference's own FAILURE diagnostics.  excluded: seeds on which the "
                     "reference itself crashed, timed out or gave two answers (at most 2 % of the sweep's seeds).",
           "cases": cases, "excluded": excluded}
    with open(os.path.join(ref_lib.GOLDEN_REF, "digests.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"sweep: {len(cases)} cases, {len(excluded)} excluded, {sum(1 for c in cases.values() if c['nans'])} with NaNs, "
          f"{sum(1 for c in cases.values() if c['failures'])} with FAILURE diagnostics")


if __name__ == "__main__":
    main()
