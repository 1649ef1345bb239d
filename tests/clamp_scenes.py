"""The setting the clamp's conditions are counted on (include/rt_clamp.h; tests/test_clamp_cpu.py, scripts/clamp_experiments.py):
pose pairs of the motion tests' scene under equal cameras, the oracle's colours as the term, accumulated by the tests' references."""
import functools

import numpy as np

import cameras
import clamp_ref
import motion_ref
import motion_scenes
import temporal_ref

GHOST_PAIRS = ("spheres_equal", "sphere_leaves")
GHOST_KW = dict(box=0, radius=1, match_color=True)


@functools.lru_cache(maxsize=None)
def ghost_setting(name, W, H, frames=8):
    """The pose pair `name` of the motion scene under equal cameras, the oracle's colours at depth 4 as the term: `frames` frames
    of the previous pose accumulated with match_color, then one frame of the current pose pushed with the pair's motion table
    -> (cur, hits, value, moments, length of that frame, ghost: the pixels of static objects (object < 4) with history whose
    colour changed by more than 0.02 between the poses, unchanged: those whose colour did not change at all)"""
    assert motion_scenes.PAIRS[name][2] == "equal"
    cam_prev, cam, prev_hits, hits = motion_scenes.records(name, W, H)
    colours = []
    for pose, c in zip(motion_scenes.PAIRS[name][:2], (cam_prev, cam)):
        scene = motion_scenes.oracle(pose)
        cameras.put(c, orc=scene)
        colours.append(scene.render(W, H, 4))
    before, cur = colours
    state = None
    for _ in range(frames):
        value, moments, length, _, _ = temporal_ref.accumulate(before, prev_hits, cam_prev, state, match_color=True)
        state = (cam_prev, prev_hits, value, moments, length)
    value, moments, length, _, none = motion_ref.accumulate(cur, hits, cam, state, motion_scenes.table(name), match_color=True)
    change = np.abs(cur - before).max(axis=-1)
    static = (hits["object"] >= 0) & (hits["object"] < 4) & ~clamp_ref.dead_records(hits) & ~none
    out = (cur, hits, value, moments, length, static & (change > 0.02), static & (change == 0))
    for a in out:
        a.setflags(write=False)
    return out


def ghost_error(value, cur, ghost):
    """the mean over the ghost pixels of the channel-wise maximum of |value - current colour|"""
    return float(np.abs(value.astype(np.float64) - cur.astype(np.float64)).max(axis=-1)[ghost].mean())
