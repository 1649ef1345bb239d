"""The frames the adaptive-supersampling tests compare bit for bit (include/rt_capi_adaptive.h), from the CPU oracle alone: a
frame's colours (oracle_lib), its camera rays' records (query_ref.intersect) and its virtual k x k frame, each computed once."""
import functools

import numpy as np

import oracle_lib
import query_ref
import scene_gen
from rays_ref import camera_rays

# (key, W, H, depth, the flagged share at normal_cos 0.9 and color_threshold 1/32)
FRAMES = [
    ("builtin", 250, 252, 3, 0.171),
    ("builtin", 61, 37, 4, 0.477),
    ("grid16", 96, 96, 8, 0.619),
    ("grid32", 64, 64, 4, 0.680),
    ("random1", 36, 28, 5, 0.084),
    ("random2", 36, 28, 5, 0.381),
    ("random3", 36, 28, 5, 0.661),
]
# the frames of two options' kernels (tables = 2, cull = 0): no share is tabulated for them, the tests assert the condition
OPTION_FRAMES = [("twomirrors", 40, 36, 6), ("builtin", 70, 50, 4)]


def build(key, scene_cls, empty):
    """the scene `key` in scene_cls (HostScene or OracleScene; empty: its constructor of an empty scene)"""
    if key.startswith("random"):
        return scene_gen.build_random(empty(), int(key[len("random"):]))
    return scene_cls.named(key)


def oracle_scene(key):
    return build(key, oracle_lib.OracleScene, oracle_lib.OracleScene)


def host_scene(key):
    from tilecoderaytracer_amd import HostScene
    return build(key, HostScene, HostScene.empty)


@functools.lru_cache(maxsize=None)
def first_pass(key, W, H, depth):
    """-> (colours float32 (W, H, 3), records HIT_DTYPE (W, H)) of the oracle's frame, read-only"""
    orc = oracle_scene(key)
    rgb = orc.render(W, H, depth)
    hits = query_ref.intersect(query_ref.Scene(orc), camera_rays(orc.cam, W, H))
    rgb.setflags(write=False), hits.setflags(write=False)
    return rgb, hits


@functools.lru_cache(maxsize=None)
def supersampled(key, W, H, depth, k):
    """the oracle's virtual k W x k H frame, box-filtered (include/rt_capi_ssaa.h), read-only"""
    from ssaa_ref import box_filter
    out = np.ascontiguousarray(box_filter(oracle_scene(key).render(k * W, k * H, depth), k))
    out.setflags(write=False)
    return out
