"""The scenes of the glass-record tests (include/rt_glass.h): mirror_scenes.py's room -- two facing full mirrors, a half-mirror
floor, walls, spheres, a light -- and, in front of part of it, a finite checkerboard pane (tf 0.9, rf 0.1) through which the far
mirror and a sphere are seen, a glass sphere (tf 0.9, ior 1.5), a "bubble" (tf 0.9, ior 0.75: its rim reflects totally, so
candidates there have no child), and a small tilted mirror high on the right that shows the pane: 18 objects.  A frame then has
chains through the pane alone, through a sphere, pane then mirror, mirror then pane, and -- pane, far mirror, pane, back mirror
-- chains cut at max_bounces = 4 with glass behind them (test_glass_cpu.py holds the reference to that).  "room" is the same
room without the four, non-refractive.  Cameras and sizes are mirror_scenes.py's."""
import functools

import numpy as np

import cameras
import mirror_scenes
import oracle_lib
import refract_ref
from mirror_scenes import EXTENT, SIZES, TRUCK, room_cameras
from rays_ref import camera_rays
from scene_gen import f32

PANE, GLASS_SPHERE, BUBBLE, SIDE_MIRROR = 14, 15, 16, 17      # Scene indices, after the room's 14
TF = 0.9
REFRACTIVE = [(PANE, TF, 1.0), (GLASS_SPHERE, TF, 1.5), (BUBBLE, TF, 0.75)]       # (object, tf, ior)


def _side_mirror_corners():
    """a 1.6 x 1.6 mirror centred at c whose normal bisects the directions to the eye and to the pane's middle"""
    c = np.array([2.2, 8.0, 4.0])
    to_eye = np.array([0.0, -1.0, 2.5]) - c
    to_pane = np.array([-1.8, 4.5, 2.5]) - c
    n = to_eye / np.linalg.norm(to_eye) + to_pane / np.linalg.norm(to_pane)
    n /= np.linalg.norm(n)
    h = np.cross(n, [0.0, 0.0, 1.0])
    h /= np.linalg.norm(h)
    v = np.cross(h, n)
    o = c - 0.8 * h - 0.8 * v
    return tuple(tuple(float(f32(x)) for x in p) for p in (o, o + 1.6 * v, o + 1.6 * h))


def build_glass_room(scene):
    """mirror_scenes.build_room and the four objects above -> the refractive list [(object, tf, ior)]"""
    mirror_scenes.build_room(scene)
    i = scene.add_finite_plane_corners((-3.2, 4.5, 0.6), (-3.2, 4.5, 4.4), (-0.4, 4.5, 0.6))
    assert i == PANE
    scene.set_checkerboard(i, (0.9, 0.95, 1.0), (0.6, 0.7, 0.8), 0.7, 0.7)
    scene.set_reflective(i, 0.1)
    scene.set_diffuse(i, 0.1)
    for want, o, r, colour in ((GLASS_SPHERE, (1.0, 3.0, 1.4), 0.6, (1, 1, 1)), (BUBBLE, (2.2, 4.5, 1.6), 0.5, (0.9, 1, 0.9))):
        i = scene.add_sphere(o, f32(r))
        assert i == want
        scene.set_color(i, colour)
        scene.set_diffuse(i, 0.1)
        scene.set_specular(i, 0.3)
    i = scene.add_finite_plane_corners(*_side_mirror_corners())
    assert i == SIDE_MIRROR
    scene.set_color(i, (1, 1, 1))
    scene.set_reflective(i, 1.0)
    scene.set_diffuse(i, 0.0)
    scene.set_object_indices(0, 1)
    return list(REFRACTIVE)


def oracle_scene(key):
    """key "glass" or "room" -> (an OracleScene under the room's first camera, its refractive list)"""
    if key == "room":
        return mirror_scenes.oracle_scene("room"), []
    assert key == "glass", key
    orc = oracle_lib.OracleScene()
    refr = build_glass_room(orc)
    cameras.put(room_cameras()[0], orc=orc)
    return orc, refr


def host_scene(key):
    """-> (a HostScene, its refractive list)"""
    from tilecoderaytracer_amd import HostScene
    if key == "room":
        return mirror_scenes.host_scene("room"), []
    assert key == "glass", key
    host = HostScene.empty()
    refr = build_glass_room(host)
    cameras.put(room_cameras()[0], host=host)
    return host, refr


@functools.lru_cache(maxsize=None)
def ref_scene(key):
    orc, refr = oracle_scene(key)
    return refract_ref.Scene(orc, {o: (tf, ior) for o, tf, ior in refr})


@functools.lru_cache(maxsize=None)
def pixel_rays(key, W, H, camera=0):
    """the (W, H, 6) pixel rays under the room's camera 0 or 1 (the same for both keys), read-only"""
    rays = camera_rays(room_cameras()[camera], W, H)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def reference(key, W, H, max_bounces, min_reflective=1.0, min_transmissive=0.5, camera=0):
    """glass_ref.records(..., details=True) of the frame's pixel rays, computed once, read-only"""
    import glass_ref
    out = glass_ref.records(ref_scene(key), pixel_rays(key, W, H, camera), max_bounces, min_reflective, min_transmissive,
                            details=True)
    for a in out[:4]:
        a.setflags(write=False)
    return out


__all__ = ["SIZES", "EXTENT", "TRUCK", "PANE", "GLASS_SPHERE", "BUBBLE", "SIDE_MIRROR", "REFRACTIVE", "build_glass_room",
           "oracle_scene", "host_scene", "ref_scene", "pixel_rays", "reference", "room_cameras"]
