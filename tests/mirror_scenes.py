"""The scenes of the mirror-record tests (include/rt_mirror.h): the built-in scene, and a small room built through scene_gen's
verbs on HostScene and OracleScene alike -- two facing planar full mirrors (a large one on the far wall, a larger one behind
the eye), a half-mirror floor (followed only with min_reflective <= 0.5), four diffuse walls and a ceiling, a few diffuse
spheres and a light: 14 objects.  The eye stands between the mirrors and looks at the far one, so that a frame has pixels that
follow no mirror, one, two, and more than max_bounces = 3 of them (test_mirror_cpu.py holds the reference to that).  Two
cameras: the second is the first trucked sideways."""
import functools

import numpy as np

import cameras
import oracle_lib
import query_ref
from rays_ref import camera_rays
from scene_gen import f32

SIZES = [(61, 37), (96, 80)]
EXTENT = 16.0                       # no coordinate of the room's surfaces inside the walls is larger
FAR_MIRROR, BACK_MIRROR = 1, 2      # Scene indices
TRUCK = 1.0


def build_room(scene):
    i = scene.add_sphere((0.5, 4.0, 5.2), f32(0.15))
    scene.set_light(i)
    scene.set_intensity(i, 1.0)
    # the far mirror, y = 10, x -4..4, z 0.25..5;  the back mirror, y = -3, x -5..5, z 0.1..5.5
    for o, vc, hc in (((-4.0, 10.0, 0.25), (-4.0, 10.0, 5.0), (4.0, 10.0, 0.25)),
                      ((-5.0, -3.0, 0.1), (-5.0, -3.0, 5.5), (5.0, -3.0, 0.1))):
        i = scene.add_finite_plane_corners(o, vc, hc)
        scene.set_color(i, (1, 1, 1))
        scene.set_reflective(i, 1.0)
        scene.set_diffuse(i, 0.0)
    g = scene.add_infinite_plane((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))              # the half-mirror floor
    scene.set_color(g, (0.33, 0.33, 0.33))
    scene.set_reflective(g, 0.5)
    scene.set_diffuse(g, 0.5)
    for o, n, h, colour in (((0.0, 0.0, 6.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (1, 1, 1)),      # ceiling
                            ((-7.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1, 0, 0)),      # left wall
                            ((7.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0, 1, 0)),      # right wall
                            ((0.0, 10.5, 0.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), (0, 1, 1)),     # far wall, behind its mirror
                            ((0.0, -3.5, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (1, 1, 0))):     # back wall, behind its mirror
        i = scene.add_infinite_plane(o, n, h)
        scene.set_color(i, colour)
    for o, r, colour in (((-2.2, 6.0, 0.8), 0.8, (1, 0, 0)), ((1.8, 7.5, 1.2), 1.2, (0, 0, 1)), ((0.3, 3.0, 0.4), 0.4, (1, 1, 0)),
                         ((-1.0, 1.0, 4.6), 0.5, (0, 1, 0)), ((2.5, -1.5, 3.0), 0.7, (1, 1, 1))):
        i = scene.add_sphere(o, f32(r))
        scene.set_color(i, colour)
        scene.set_specular(i, 0.3)
    scene.set_object_indices(0, 1)
    return scene


def room_cameras():
    """-> (the room's camera, the same trucked TRUCK to the right)"""
    return (cameras.camera((0.0, -1.0, 2.5), (0.0, 0.0, 2.5)), cameras.camera((TRUCK, -1.0, 2.5), (TRUCK, 0.0, 2.5)))


def oracle_scene(key):
    """key "builtin" or "room" -> an OracleScene under its first camera"""
    if key == "builtin":
        return oracle_lib.OracleScene.builtin()
    assert key == "room", key
    orc = build_room(oracle_lib.OracleScene())
    cameras.put(room_cameras()[0], orc=orc)
    return orc


def host_scene(key):
    from tilecoderaytracer_amd import HostScene
    if key == "builtin":
        return HostScene.builtin()
    assert key == "room", key
    host = build_room(HostScene.empty())
    cameras.put(room_cameras()[0], host=host)
    return host


@functools.lru_cache(maxsize=None)
def ref_scene(key):
    return query_ref.Scene(oracle_scene(key))


@functools.lru_cache(maxsize=None)
def pixel_rays(key, W, H, camera=0):
    """the (W, H, 6) pixel rays of scene `key` under its camera (the room: camera 0 or 1), read-only"""
    cam = room_cameras()[camera] if key == "room" else oracle_scene(key).cam
    rays = camera_rays(cam, W, H)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def reference(key, W, H, max_bounces, min_reflective=1.0, camera=0):
    """mirror_ref.records(..., details=True) of the frame's pixel rays, computed once, read-only"""
    import mirror_ref
    out = mirror_ref.records(ref_scene(key), pixel_rays(key, W, H, camera), max_bounces, min_reflective, details=True)
    for a in out[:4]:
        a.setflags(write=False)
    return out
