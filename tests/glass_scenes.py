"""The scenes of the glass-record tests (include/rt_glass.h): mirror_scenes.py's room -- two facing full mirrors, a half-mirror
floor, walls, spheres, a light -- and, in front of part of it, a finite checkerboard pane (tf 0.9, rf 0.1) through which the far
mirror and a sphere are seen, a glass sphere (tf 0.9, ior 1.5), a "bubble" (tf 0.9, ior 0.75: its rim reflects totally, so
candidates there have no child), and a small tilted mirror high on the right that shows the pane: 18 objects.  A frame then has
chains through the pane alone, through a sphere, pane then mirror, mirror then pane, and -- pane, far mirror, pane, back mirror
-- chains cut at max_bounces = 4 with glass behind them (test_glass_cpu.py holds the reference to that).  "room" is the same
room without the four, non-refractive.  Cameras and sizes are mirror_scenes.py's.

Two more keys hold the step to what the glass room never asks of it (test_glass_cpu.py counts each category):
  "edges" is the glass room with other materials: seven refractive entries with tf 0.9, 0.6, 0.45, 0.3, 0.2 and 0, so that
      min_transmissive has five thresholds to sit on and one ulp above; the glass sphere (rf 0.7) and the far mirror (rf 1) and
      the floor (rf 0.5) qualify as glass and as a mirror at once; the bubble is a full mirror, so its rim -- candidates without
      a child -- is followed as a mirror; the far mirror is a finite plane and the floor an infinite plane that are glass; the
      red sphere is listed with tf 0 (never a candidate, whatever min_transmissive); the yellow sphere has ior exactly 1.
  "open" has no walls -- the room's light, the far mirror, the pane, the glass sphere and one diffuse sphere -- so that chains
      which followed something end in a miss."""
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
FAR_MIRROR, FLOOR, RED_SPHERE, CLEAR_SPHERE = mirror_scenes.FAR_MIRROR, 3, 9, 11  # the room's own, made refractive in "edges"
EDGES_REFLECTIVE = {GLASS_SPHERE: 0.7, BUBBLE: 1.0}                               # rf that "edges" changes
EDGES_REFRACTIVE = [(PANE, TF, 1.0), (GLASS_SPHERE, 0.6, 1.5), (BUBBLE, 0.3, 0.75), (FAR_MIRROR, 0.45, 1.0), (FLOOR, 0.2, 1.0),
                    (RED_SPHERE, 0.0, 1.3), (CLEAR_SPHERE, 0.6, 1.0)]
EDGES_TF = (0.2, 0.3, 0.45, 0.6, 0.9)                                             # its thresholds, ascending
OPEN_MIRROR, OPEN_PANE, OPEN_GLASS_SPHERE, OPEN_SPHERE = 1, 2, 3, 4               # "open"'s Scene indices, after its light
OPEN_REFRACTIVE = [(OPEN_PANE, TF, 1.0), (OPEN_GLASS_SPHERE, TF, 1.5)]
KEYS = ("glass", "edges", "open")


def up(x):
    """the float32 next above float32(x), as a Python float"""
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


# min_transmissive of the "edges" tests: below every tf (all the same words), and every threshold with its up()
EDGES_LOOKS = (-float("inf"), -1.0, 0.0) + tuple(v for tf in EDGES_TF for v in (tf, up(tf))) + (float("inf"),)
EDGES_FLOORS = (0.05, 0.5, 0.7, 1.0)


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


def build_edges(scene):
    """the glass room with "edges"' materials -> its refractive list"""
    build_glass_room(scene)
    for o, rf in EDGES_REFLECTIVE.items():
        scene.set_reflective(o, rf)
    return list(EDGES_REFRACTIVE)


def build_open(scene):
    """the room's light and far mirror, the glass room's pane and glass sphere, and the room's blue sphere: nothing behind them"""
    i = scene.add_sphere((0.5, 4.0, 5.2), f32(0.15))
    scene.set_light(i)
    scene.set_intensity(i, 1.0)
    i = scene.add_finite_plane_corners((-4.0, 10.0, 0.25), (-4.0, 10.0, 5.0), (4.0, 10.0, 0.25))
    assert i == OPEN_MIRROR
    scene.set_color(i, (1, 1, 1))
    scene.set_reflective(i, 1.0)
    scene.set_diffuse(i, 0.0)
    i = scene.add_finite_plane_corners((-3.2, 4.5, 0.6), (-3.2, 4.5, 4.4), (-0.4, 4.5, 0.6))
    assert i == OPEN_PANE
    scene.set_checkerboard(i, (0.9, 0.95, 1.0), (0.6, 0.7, 0.8), 0.7, 0.7)
    scene.set_reflective(i, 0.1)
    scene.set_diffuse(i, 0.1)
    i = scene.add_sphere((1.0, 3.0, 1.4), f32(0.6))
    assert i == OPEN_GLASS_SPHERE
    scene.set_color(i, (1, 1, 1))
    scene.set_diffuse(i, 0.1)
    scene.set_specular(i, 0.3)
    i = scene.add_sphere((1.8, 7.5, 1.2), f32(1.2))
    assert i == OPEN_SPHERE
    scene.set_color(i, (0, 0, 1))
    scene.set_specular(i, 0.3)
    scene.set_object_indices(0, 1)
    return list(OPEN_REFRACTIVE)


BUILDERS = {"glass": build_glass_room, "edges": build_edges, "open": build_open}


def oracle_scene(key):
    """key "glass", "edges", "open" or "room" -> (an OracleScene under the room's first camera, its refractive list)"""
    if key == "room":
        return mirror_scenes.oracle_scene("room"), []
    orc = oracle_lib.OracleScene()
    refr = BUILDERS[key](orc)
    cameras.put(room_cameras()[0], orc=orc)
    return orc, refr


def host_scene(key):
    """-> (a HostScene, its refractive list)"""
    from tilecoderaytracer_amd import HostScene
    if key == "room":
        return mirror_scenes.host_scene("room"), []
    host = HostScene.empty()
    refr = BUILDERS[key](host)
    cameras.put(room_cameras()[0], host=host)
    return host, refr


@functools.lru_cache(maxsize=None)
def ref_scene(key):
    orc, refr = oracle_scene(key)
    return refract_ref.Scene(orc, {o: (tf, ior) for o, tf, ior in refr})


@functools.lru_cache(maxsize=None)
def pixel_rays(key, W, H, camera=0):
    """the (W, H, 6) pixel rays under the room's camera 0 or 1 (the same for every key), read-only"""
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


LARGE = dict(bounces=8, floor=0.5, look=0.5)                # test_glass_large_gpu.py's call
# large_tile_figures() of its batch: test_glass_cpu.py holds the reference to them, the large test asserts them again
LARGE_FIGURES = dict(alive=[7679, 5319, 2632, 1039, 577, 288, 148, 111, 64], cut=47, g=3495,
                     glass_steps=[3007, 288, 367, 177, 76, 55, 24, 23], glass_sphere=627, bubble=123, childless=85)


def large_tile():
    """the batch of test_glass_large_gpu.py: the glass room's 96 x 80 pixel rays, flat, cut to mirror_large.TILE_RAYS, under
    LARGE -> (rays float32 (M, 6), {output: its reference as int32 words (M, words a ray)}, the reference's details of those M
    rays, flat)"""
    import mirror_large
    W, H = SIZES[1]
    ref = reference("glass", W, H, LARGE["bounces"], LARGE["floor"], LARGE["look"])
    rays, words = mirror_large.room_tile(LARGE["bounces"], LARGE["floor"], (pixel_rays("glass", W, H), ref))
    details = {name: a.reshape((W * H,) + a.shape[2:])[:len(rays)] for name, a in ref[4].items()}
    return rays, words, details


def large_tile_figures(words, details):
    """what test_glass_large_gpu.py needs of large_tile()'s reference, so that it cannot pass vacuously:
    mirror_large.tile_preconditions (no sentinel word, no NaN; the chains of length >= b, the chains cut at the limit) and the
    counts of what only a glass chain has"""
    import mirror_large
    alive, cut = mirror_large.tile_preconditions(words)
    chain, glass = details["chain"], details["glass"]
    through = lambda o: int(((chain == o) & glass).any(-1).sum())
    return dict(alive=alive, cut=cut, g=int(details["g"].sum()), glass_steps=[int(c) for c in glass.sum(0)],
                glass_sphere=through(GLASS_SPHERE), bubble=through(BUBBLE), childless=int((details["childless"] > 0).sum()))


__all__ = ["SIZES", "EXTENT", "TRUCK", "PANE", "GLASS_SPHERE", "BUBBLE", "SIDE_MIRROR", "REFRACTIVE", "build_glass_room",
           "FAR_MIRROR", "FLOOR", "RED_SPHERE", "CLEAR_SPHERE", "EDGES_REFLECTIVE", "EDGES_REFRACTIVE", "EDGES_TF", "EDGES_LOOKS",
           "EDGES_FLOORS", "OPEN_MIRROR", "OPEN_PANE", "OPEN_GLASS_SPHERE", "OPEN_SPHERE", "OPEN_REFRACTIVE", "up", "build_edges",
           "build_open", "KEYS", "LARGE", "LARGE_FIGURES", "large_tile", "large_tile_figures",
           "oracle_scene", "host_scene", "ref_scene", "pixel_rays", "reference", "room_cameras"]
