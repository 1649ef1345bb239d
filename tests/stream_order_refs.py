"""The pairs of calls that tests/test_stream_order_gpu.py issues on one handle with a change of stream between them, and the
reference of each call -- the suite's existing ones (lens_ref, indirect_ref, adaptive_ref, mirror_ref, glass_ref, query_ref, ao_ref
and the oracle's frames), from the CPU alone, each computed once and read-only.  Every call is a 61 x 37 frame, or that frame's
rays or records.  tests/test_stream_order_cpu.py holds what the GPU tests rely on: the two references of a pair differ in more
than half of their pixels or records, so that a test which confused the two calls could not pass, and none holds poisoned.py's
sentinel, so that an unwritten word shows.

reference(case, k) -> the tuple of arrays that call k (0 or 1) of PAIRS[case] must write, in the order of the call's outputs."""
import functools

import numpy as np

import adaptive_ref
import ao_ref
import cameras
import glass_scenes
import indirect_ref
import lens_ref
import mirror_ref
import mirror_scenes
import oracle_lib
import query_ref
import rays_ref
from ssaa_ref import box_filter

F = np.float32
INF = float("inf")
W, H = 61, 37
OTHER_CAMERA = "pitched_down"             # of cameras.catalogue("builtin"); None is the built-in scene's own
APERTURE, FOCUS = lens_ref.lens_of("builtin", cameras.ANCHORS["builtin"]["focus"])

# ---- the calls' parameters: call 2 has call 1's shape, and parameters that change most of what it writes ------------------------
LENS = dict(depth=2, samples=2, calls=(dict(seed=4, aperture=APERTURE), dict(seed=9, aperture=float(F(3.0 * APERTURE)))))
LENS_CHUNK_COLUMNS = 16                   # call 1 in four chunks
INDIRECT = dict(depth=4, samples=2, gather_depth=1, calls=(dict(seed=0, key0=0), dict(seed=5, key0=1000)))
ADAPTIVE = dict(depth=4, samples=2)
BOUNCES = 3
# (another floor alone changes 0.273 of the mirror records, another floor or min_transmissive alone 0.281 and 0.461 of the glass
# records: call 2 looks through the rooms' second camera as well)
MIRROR = dict(key="room", calls=(dict(min_reflective=0.5, camera=0), dict(min_reflective=1.0, camera=1)))
GLASS = dict(key="glass", min_reflective=0.5, calls=(dict(min_transmissive=0.5, camera=0), dict(min_transmissive=INF, camera=1)))
CROSSED = dict(key="glass", min_reflective=0.5, min_transmissive=0.5, cameras=(0, 1))   # (one camera: 0.461 of the records differ)
STACK_DEPTH = 8
DEPTH = 4
# (a value is one of 17, and most records are open at radius 1: another seed and key0 alone change 0.140 of them, radius 3 as
# well 0.747)
AO = dict(samples=4, calls=(dict(seed=1, key0=0, radius=1.0), dict(seed=2, key0=5000, radius=3.0)))
# (scene, camera, depth) of the four frames of two handles, in the order of the calls
TWO_HANDLES = (("builtin", None, 4), ("grid16", None, 4), ("builtin", OTHER_CAMERA, 4), ("grid16", "rolled_pi", 4))


def frozen(*arrays):
    out = tuple(np.ascontiguousarray(a) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def camera_desc(scene, camera):
    """camera None -> None (the scene's own); of the built-in scene: cameras.catalogue's; of the sphere grid "rolled_pi": the
    usual eye, upside down"""
    if camera is None:
        return None
    if scene == "builtin":
        return cameras.catalogue("builtin")[camera]
    assert (scene, camera) == ("grid16", "rolled_pi"), (scene, camera)
    return cameras.camera((0.0, -1.0, 2.5), (0.0, 0.0, 2.5), roll=np.pi)


@functools.lru_cache(maxsize=None)
def oracle(scene="builtin", camera=None):
    """the scene on the CPU oracle, under its own camera or camera_desc()'s"""
    orc = oracle_lib.OracleScene.named(scene)
    if camera is not None:
        cameras.put(camera_desc(scene, camera), orc=orc)
    return orc


@functools.lru_cache(maxsize=None)
def frame(scene, camera, depth):
    return frozen(oracle(scene, camera).render(W, H, depth))[0]


@functools.lru_cache(maxsize=None)
def pixel_rays(camera=None):
    return frozen(rays_ref.camera_rays(oracle("builtin", camera).cam, W, H))[0]


@functools.lru_cache(maxsize=None)
def records(camera=None):
    """the records of the frame's camera rays (rt_render_gbuffer's, rt_intersect_rays')"""
    return frozen(query_ref.intersect(query_ref.Scene(oracle("builtin", camera)), pixel_rays(camera)))[0]


def _lens(k):
    return (lens_ref.oracle_frame("builtin", W, H, LENS["depth"], LENS["samples"], LENS["calls"][k]["seed"],
                                  LENS["calls"][k]["aperture"], FOCUS),)


def _indirect(k, emitters):
    call = INDIRECT["calls"][k]
    return (indirect_ref.indirect(oracle(), records(), INDIRECT["samples"], INDIRECT["gather_depth"], 1.0, call["seed"],
                                  call["key0"], emitters),)


def _adaptive(k):
    camera, depth, n = (None, OTHER_CAMERA)[k], ADAPTIVE["depth"], ADAPTIVE["samples"]
    plain = frame("builtin", camera, depth)
    flags = adaptive_ref.flags(plain, records(camera))
    ssaa = box_filter(oracle("builtin", camera).render(n * W, n * H, depth), n)
    return adaptive_ref.expected_frame(flags, ssaa, plain), flags.astype(np.uint8)


def _mirror(k):
    call = MIRROR["calls"][k]
    return mirror_scenes.reference(MIRROR["key"], W, H, BOUNCES, call["min_reflective"], call["camera"])[:4]


def _glass(k):
    call = GLASS["calls"][k]
    return glass_scenes.reference(GLASS["key"], W, H, BOUNCES, GLASS["min_reflective"], call["min_transmissive"], call["camera"])[:4]


def _crossed(k):
    """rt_mirror_records of the glass room's pixel rays, then rt_glass_records of its second camera's, on the glass room's handle"""
    if k == 1:
        return glass_scenes.reference(CROSSED["key"], W, H, BOUNCES, CROSSED["min_reflective"], CROSSED["min_transmissive"],
                                      CROSSED["cameras"][1])[:4]
    scene = query_ref.Scene(glass_scenes.oracle_scene(CROSSED["key"])[0])
    rays = glass_scenes.pixel_rays(CROSSED["key"], W, H, CROSSED["cameras"][0])
    return mirror_ref.records(scene, rays, BOUNCES, CROSSED["min_reflective"])[:4]


def _ao(k):
    call = AO["calls"][k]
    return (ao_ref.ambient_occlusion(query_ref.Scene(oracle()), records(), AO["samples"], call["radius"], call["seed"], call["key0"]),)


# case -> (what call 1 must write, what call 2 must write), each a function of nothing -> a tuple of arrays
PAIRS = {
    "lens": (lambda: _lens(0), lambda: _lens(1)),
    "indirect-emitters0": (lambda: _indirect(0, False), lambda: _indirect(1, False)),
    "indirect-emitters1": (lambda: _indirect(0, True), lambda: _indirect(1, True)),
    "adaptive": (lambda: _adaptive(0), lambda: _adaptive(1)),
    "mirror": (lambda: _mirror(0), lambda: _mirror(1)),
    "glass": (lambda: _glass(0), lambda: _glass(1)),
    "crossed": (lambda: _crossed(0), lambda: _crossed(1)),
    "stack": (lambda: (frame("builtin", None, STACK_DEPTH),), lambda: (frame("builtin", OTHER_CAMERA, STACK_DEPTH),)),
    "gbuffer": (lambda: (frame("builtin", None, DEPTH), records(None)),
                lambda: (frame("builtin", OTHER_CAMERA, DEPTH), records(OTHER_CAMERA))),
    "rays-queries": (lambda: (rays_ref.oracle_trace(oracle(), pixel_rays(), DEPTH),), lambda: (records(None),)),
    "ao": (lambda: _ao(0), lambda: _ao(1)),
    "repack": (lambda: (frame("builtin", None, DEPTH),), lambda: (frame("builtin", None, DEPTH),)),
}
# the pairs whose two calls write the same kind of output with other parameters: their references must differ (the others are
# rays-queries, colours against records, which nothing could confuse, and repack, one frame twice on purpose)
DIFFERING = tuple(c for c in PAIRS if c not in ("rays-queries", "repack"))


@functools.lru_cache(maxsize=None)
def reference(case, k):
    return frozen(*PAIRS[case][k]())


@functools.lru_cache(maxsize=None)
def two_handles_reference(i):
    scene, camera, depth = TWO_HANDLES[i]
    return frame(scene, camera, depth)


def words(a):
    """an output (W, H, ...) or (W, H) of 4-byte items, records or bytes -> unsigned (W * H, words of a cell)"""
    a = np.ascontiguousarray(a)
    flat = a.reshape(W * H, -1)
    return flat.view(np.uint8 if a.dtype.itemsize == 1 else np.uint32).reshape(W * H, -1)


def differing_share(one, two):
    """the share of the W * H cells in which some output of `one` differs from the same output of `two` in some bit"""
    differ = np.zeros(W * H, dtype=bool)
    for a, b in zip(one, two):
        differ |= (words(a) != words(b)).any(axis=1)
    return float(differ.mean())


def equal_words(got, other):
    """how many words of the outputs `got` equal the same word of `other` (a call's outputs against the OTHER call's reference)"""
    return int(sum((words(a) == words(b)).sum() for a, b in zip(got, other) if np.shape(a) == np.shape(b)))
