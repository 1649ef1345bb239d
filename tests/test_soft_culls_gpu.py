"""The culls under glass and area lights, bit for bit against soft_ref: the seeded generators of scene_gen (rooms, far grazing
plates, clustered sphere fields, random scenes) with glass and area lights derived from the seed, each also compared with the
plain in-order scans (option "cull" = 0) so that a failure tells a cull from a shading; and rim blockers -- a small sphere or
rectangle beside an area light, off its centre by 0.7 of its radius across the way to the lit floor -- which shadow the samples
on one side of the disc and not the segment to the centre, so that a cull or a voxel mask that grew the light by its centre
instead of its reach r'  changes pixels."""
import functools

import numpy as np
import pytest

import oracle_lib as oracle
import scene_gen
import soft_ref
from test_soft_gpu import make
from test_texture_gpu import Desc, assert_same_bits, kernel
from tilecoderaytracer_amd import HostScene

pytestmark = pytest.mark.gpu
F = np.float32
W, H, DEPTH = 40, 31, 3

# ---- 1. seeded scenes --------------------------------------------------------------------------------------------------------

GENERATORS = {"room": scene_gen.build_room, "far": scene_gen.build_far_grazing,
              "field": lambda s, seed: scene_gen.build_sphere_field(s, seed, n_spheres=90),
              "random": scene_gen.build_random}
SEEDS = {"room": [201, 202, 203, 206, 210, 211], "far": [1, 2, 3, 4, 5, 6], "field": [1, 2, 3, 4, 5, 6],
         "random": [3, 17, 29, 41, 53, 67]}


def dressing(orc, gen, seed):
    """glass and area lights from the seed: two or three spheres and up to two planes (at least one where there is no sphere) refractive (tf 0.5 or 0.9, ior from
    0.7 to 2.4); every light an area light with 1 to 3 samples a side and 0.5 to 10 times its own radius -- 1.5 to 10 in the
    rooms, whose lights hug walls up to 0.1 of the scale away, so that their discs cross the wall -> (glass, area)"""
    rng = np.random.RandomState(seed * 7 + 3)
    objs = [orc.get_object(i) for i in range(orc.object_count)]
    spheres = [i for i, o in enumerate(objs) if o.kind == 0 and not o.is_light]
    planes = [i for i, o in enumerate(objs) if o.kind != 0]
    picks = list(rng.choice(spheres, min(len(spheres), int(rng.randint(2, 4))), replace=False)) if spheres else []
    picks += list(rng.choice(planes, min(len(planes), int(rng.randint(0 if picks else 1, 3))), replace=False)) if planes else []
    glass = [(int(k), float(rng.choice([0.5, 0.9])), float(rng.choice([0.7, 1.0, 1.33, 1.5, 2.4]))) for k in picks]
    lo = 1.5 if gen == "room" else 0.5
    area = [(i, int(rng.randint(1, 4)), float(F(objs[i].radius * rng.uniform(lo, 10.0)))) for i, o in enumerate(objs) if o.is_light]
    return glass, area


@functools.lru_cache(maxsize=None)
def seeded(gen, seed, with_glass):
    orc = GENERATORS[gen](oracle.OracleScene(), seed)
    glass, area = dressing(orc, gen, seed)
    glass = glass if with_glass else []
    rs = soft_ref.Scene(orc, {k: (n, r) for k, n, r in area}, seed, {k: (tf, ior) for k, tf, ior in glass})
    host = GENERATORS[gen](HostScene.empty(), seed)
    return host, glass, area, soft_ref.render(rs, Desc(host).cam, W, H, DEPTH)


@pytest.mark.parametrize("with_glass", [False, True], ids=["area lights", "area lights and glass"])
@pytest.mark.parametrize("gen, seed", [(g, s) for g in GENERATORS for s in SEEDS[g]])
def test_seeded_scenes_with_glass_and_area_lights(gen, seed, with_glass):
    host, glass, area, want = seeded(gen, seed, with_glass)
    d = Desc(host)
    variants = [{}, {"cull": 0}] + ([{"svox": 0}, {"svox": 800}] if gen == "field" else [])
    for options in variants:
        r = make(d, area, refractive=glass or None, options=options, seed=seed)
        try:
            assert_same_bits(r.render(W, H, DEPTH), want, f"{gen} {seed} {options}")
            assert kernel(r).endswith("_refract_soft" if glass else "_soft"), kernel(r)
        finally:
            r.close()


# ---- 2. rim blockers ---------------------------------------------------------------------------------------------------------

LIGHTS = [((9.0, 8.0, 5.0), 1.0), ((-4.0, 12.0, 10.0), 0.8)]       # centre, area radius; both out of the camera's view
LIT = np.array([0.0, 8.0, 0.0])                                       # the middle of the floor the camera sees


def rim_point(light, offset=0.7):
    """a point beside the light's disc, `offset` radii off its centre across the way D to the lit floor -- upwards, so that it
    lies above every segment from the floor to the centre and outside every box around them -> (the point, D, the offset's
    direction)"""
    C, R = np.array(light[0]), light[1]
    D = (C - LIT) / np.linalg.norm(C - LIT)
    u = np.array([0.0, 0.0, 1.0]) - D * D[2]
    u /= np.linalg.norm(u)
    return C + u * (offset * R), D, u


def rim_scene(scene, blocker, clustered):
    """two lights, a floor, a few spheres; blocker None, "sphere" or "rectangle" beside light 0; clustered: the spheres are a run
    of 70 and, in its middle, the blocker sphere with a tight group of 31 small ones beside it"""
    for (c, _), k in zip(LIGHTS, range(2)):
        i = scene.add_sphere(c, 0.15)
        scene.set_light(i)
        scene.set_intensity(i, 0.9 - 0.2 * k)
    floor = scene.add_infinite_plane((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    scene.set_color(floor, (0.9, 0.9, 0.9))
    rng = np.random.RandomState(4)
    B, D, u = rim_point(LIGHTS[0])
    R = LIGHTS[0][1]
    n_run = 70 if clustered else 5
    for k in range(n_run):
        if clustered and k == n_run // 2:
            if blocker == "sphere":
                scene.add_sphere(tuple(float(F(v)) for v in B), 0.25 * R)
            for j in range(31):                               # a tight group beside it, so that its cluster leaves hold no other
                p = B + u * (0.12 * R) + rng.uniform(-0.05, 0.05, 3) * R
                scene.add_sphere(tuple(float(F(v)) for v in p), 0.03 * R)
        i = scene.add_sphere((float(F(rng.uniform(-4, 4))), float(F(rng.uniform(12, 30))), float(F(rng.uniform(0.3, 1.0)))),
                             float(F(rng.uniform(0.2, 0.6))))
        scene.set_color(i, scene_gen.PALETTE[k % len(scene_gen.PALETTE)])
    if blocker == "sphere" and not clustered:
        scene.add_sphere(tuple(float(F(v)) for v in B), 0.25 * R)
    if blocker == "rectangle":                               # 0.4 x 0.4 radii, facing the floor, centred on the point
        corner = B - u * (0.2 * R) - np.cross(D, u) * (0.2 * R)
        scene.add_finite_plane_axes(tuple(float(F(v)) for v in corner), tuple(float(F(v)) for v in D),
                                    tuple(float(F(v)) for v in u), 0.4 * R, 0.4 * R)
    scene.set_object_indices(0, 1)
    scene.camera_two_mirrors()
    return scene


AREA = [(0, 3, LIGHTS[0][1]), (1, 2, LIGHTS[1][1])]


@functools.lru_cache(maxsize=None)
def rim_want(blocker, clustered):
    orc = rim_scene(oracle.OracleScene(), blocker, clustered)
    rs = soft_ref.Scene(orc, {k: (n, r) for k, n, r in AREA})
    return soft_ref.render(rs, orc.cam, W, H, 1), orc.render(W, H, 1)


RIM_MODES = {False: [{}, {"fast": 0}, {"tables": 2}],
             True: [{"wide": 0, "svox": 800}, {"wide": 1, "svox": 800}, {"wide": 0, "svox": 4096}, {"tables": 2}]}


@pytest.mark.parametrize("clustered", [False, True], ids=["fast scene", "clustered run"])
@pytest.mark.parametrize("blocker", ["sphere", "rectangle"])
def test_rim_blockers(blocker, clustered):
    want, hard = rim_want(blocker, clustered)
    want_open, hard_open = rim_want(None, clustered)
    assert_same_bits(hard, hard_open, "the blocker shadows no segment to a light's centre, and no camera ray sees it")
    assert (want != want_open).any(axis=-1).sum() >= 10, "the blocker shadows samples at the rim"
    host = rim_scene(HostScene.empty(), blocker, clustered)
    names = set()
    for options in RIM_MODES[clustered]:
        r = make(Desc(host), AREA, options=options)
        try:
            assert_same_bits(r.render(W, H, 1), want, f"{blocker} {options}")
            names.add(kernel(r))
        finally:
            r.close()
    if clustered:
        assert {"rt_render_kernel_clusters_soft", "rt_render_kernel_clusters_wide_soft", "rt_render_kernel_large_soft"} <= names, names
    else:
        assert names == {"rt_render_kernel_soft", "rt_render_kernel_items_soft", "rt_render_kernel_large_soft"}, names
