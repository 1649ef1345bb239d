"""Every render kernel of the catalogue, launched and compared bit for bit with its reference (kernel_matrix.py: one case per
table mode and family).  The built-in scene carries the FAST and item-table modes; a clustered field of 120 spheres carries the
clustered modes and, with its tables in global memory, _large.  The shadings: Desc.checker_images() plus one random image on a
plane; glass (three spheres, one of them a mirror too, iors 0.7 to 2.4, members of the clustered run in the field, and a clear pane
before the eye); both lights area lights; glass and area lights with a seed.  References: soft_ref (with neither glass nor area
lights it is refract_ref's frame, and so the oracle's), query_ref and texture_ref for the records and verdicts.  Frames are 37 x
29, not a tile multiple, at depth 3; the _refract cases also at depth 8 with the bounce stack in HBM.  Last, the clustered
scheduling paths -- HELP forced and timed out, HEAVY forced, a narrow strip, the stack in HBM -- on the newer families."""
import ctypes as C
import functools

import numpy as np
import pytest

import kernel_matrix as km
import oracle_lib as oracle
import query_ref
import scene_gen
import soft_ref
import texture_ref
from rays_ref import camera_rays
from test_query_gpu import assert_hits_same, assert_verdicts_same
from test_refract_gpu import glass_builtin, make as make_refractive
from test_soft_gpu import make as make_soft
from test_texture_gpu import Desc, assert_same_bits
from tilecoderaytracer_amd import HostScene, capi

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 37, 29
STRIP = (5, 23)
FIELD_SEED = 7
AREA = {"builtin": (2, 0.6), "field": (2, 1.5)}                      # (samples, radius) of both lights; their own radius is 0.15
GLASS = {"builtin": [(4, 0.9, 1.5), (2, 0.5, 0.7), (5, 0.6, 2.4)],   # sphere 2 is a mirror already
         "field": [(35, 0.9, 1.5), (40, 0.7, 0.7), (27, 0.5, 2.4)]}   # the three spheres the field's camera sees most of
IMAGE_PLANE = {"builtin": (7, texture_ref.CLAMP), "field": (123, texture_ref.REPEAT)}    # the floor; the field's upper plane


def kernel(r):
    """the whole name of the kernel of r's last launch (include/rt_capi_launch.h); rt_launch_info's is its first 47 characters"""
    name = r.kernel_name()
    assert r.launch_info().kernel.decode() == name[:47], (r.launch_info().kernel, name)
    return name


def field(scene):
    """the clustered field (scene_gen.build_sphere_field, 120 spheres) with sphere 40 a mirror as well"""
    scene_gen.build_sphere_field(scene, FIELD_SEED)
    scene.set_reflective(40, 0.3)
    return scene


def field_pane(scene):
    pane = scene.add_finite_plane_axes((-0.9, 1.0, 1.75), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), 0.5, 0.9)
    scene.set_color(pane, (0.2, 0.3, 0.9))
    scene.set_diffuse(pane, 0.3)
    return [(pane, 0.8, 1.0)]


def build(name, shading, host):
    """the scene `name` with the shading's glass on a HostScene (host) or an OracleScene -> (scene, glass)"""
    if name == "builtin":
        scene = HostScene.builtin() if host else oracle.OracleScene.builtin()
    else:
        scene = field(HostScene.empty() if host else oracle.OracleScene())
    glass = []
    if "_refract" in shading:
        pane = glass_builtin(scene)[-1:] if name == "builtin" else field_pane(scene)
        glass = GLASS[name] + pane
    return scene, glass


class World:
    """one scene with one shading: the description the renderers are made from and the references' scene"""

    def __init__(self, name, shading, builder=None, area=None):
        """builder(scene) -> the scene it has built on a fresh HostScene / OracleScene, in place of the scene `name` (without
        glass or images); area: (samples, radius) of the area lights -- every light of a builder's scene -- in place of AREA[name]"""
        self.name, self.shading = name, shading
        if builder is None:
            host, self.glass = build(name, shading, True)
            self.orc, _ = build(name, shading, False)
            lights = (0, 1)
        else:
            host, self.glass = builder(HostScene.empty()), []
            self.orc = builder(oracle.OracleScene())
            lights = [k for k in range(self.orc.object_count) if self.orc.get_object(k).is_light]
        n, r = area or AREA[name]
        self.area = [(k, n, r) for k in lights] if "_soft" in shading else []
        self.seed = 5 if shading == "_refract_soft" else 0
        self.desc = Desc(host)
        self.images, self.image_of = None, {}
        if shading == "_image":
            self.images = self.desc.checker_images()
            plane, wrap = IMAGE_PLANE[name]
            image = (np.random.RandomState(5).rand(7, 9, 3).astype(F), F(0.9), F(0.7), wrap)
            self.images.append(image)
            self.desc.objs[plane].texture = self.desc.n_textures + len(self.images) - 1
            self.image_of = {plane: image}
        self.ref = soft_ref.Scene(self.orc, {k: (n, r) for k, n, r in self.area}, self.seed,
                                  {k: (tf, ior) for k, tf, ior in self.glass}, self.image_of)
        self.query = query_ref.Scene(self.orc)

    def renderer(self, options):
        if self.area:
            return make_soft(self.desc, self.area, refractive=self.glass or None, images=self.images, options=options,
                             seed=self.seed)
        if self.glass:
            return make_refractive(self.desc, refractive=self.glass, images=self.images, options=options)
        return self.desc.make(images=self.images, options=options)

    def records(self, rays):
        """query_ref's records of rays, the image planes' colours their texels"""
        hits, colours = texture_ref.colours(self.query, rays, self.image_of)
        hits = hits.reshape(-1).copy()
        hits["color"] = colours
        return hits.reshape(rays.shape[:-1])


@functools.lru_cache(maxsize=None)
def world(name, shading):
    return World(name, shading)


@functools.lru_cache(maxsize=None)
def frame(name, shading, depth):
    w = world(name, shading)
    return soft_ref.render(w.ref, w.desc.cam, W, H, depth)


@functools.lru_cache(maxsize=None)
def ssaa_frame(name, shading, depth):
    w = world(name, shading)
    return soft_ref.render_ssaa(w.ref, w.desc.cam, W, H, depth, 2)


@functools.lru_cache(maxsize=None)
def ray_batch(name, shading):
    """the camera's rays in a shuffled order, rays that start inside the glass spheres (opaque ones in the scenes without glass)
    and rays that start on the pane, both ways -> (rays, soft_ref's colours at depth km.DEPTH, the records)"""
    w = world(name, shading)
    rng = np.random.RandomState(11)
    cam = camera_rays(w.desc.cam, W, H).reshape(-1, 6)
    parts = [cam[rng.permutation(len(cam))]]
    for k, _, _ in GLASS[name]:
        o = w.orc.get_object(k)
        c, r = np.array(o.origin.tuple(), dtype=F), F(o.radius)
        E = (c + rng.uniform(-0.5, 0.5, (24, 3)) * r).astype(F)
        parts.append(np.concatenate([E, E + rng.normal(size=(24, 3)).astype(F)], axis=1))
    if w.glass:
        o = w.orc.get_object(w.glass[-1][0])
        po, hz, vt = (np.array(v.tuple(), dtype=F) for v in (o.plane_origin, o.horizontal, o.vertical))
        u, v = rng.uniform(0, 1, (2, 32, 1)).astype(F)
        E = (po + hz * (u * F(o.h_distance)) + vt * (v * F(o.v_distance))).astype(F)
        ahead = np.where(rng.rand(32, 1) < 0.5, F(1), F(-1)) * np.array([0, 1, 0], dtype=F)
        T = E + ahead + rng.uniform(-0.3, 0.3, (32, 3)).astype(F)
        parts.append(np.concatenate([E, T], axis=1))
    rays = np.ascontiguousarray(np.concatenate(parts).astype(F))
    return rays, soft_ref.trace(w.ref, rays, km.DEPTH), w.records(rays)


@functools.lru_cache(maxsize=None)
def segments(name, shading):
    """segments from the camera rays' hit points to the lights' centres and to points of their discs, and from points inside
    the glass spheres -> (segments, query_ref's verdicts)"""
    w = world(name, shading)
    rng = np.random.RandomState(13)
    hits = query_ref.intersect(w.query, camera_rays(w.desc.cam, W, H).reshape(-1, 6))
    P = hits["point"][hits["object"] >= 0]
    n, r = AREA[name]
    parts = []
    for k in (0, 1):
        L = np.array(w.orc.get_object(k).origin.tuple(), dtype=F)
        parts.append(np.concatenate([P, np.broadcast_to(L, P.shape)], axis=1))
        parts.append(np.concatenate([P, (L + rng.uniform(-r, r, P.shape)).astype(F)], axis=1))
        for g, _, _ in GLASS[name]:
            o = w.orc.get_object(g)
            E = np.array(o.origin.tuple(), dtype=F) + rng.uniform(-0.5, 0.5, (16, 3)).astype(F) * F(o.radius)
            parts.append(np.concatenate([E, np.broadcast_to(L, E.shape)], axis=1))
    segs = np.ascontiguousarray(np.concatenate(parts).astype(F))
    return segs, query_ref.occluded(w.query, segs)


@functools.lru_cache(maxsize=None)
def camera_records(name, shading):
    w = world(name, shading)
    return w.records(camera_rays(w.desc.cam, W, H))


# ---- the matrix -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", km.CASES, ids=km.case_id)
def test_every_render_kernel_equals_its_reference(case):
    w = world(case.scene, case.shading)
    r = w.renderer(case.options)
    name, depth, what = km.kernel_name(case), km.DEPTH, km.case_id(case)
    try:
        if case.call == "render":
            want = frame(case.scene, case.shading, depth)
            assert_same_bits(r.render(W, H, depth), want, f"{what}: render")
            assert kernel(r) == name, (kernel(r), name)
            x0, x1 = STRIP
            assert_same_bits(r.render(W, H, depth, x0, x1), want[x0:x1], f"{what}: strip {x0}:{x1}")
        elif case.call == "ssaa":
            assert_same_bits(r.render_ssaa(W, H, depth, 2), ssaa_frame(case.scene, case.shading, depth), f"{what}: ssaa")
        elif case.call == "rays":
            rays, want, _ = ray_batch(case.scene, case.shading)
            assert_same_bits(r.trace_rays(rays, depth), want, f"{what}: trace_rays")
        elif case.call == "hits":
            rays, _, want = ray_batch(case.scene, case.shading)
            assert_hits_same(r.intersect_rays(rays), want, f"{what}: intersect_rays")
        elif case.call == "occluded":
            segs, want = segments(case.scene, case.shading)
            assert_verdicts_same(r.occluded_rays(segs), want, f"{what}: occluded_rays")
        else:
            rgb, hits = r.render_gbuffer(W, H, depth)
            assert_same_bits(rgb, frame(case.scene, case.shading, depth), f"{what}: gbuffer colours")
            assert_hits_same(hits, camera_records(case.scene, case.shading), f"{what}: gbuffer records")
        assert kernel(r) == name, (kernel(r), name)
        if case.deep:
            r.set_option("stack", 2)
            assert_same_bits(r.render(W, H, km.DEEP), frame(case.scene, case.shading, km.DEEP), f"{what}: depth {km.DEEP}, stack 2")
            assert kernel(r) == name, (kernel(r), name)
    finally:
        r.close()


# ---- the clustered scheduling paths with the newer families -----------------------------------------------------------------

SCHEDULED = [c for c in km.CASES if (c.mode, c.family) in
             {("_clusters", "_refract"), ("_clusters_wide", "_refract_soft"), ("_clusters", "_ssaa_image"),
              ("_clusters", "_gbuffer_refract_soft")}]
CONFIGS = {
    "help": ({"help": 2, "block_threads": 256}, km.DEPTH, None),
    "help_timed_out": ({"help": 2, "block_threads": 256, "help_spin_limit": -1}, km.DEPTH, None),
    "heavy": ({"heavy": 2}, km.DEPTH, None),
    "strip": ({}, km.DEPTH, (12, 24)),                       # a third of the width: HELP, HEAVY, tile priorities on their own
    "stack_hbm": ({"stack": 2}, km.DEEP, None),
}


def raw_call(r, call, depth, x0, x1):
    """the C call itself -> (rc, colours, records or None)"""
    lib = capi.load_library()
    rgb = np.zeros((x1 - x0, H, 3), dtype=F)
    if call == "render":
        return lib.rt_render(r._scene, r._cam, W, H, x0, x1, depth, rgb.ctypes.data), rgb, None
    if call == "ssaa":
        return lib.rt_render_ssaa(r._scene, r._cam, W, H, x0, x1, depth, 2, rgb.ctypes.data), rgb, None
    from tilecoderaytracer_amd.renderer import HIT_DTYPE
    hits = np.zeros((x1 - x0, H), dtype=HIT_DTYPE)
    return lib.rt_render_gbuffer(r._scene, r._cam, W, H, x0, x1, depth, rgb.ctypes.data, hits.ctypes.data), rgb, hits


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("case", SCHEDULED, ids=km.case_id)
def test_clustered_scheduling_paths(case, config):
    options, depth, strip = CONFIGS[config]
    w = world(case.scene, case.shading)
    r = w.renderer({**case.options, **options})
    x0, x1 = strip or (0, W)
    want = (ssaa_frame if case.call == "ssaa" else frame)(case.scene, case.shading, depth)[x0:x1]
    what = f"{km.case_id(case)} {config}"
    try:
        rc, rgb, hits = raw_call(r, case.call, depth, x0, x1)
        if config == "help_timed_out":
            assert rc in (capi.RT_OK, capi.RT_ERR_HIP), rc
        else:
            assert rc == capi.RT_OK, (rc, capi.load_library().rt_last_error())
        assert_same_bits(rgb, want, what)
        if hits is not None:
            assert_hits_same(hits, camera_records(case.scene, case.shading)[x0:x1], f"{what}: records")
        if config == "help_timed_out":
            r.set_option("help_spin_limit", 1 << 22)
            rc, rgb, _ = raw_call(r, case.call, depth, x0, x1)
            assert rc == capi.RT_OK
            assert_same_bits(rgb, want, f"{what}: usable afterwards")
        assert kernel(r) == km.kernel_name(case), (kernel(r), km.kernel_name(case))
    finally:
        r.close()


# ---- the whole name ---------------------------------------------------------------------------------------------------------

def test_the_longest_name_whole_and_the_buffer_checks():
    """rt_get_launch_kernel: "" before the first launch; the 51 characters of the longest name with a buffer of 52 bytes, and
    RT_ERR_INVALID, nothing written, with 51"""
    case = [c for c in km.CASES if (c.mode, c.family) == ("_clusters_wide", "_gbuffer_refract_soft")][0]
    r = world(case.scene, case.shading).renderer(case.options)
    lib = capi.load_library()
    try:
        assert r.kernel_name() == ""
        r.render_gbuffer(W, H, 1)
        name = km.kernel_name(case)
        assert len(name) == 51 and kernel(r) == name
        exact = C.create_string_buffer(len(name) + 1)
        assert lib.rt_get_launch_kernel(r._scene, exact, len(exact)) == capi.RT_OK and exact.value.decode() == name
        short = C.create_string_buffer(b"x" * len(name), len(name))
        assert lib.rt_get_launch_kernel(r._scene, short, len(short)) == capi.RT_ERR_INVALID
        assert short.raw == b"x" * len(name)
        assert lib.rt_get_launch_kernel(r._scene, None, 64) == capi.RT_ERR_INVALID
    finally:
        r.close()
