"""Image textures (include/rt_capi_texture.h) on the GPU, every comparison bit-exact: the 2 x 2 CHECKER image of a
checkerboard and a one-colour image reproduce the checkerboard and the untextured plane through every call; a 1024^2 image's
texels land where texture_ref puts them, in the primary records and through the bounce stack (LDS and HBM levels); the
*_image kernels run exactly when a plane references an image."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as oracle
import query_ref
import scene_gen
import texture_ref
from rays_ref import camera_rays
from test_query_gpu import assert_hits_same
from tilecoderaytracer_amd import HostScene, Renderer, RtError, capi

pytestmark = pytest.mark.gpu
F = np.float32


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)):
        bad = np.argwhere(np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32))
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {tuple(bad[0])}")


class Desc:
    """a HostScene's description and camera, copied so that texture indices can be changed; images: make() passes them"""

    def __init__(self, host):
        d = host.desc.contents
        self.objs = (capi.RtObjectDesc * max(d.n_objects, 1))()
        for i in range(d.n_objects):
            self.objs[i] = d.objects[i]
        self.texs = (capi.RtTextureDesc * max(d.n_textures, 1))()
        for i in range(d.n_textures):
            self.texs[i] = d.textures[i]
        self.n, self.n_textures = d.n_objects, d.n_textures
        self.shadow = (d.shadow_begin, d.shadow_end)
        self.null = tuple(d.null_color)
        self.cam = capi.RtCameraDesc()
        C.memmove(C.byref(self.cam), host.camera, C.sizeof(capi.RtCameraDesc))

    def make(self, images=None, options=None):
        desc = capi.RtSceneDesc(self.n, self.objs, self.n_textures, self.texs, self.shadow[0], self.shadow[1],
                                (C.c_float * 3)(*self.null))
        r = Renderer.from_desc(desc, self.cam, keepalive=(self, desc), images=images)
        for k, v in (options or {}).items():
            r.set_option(k, v)
        return r

    def checker_images(self):
        """every checkerboard referenced as its 2 x 2 CHECKER image instead -> the images"""
        images = []
        for t in range(self.n_textures):
            x = self.texs[t]
            images.append(texture_ref.checker_image(tuple(x.light), tuple(x.dark), x.width, x.height))
        for i in range(self.n):
            if self.objs[i].texture >= 0:
                self.objs[i].texture += self.n_textures
        return images


def kernel(r):
    return r.launch_info().kernel.decode()


def compare_all_calls(plain, textured, W, H, depth, what):
    """rt_render, rt_render_ssaa (k = 2), rt_trace_rays, rt_intersect_rays, rt_render_gbuffer: the same bits on both"""
    want = plain.render(W, H, depth)
    assert_same_bits(textured.render(W, H, depth), want, f"{what}: render")
    assert kernel(textured) == kernel(plain) + "_image", (kernel(textured), kernel(plain))
    assert_same_bits(textured.render_ssaa(W, H, depth, 2), plain.render_ssaa(W, H, depth, 2), f"{what}: ssaa")
    rays = np.ascontiguousarray(camera_rays(plain._cam, W, H))
    assert_same_bits(textured.trace_rays(rays, depth), plain.trace_rays(rays, depth), f"{what}: trace_rays")
    assert_hits_same(textured.intersect_rays(rays), plain.intersect_rays(rays), f"{what}: intersect_rays")
    assert_same_bits(textured.occluded_rays(rays), plain.occluded_rays(rays), f"{what}: occluded_rays")
    rgb_t, hits_t = textured.render_gbuffer(W, H, depth, 3, W - 5)
    rgb_p, hits_p = plain.render_gbuffer(W, H, depth, 3, W - 5)
    assert_same_bits(rgb_t, rgb_p, f"{what}: gbuffer colours")
    assert_hits_same(hits_t, hits_p, f"{what}: gbuffer records")
    return want


# ---- 1. checker identity ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", [{}, {"fast": 0}, {"tables": 2}])
def test_builtin_checker_as_image_is_the_checkerboard_and_the_oracle(options):
    host = HostScene.builtin()
    base = Desc(host)
    plain = base.make(options=options)
    img = Desc(host)
    textured = img.make(images=img.checker_images(), options=options)
    W, H, depth = 256, 192, 4
    got = compare_all_calls(plain, textured, W, H, depth, f"builtin {options}")
    if not options:
        want = oracle.OracleScene.builtin().render(W, H, depth)
        assert_same_bits(got, want, "builtin: oracle")


@pytest.mark.parametrize("seed", [3, 17, 29, 41])
def test_fuzzed_checker_scenes_as_images(seed):
    host = HostScene.empty()
    scene_gen.build_random(host, seed)
    img = Desc(host)
    images = img.checker_images()
    if not any(img.objs[i].texture >= 0 and img.objs[i].kind != capi.RT_KIND_SPHERE for i in range(img.n)):
        pytest.skip("no textured plane in this scene")
    compare_all_calls(Desc(host).make(), img.make(images=images), 96, 80, 4, f"seed {seed}")


def reflective_checker_planes(scene):
    i = scene.add_sphere((2.0, 8.0, 9.0), 0.15)
    scene.set_light(i)
    i = scene.add_infinite_plane((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    scene.set_checkerboard(i, (1, 1, 0), (0, 0, 1), 1.5, 2.5)
    scene.set_reflective(i, 0.6)
    i = scene.add_finite_plane_axes((-6.0, 18.0, 0.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 8.0, 12.0)
    scene.set_checkerboard(i, (1, 1, 1), (1, 0, 0), 0.75, 0.5)
    scene.set_reflective(i, 0.5)
    for k in range(3):
        i = scene.add_sphere((-2.0 + 2.0 * k, 9.0, 1.0), 0.8)
        scene.set_color(i, scene_gen.PALETTE[k])
        scene.set_reflective(i, 0.3)
    scene.set_object_indices(0, 1)
    scene.camera_two_mirrors()
    return scene


def test_reflective_checker_planes_depth_4_equal_the_oracle():
    host = reflective_checker_planes(HostScene.empty())
    img = Desc(host)
    textured = img.make(images=img.checker_images())
    W, H = 160, 120
    want = reflective_checker_planes(oracle.OracleScene()).render(W, H, 4)
    assert_same_bits(textured.render(W, H, 4), want, "reflective checker planes: oracle")
    assert_same_bits(Desc(host).make().render(W, H, 4), want, "reflective checker planes: plain")


# ---- 2. uniform identity ----------------------------------------------------------------------------------------------------

def test_one_colour_image_is_the_untextured_plane():
    c = (0.25, 0.75, 0.5)

    def build(scene, coloured):
        i = scene.add_sphere((2.0, 8.0, 9.0), 0.15)
        scene.set_light(i)
        i = scene.add_infinite_plane((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
        scene.set_reflective(i, 0.5)
        if coloured:
            scene.set_color(i, c)
        i = scene.add_sphere((0.0, 8.0, 1.0), 1.0)
        scene.set_color(i, (1, 0, 0))
        scene.set_reflective(i, 0.4)
        scene.set_object_indices(0, 1)
        scene.camera_two_mirrors()
        return scene

    host = build(HostScene.empty(), False)
    img = Desc(host)
    img.objs[1].texture = 0                                  # no checkerboards: image 0
    texels = np.broadcast_to(np.array(c, dtype=F), (5, 3, 3)).copy()
    W, H, depth = 128, 96, 4
    for wrap in (texture_ref.CHECKER, texture_ref.REPEAT, texture_ref.CLAMP):
        textured = img.make(images=[(texels, 0.7, 1.3, wrap)])
        plain = Desc(build(HostScene.empty(), True)).make()
        got = compare_all_calls(plain, textured, W, H, depth, f"uniform wrap {wrap}")
        assert_same_bits(got, build(oracle.OracleScene(), True).render(W, H, depth), "uniform: oracle")


# ---- 3. texel lookup in the primary record ----------------------------------------------------------------------------------

def image_planes(scene, floor_colour=(1, 1, 1), floor_reflective=0.0):
    i = scene.add_sphere((3.0, 6.0, 9.0), 0.15)
    scene.set_light(i)
    floor = scene.add_infinite_plane((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    scene.set_color(floor, floor_colour)
    scene.set_reflective(floor, floor_reflective)
    wall = scene.add_finite_plane_axes((-7.0, 22.0, -0.5), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 9.0, 13.0)
    for k in range(4):
        i = scene.add_sphere((-3.0 + 2.0 * k, 7.0 + k, 1.2), 0.7)
        scene.set_color(i, scene_gen.PALETTE[k])
    scene.set_object_indices(0, 1)
    scene.camera_two_mirrors()
    return scene, floor, wall


@pytest.mark.parametrize("wrap", [texture_ref.CHECKER, texture_ref.REPEAT, texture_ref.CLAMP])
def test_random_1024_image_records_equal_texture_ref(wrap):
    host, floor, wall = image_planes(HostScene.empty())
    orc, _, _ = image_planes(oracle.OracleScene())
    rng = np.random.RandomState(wrap + 7)
    texels = rng.uniform(0, 1, (1024, 1024, 3)).astype(F)
    image = (texels, F(5.0), F(3.5), wrap)
    img = Desc(host)
    img.objs[floor].texture = 0
    img.objs[wall].texture = 0
    r = img.make(images=[image])
    W, H = 160, 120
    rays = np.ascontiguousarray(camera_rays(img.cam, W, H))
    want_hits, want_colour = texture_ref.colours(query_ref.Scene(orc), rays.reshape(-1, 6), {floor: image, wall: image})
    on_image = np.isin(want_hits["object"], [floor, wall])
    assert on_image.mean() > 0.3
    _, hits = r.render_gbuffer(W, H, 2)
    assert kernel(r) == "rt_render_kernel_gbuffer_image"
    q = r.intersect_rays(rays)
    for what, got in (("gbuffer", hits), ("intersect_rays", q)):
        got = got.reshape(-1)
        np.testing.assert_array_equal(got["object"], want_hits["object"], err_msg=what)
        assert_same_bits(got["color"], want_colour, f"{what}: texel colours")


# ---- 4. the texel through the bounce stack ----------------------------------------------------------------------------------

@pytest.mark.parametrize("stack, depth, strip", [(1, 4, None), (2, 4, None), (0, 2, (37, 101)), (0, 4, (0, 64))])
def test_two_colour_texels_through_the_bounce_stack(stack, depth, strip):
    a, b = (0.9, 0.3, 0.1), (0.1, 0.5, 0.9)
    host, floor, wall = image_planes(HostScene.empty(), floor_reflective=0.5)
    rng = np.random.RandomState(99)
    mask = rng.randint(0, 2, (1024, 1024)).astype(bool)     # > 65 536 texels: a 16-bit selector would lose the texel
    texels = np.where(mask[..., None], np.array(b, dtype=F), np.array(a, dtype=F)).astype(F)
    image = (texels, F(6.0), F(6.0), texture_ref.REPEAT)
    img = Desc(host)
    img.objs[floor].texture = 0
    r = img.make(images=[image], options={"stack": stack} if stack else None)
    W, H = 160, 128
    x0, x1 = strip if strip else (0, W)
    got = r.render(W, H, depth, x0, x1)
    assert kernel(r) == "rt_render_kernel_image"
    want_a = image_planes(oracle.OracleScene(), floor_colour=a, floor_reflective=0.5)[0].render(W, H, depth, x0, x1)
    want_b = image_planes(oracle.OracleScene(), floor_colour=b, floor_reflective=0.5)[0].render(W, H, depth, x0, x1)
    gu, au, bu = (v.view(np.uint32).reshape(-1, 3) for v in (got, want_a, want_b))
    is_a, is_b = (gu == au).all(axis=1), (gu == bu).all(axis=1)
    assert (is_a | is_b).all(), f"{int((~(is_a | is_b)).sum())} pixels are neither frame"
    orc = image_planes(oracle.OracleScene(), floor_reflective=0.5)[0]
    rays = np.ascontiguousarray(camera_rays(img.cam, W, H)[x0:x1]).reshape(-1, 6)
    hits = query_ref.intersect(query_ref.Scene(orc), rays)
    x, y = texture_ref.plane_coords(query_ref.Scene(orc), rays, hits)
    on_floor = hits["object"] == floor
    assert on_floor.mean() > 0.2
    names_b = mask.reshape(-1)[texture_ref.texel(x[on_floor], y[on_floor], image)]
    differ = ~((au == bu).all(axis=1))[on_floor]                   # where the floor's colour shows at all
    assert differ.sum() > 100
    np.testing.assert_array_equal(is_b[on_floor][differ], names_b[differ])
    np.testing.assert_array_equal(is_a[on_floor][differ], ~names_b[differ])


# ---- 5. kernel choice -------------------------------------------------------------------------------------------------------

def test_no_images_is_rt_scene_create():
    host = HostScene.builtin()
    want = Renderer(host).render(200, 150, 4)
    r = Desc(host).make(images=[])
    assert_same_bits(r.render(200, 150, 4), want, "textured create with no images")
    assert kernel(r) == "rt_render_kernel"


def test_unused_or_sphere_only_images_keep_the_plain_kernels():
    host = HostScene.builtin()
    d = Desc(host)
    sphere = [i for i in range(d.n) if d.objs[i].kind == capi.RT_KIND_SPHERE and not d.objs[i].is_light][0]
    d.objs[sphere].texture = d.n_textures                       # a sphere's texture is never sampled
    texels = np.zeros((4, 4, 3), dtype=F)
    r = d.make(images=[(texels, 1.0, 1.0, texture_ref.REPEAT)])
    assert_same_bits(r.render(200, 150, 4), Renderer(host).render(200, 150, 4), "sphere with an image")
    assert kernel(r) == "rt_render_kernel"


def test_counting_build_refuses_image_scenes():
    img = Desc(HostScene.builtin())
    r = img.make(images=img.checker_images())
    with pytest.raises(RtError) as e:
        r.render_stats(64, 64, 2)
    assert e.value.code == capi.RT_ERR_INVALID
    with pytest.raises(RtError) as e:
        r.learn_tile_order(64, 64, 2)
    assert e.value.code == capi.RT_ERR_INVALID


# ---- 6. errors --------------------------------------------------------------------------------------------------------------

def test_capacity_limit_and_a_full_scene():
    host, floor, wall = image_planes(HostScene.empty())
    d = Desc(host)
    d.objs[floor].texture = 0
    d.objs[wall].texture = 1
    full = [(np.zeros((1024, 1023, 3), F), 1.0, 1.0, 0), (np.ones((1, 1024, 3), F), 1.0, 1.0, 1)]   # 2^20 texels exactly
    r = d.make(images=full)
    assert r.render(32, 32, 1).shape == (32, 32, 3)
    over = [(np.zeros((1024, 1023, 3), F), 1.0, 1.0, 0), (np.ones((1, 1025, 3), F), 1.0, 1.0, 1)]
    with pytest.raises(RtError) as e:
        d.make(images=over)
    assert e.value.code == capi.RT_ERR_CAPACITY
    with pytest.raises(RtError) as e:
        d.make(images=[(np.zeros((2, 2, 3), F), 1.0, -1.0, 0)] * 2)
    assert e.value.code == capi.RT_ERR_INVALID


# ---- 7. the host model: a Texture_Image scene -------------------------------------------------------------------------------

def test_host_model_texture_image_is_the_desc_scene():
    """Texture_Image set through the host model (Scene::flatten() emits it, Renderer(HostScene) takes
    rt_scene_create_textured) renders as the same scene made by Renderer.from_desc(images=...)"""
    rng = np.random.RandomState(4)
    texels = rng.uniform(0, 1, (256, 384, 3)).astype(F)
    host, floor, wall = image_planes(HostScene.empty(), floor_reflective=0.5)
    plain = Desc(host)                                       # taken before any texture is set
    host.set_checkerboard(wall, (1, 1, 1), (0, 0, 1), 1.25, 0.75)
    host.set_image_texture(floor, texels, 4.0, 3.0, texture_ref.REPEAT)
    r = Renderer(host)
    plain.texs[0] = capi.RtTextureDesc((1, 1, 1), (0, 0, 1), 1.25, 0.75)
    plain.n_textures = 1
    plain.objs[wall].texture = 0
    plain.objs[floor].texture = 1
    want = plain.make(images=[(texels, 4.0, 3.0, texture_ref.REPEAT)])
    W, H = 160, 120
    for depth in (0, 4):
        assert_same_bits(r.render(W, H, depth), want.render(W, H, depth), f"host model, depth {depth}")
    assert kernel(r) == "rt_render_kernel_image"
    rgb, hits = r.render_gbuffer(W, H, 2)
    rgb_w, hits_w = want.render_gbuffer(W, H, 2)
    assert_same_bits(rgb, rgb_w, "host model: gbuffer colours")
    assert_hits_same(hits, hits_w, "host model: gbuffer records")


@pytest.mark.parametrize("width", [3e38, 1e-38, 7e-45])
def test_extreme_world_sizes_stay_exact(width):
    """a world size near the top of the float range or in the subnormals: the records still name texture_ref's texel"""
    host, floor, wall = image_planes(HostScene.empty())
    orc, _, _ = image_planes(oracle.OracleScene())
    texels = np.random.RandomState(2).uniform(0, 1, (64, 1024, 3)).astype(F)
    image = (texels, F(width), F(2.0), texture_ref.CLAMP)
    img = Desc(host)
    img.objs[floor].texture = 0
    r = img.make(images=[image])
    rays = np.ascontiguousarray(camera_rays(img.cam, 96, 64)).reshape(-1, 6)
    want_hits, want_colour = texture_ref.colours(query_ref.Scene(orc), rays, {floor: image})
    got = r.intersect_rays(rays)
    np.testing.assert_array_equal(got["object"], want_hits["object"])
    assert_same_bits(got["color"], want_colour, f"width {width}: texel colours")
