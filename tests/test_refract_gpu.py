"""Refraction (include/rt_capi_refract.h) on the GPU, every comparison bit-exact against refract_ref: a glass sphere and a clear
pane in the built-in scene through every render call, table mode and several depths; glass spheres in a clustered grid; reflective
glass deep enough that the bounce stack runs into HBM; an image floor seen through glass; the create's errors and its fall-back
to rt_scene_create / rt_scene_create_textured; the counting build's refusal; the host model; the drop-in executable's
one-GPU rule."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as oracle
import refract_ref
import texture_ref
from rays_ref import camera_rays
from test_texture_gpu import Desc, assert_same_bits, kernel
from tilecoderaytracer_amd import HostScene, Renderer, RtError, capi

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(d, refractive=None, images=None, options=None):
    """a Renderer of Desc d through rt_scene_create_refractive (refractive: [(object, tf, ior)])"""
    desc = capi.RtSceneDesc(d.n, d.objs, d.n_textures, d.texs, d.shadow[0], d.shadow[1], (C.c_float * 3)(*d.null))
    r = Renderer.from_desc(desc, d.cam, keepalive=(d, desc), images=images, refractive=refractive)
    for k, v in (options or {}).items():
        r.set_option(k, v)
    return r


def glass_builtin(scene):
    """the built-in scene with its red sphere (4) made glass and a clear finite pane added between the eye and the spheres
    (scene: HostScene or OracleScene built-in) -> the refractive list"""
    pane = scene.add_finite_plane_axes((-2.0, -1.0, 2.5), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), 2.5, 2.0)
    scene.set_color(pane, (0.2, 0.3, 0.9))
    scene.set_diffuse(pane, 0.3)
    return [(4, 0.9, 1.5), (pane, 0.8, 1.0)]


def ref_scene(oscene, refractive, images=None):
    return refract_ref.Scene(oscene, {o: (tf, ior) for o, tf, ior in refractive}, images)


# ---- 1. the built-in scene with glass, through every call -----------------------------------------------------------------

@pytest.mark.parametrize("options", [{}, {"fast": 0}, {"tables": 2}])
@pytest.mark.parametrize("depth", [0, 1, 4, 8])
def test_builtin_glass_every_call(options, depth):
    import torch
    host = HostScene.builtin()
    refr = glass_builtin(host)
    d = Desc(host)
    r = make(d, refractive=refr, options=options)
    plain = make(Desc(host), options=options)
    o = oracle.OracleScene.builtin()
    rs = ref_scene(o, glass_builtin(o))
    W, H = 64, 48
    want = refract_ref.render(rs, d.cam, W, H, depth)
    assert_same_bits(r.render(W, H, depth), want, f"render d{depth} {options}")
    plain.render(W, H, depth)
    assert kernel(r) == kernel(plain) + "_refract", (kernel(r), kernel(plain))
    buf = torch.zeros((40 - 12, H, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    r.render_device(W, H, depth, 12, 40, buf.data_ptr(), stream)
    torch.cuda.synchronize()
    assert_same_bits(buf.cpu().numpy(), want[12:40], f"render_device strip d{depth}")
    ssaa_want = refract_ref.render(rs, d.cam, 2 * W, 2 * H, depth).reshape(W, 2, H, 2, 3)
    acc = ssaa_want[:, 0, :, 0]
    for i, j in ((0, 1), (1, 0), (1, 1)):                        # the kernel's order: s = i k + j
        acc = acc + ssaa_want[:, i, :, j]
    assert_same_bits(r.render_ssaa(W, H, depth, 2), (acc * F(0.25)).astype(F), f"ssaa d{depth}")
    rays = np.ascontiguousarray(camera_rays(d.cam, W, H))
    assert_same_bits(r.trace_rays(rays, depth), want, f"trace_rays d{depth}")
    rgb, hits = r.render_gbuffer(W, H, depth, 3, W - 5)
    assert_same_bits(rgb, want[3:W - 5], f"gbuffer colours d{depth}")
    _, hits_plain = plain.render_gbuffer(W, H, depth, 3, W - 5)
    assert hits.tobytes() == hits_plain.tobytes()                  # the records stay the primary hit's


def test_refract_kernel_names_follow_one_rule():
    host = HostScene.builtin()
    refr = glass_builtin(host)
    r = make(Desc(host), refractive=refr)
    plain = make(Desc(host))
    r.render(16, 16, 2)
    plain.render(16, 16, 2)
    assert kernel(r) == "rt_render_kernel_refract" and kernel(plain) == "rt_render_kernel"
    r.render_ssaa(16, 16, 2, 2)
    assert kernel(r) == "rt_render_kernel_ssaa_refract"
    # the queries answer geometry: the *_image sibling (the tables are an image scene's)
    r.intersect_rays(np.ascontiguousarray(camera_rays(Desc(host).cam, 4, 4)))
    assert kernel(r) == "rt_render_kernel_hits_image"


# ---- 2. clustered grid with glass spheres -----------------------------------------------------------------------------------

def test_grid16_glass_spheres_clusters_kernel():
    host = HostScene.grid(16)
    o = oracle.OracleScene.grid(16)
    spheres = [i for i in range(o.object_count) if o.get_object(i).kind == 0 and not o.get_object(i).is_light]
    refr = [(spheres[k], 0.7, 1.3 + 0.1 * k) for k in (3, 40, 77, 120, 200)]
    r = make(Desc(host), refractive=refr)
    W, H, depth = 128, 96, 4
    want = refract_ref.render(ref_scene(o, refr), Desc(host).cam, W, H, depth)
    assert_same_bits(r.render(W, H, depth), want, "grid16 glass")
    assert "clusters" in kernel(r) and kernel(r).endswith("_refract"), kernel(r)


# ---- 3. reflective glass, deep, the stack in HBM ----------------------------------------------------------------------------

@pytest.mark.parametrize("stack", [0, 2])
def test_reflective_glass_depth_10_stack_in_hbm(stack):
    host = HostScene.builtin()
    host.set_reflective(4, 0.5)
    refr = [(4, 0.5, 1.5), (2, 0.5, 1.2)]                          # sphere 2 is a mirror already: rf 1 and tf 0.5
    r = make(Desc(host), refractive=refr, options={"stack": stack})
    o = oracle.OracleScene.builtin()
    o.set_reflective(4, 0.5)
    W, H, depth = 32, 32, 10
    want = refract_ref.render(ref_scene(o, refr), Desc(host).cam, W, H, depth)
    assert_same_bits(r.render(W, H, depth), want, f"reflective glass d10 stack {stack}")


# ---- 4. an image floor through glass ----------------------------------------------------------------------------------------

def test_image_floor_through_glass():
    host = HostScene.builtin()
    d = Desc(host)
    images = d.checker_images()
    rng = np.random.RandomState(5)
    floor_image = (rng.rand(7, 9, 3).astype(F), F(0.9), F(0.7), texture_ref.REPEAT)
    images.append(floor_image)
    d.objs[7].texture = d.n_textures + len(images) - 1              # the floor (object 7) samples the new image
    refr = [(4, 0.9, 1.5), (5, 0.6, 1.1)]
    r = make(d, refractive=refr, images=images)
    o = oracle.OracleScene.builtin()
    W, H, depth = 64, 64, 4
    want = refract_ref.render(ref_scene(o, refr, {7: floor_image}), d.cam, W, H, depth)
    assert_same_bits(r.render(W, H, depth), want, "image floor through glass")


# ---- 5. nothing refractive: the old create, the old kernels, the same bits -------------------------------------------------

def test_no_refraction_is_the_old_create():
    host = HostScene.builtin()
    W, H, depth = 48, 40, 4
    plain = make(Desc(host))
    want = plain.render(W, H, depth)
    for refr in ([], [(4, 0.0, 1.5)], [(4, 0.0, 1.5), (9, 0.0, 2.0)]):
        r = make(Desc(host), refractive=refr)
        assert_same_bits(r.render(W, H, depth), want, f"refractive {refr}")
        assert kernel(r) == kernel(plain)
    d = Desc(host)
    images = d.checker_images()
    textured = make(d, images=images)
    want_t = textured.render(W, H, depth)
    d2 = Desc(host)
    r = make(d2, refractive=[(4, 0.0, 1.5)], images=d2.checker_images())
    assert_same_bits(r.render(W, H, depth), want_t, "textured, tf 0")
    assert kernel(r) == kernel(textured) == kernel(plain) + "_image"


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("refr, what", [
    ([(99, 0.5, 1.5)], "out of range"),
    ([(-1, 0.5, 1.5)], "out of range"),
    ([(4, 0.5, 1.5), (4, 0.2, 1.5)], "twice"),
    ([(0, 0.5, 1.5)], "light"),
    ([(4, float("nan"), 1.5)], "refractive"),
    ([(4, -0.5, 1.5)], "refractive"),
    ([(4, 0.5, 0.0)], "ior"),
    ([(4, 0.5, -1.0)], "ior"),
    ([(4, 0.5, float("inf"))], "ior"),
    ([(4, 0.5, float("nan"))], "ior"),
])
def test_validation_errors(refr, what):
    host = HostScene.builtin()
    with pytest.raises(RtError) as e:
        make(Desc(host), refractive=refr)
    assert e.value.code == capi.RT_ERR_INVALID, e.value
    assert what in str(e.value), str(e.value)


def test_counting_build_refuses_refraction():
    host = HostScene.builtin()
    r = make(Desc(host), refractive=[(4, 0.5, 1.5)])
    with pytest.raises(RtError) as e:
        r.render_stats(16, 16, 2)
    assert e.value.code == capi.RT_ERR_INVALID
    with pytest.raises(RtError) as e:
        r.learn_tile_order(16, 16, 2)
    assert e.value.code == capi.RT_ERR_INVALID


# ---- 7. host model and the drop-in executable -------------------------------------------------------------------------------

def test_host_scene_refraction_equals_desc_scene():
    host = HostScene.builtin()
    refr = glass_builtin(host)
    for obj, tf, ior in refr:
        host.set_refraction(obj, tf, ior)
    assert host.refractions[0] == len(refr)
    r = Renderer(host)
    W, H, depth = 48, 40, 4
    got = r.render(W, H, depth)
    assert kernel(r).endswith("_refract")
    plain_host = HostScene.builtin()
    glass_builtin(plain_host)
    want = make(Desc(plain_host), refractive=refr).render(W, H, depth)
    assert_same_bits(got, want, "HostScene refraction")


def test_raytracer_refuses_refraction_on_two_gpus(tmp_path):
    exe = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
    common = [exe, "--width", "16", "--height", "16", "--depth", "2", "--no-txt"]
    p = subprocess.run(common + ["--gpus", "2", "--glass", "4:0.9:1.5"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode != 0 and "refraction renders on one GPU" in p.stderr, (p.returncode, p.stderr)
    p = subprocess.run(common + ["--gpus", "1", "--glass", "4:0.9:1.5"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-500:])
