"""Soft shadows (include/rt_capi_soft.h) on the GPU, every comparison bit-exact against soft_ref: the built-in scene with both
lights made area lights through every render call, table mode and several depths; strips; clustered grids with the SHADOW
VOXELS on and off and with HELP forced and timed out; an image floor and glass; seeds; a bounce stack in HBM; the kernel
names; the counting build's refusal; the host model and the drop-in executable."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as oracle
import soft_ref
import texture_ref
from rays_ref import camera_rays
from test_texture_gpu import Desc, assert_same_bits, kernel
from tilecoderaytracer_amd import HostScene, Renderer, RtError, capi
from tilecoderaytracer_amd.host import write_screen_txt

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(d, area, refractive=None, images=None, options=None, seed=None):
    """a Renderer of Desc d through rt_scene_create_soft (area: [(object, samples, radius)])"""
    desc = capi.RtSceneDesc(d.n, d.objs, d.n_textures, d.texs, d.shadow[0], d.shadow[1], (C.c_float * 3)(*d.null))
    r = Renderer.from_desc(desc, d.cam, keepalive=(d, desc), images=images, refractive=refractive, area_lights=area)
    for k, v in (options or {}).items():
        r.set_option(k, v)
    if seed is not None:
        r.set_shadow_seed(seed)
    return r


def lights_of(o):
    return [i for i in range(o.object_count) if o.get_object(i).is_light]


def ref_scene(o, area, seed=0, refractive=None, images=None):
    return soft_ref.Scene(o, {k: (n, r) for k, n, r in area}, seed,
                          {k: (tf, ior) for k, tf, ior in (refractive or [])}, images)


# ---- 1. the built-in scene, both lights area lights, through every call ----------------------------------------------------

SAMPLINGS = [(1, 0.15), (2, 0.15), (2, 0.6), (4, 1.0)]
W1, H1 = 40, 32


@functools.lru_cache(maxsize=None)
def builtin_want(n, r, depth):
    o = oracle.OracleScene.builtin()
    rs = ref_scene(o, [(k, n, r) for k in lights_of(o)])
    cam = Desc(HostScene.builtin()).cam
    return soft_ref.render(rs, cam, W1, H1, depth), soft_ref.render_ssaa(rs, cam, W1, H1, depth, 2)


@pytest.mark.parametrize("options", [{}, {"fast": 0}, {"tables": 2}])
@pytest.mark.parametrize("depth", [0, 1, 4])
@pytest.mark.parametrize("n, r", SAMPLINGS)
def test_builtin_soft_every_call(n, r, depth, options):
    import torch
    host = HostScene.builtin()
    d = Desc(host)
    area = [(0, n, r), (1, n, r)]
    s = make(d, area, options=options)
    plain = Desc(host).make(options=options)
    want, ssaa_want = builtin_want(n, r, depth)
    W, H = W1, H1
    assert_same_bits(s.render(W, H, depth), want, f"render n{n} r{r} d{depth} {options}")
    plain.render(W, H, depth)
    assert kernel(s) == kernel(plain) + "_soft", (kernel(s), kernel(plain))
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros((30 - 7, H, 3), dtype=torch.float32, device="cuda")
    s.render_device(W, H, depth, 7, 30, buf.data_ptr(), stream)
    torch.cuda.synchronize()
    assert_same_bits(buf.cpu().numpy(), want[7:30], f"render_device strip d{depth}")
    assert_same_bits(s.render_ssaa(W, H, depth, 2), ssaa_want, f"ssaa d{depth}")
    assert kernel(s).endswith("_ssaa_soft"), kernel(s)
    sbuf = torch.zeros((W, H, 3), dtype=torch.float32, device="cuda")
    s.render_ssaa_device(W, H, depth, 2, 0, W, sbuf.data_ptr(), stream)
    torch.cuda.synchronize()
    assert_same_bits(sbuf.cpu().numpy(), ssaa_want, f"ssaa_device d{depth}")
    # a ray batch's key is the ray index: the camera's rays in the frame's order are the frame (x * H + z)
    rays = np.ascontiguousarray(camera_rays(d.cam, W, H))
    assert_same_bits(s.trace_rays(rays, depth), want, f"trace_rays d{depth}")
    assert kernel(s).endswith("_rays_soft"), kernel(s)
    drays = torch.from_numpy(rays.reshape(-1, 6)).cuda()
    dout = torch.zeros((W * H, 3), dtype=torch.float32, device="cuda")
    s.trace_rays_device(W * H, H, drays.data_ptr(), depth, dout.data_ptr(), stream)
    torch.cuda.synchronize()
    assert_same_bits(dout.cpu().numpy().reshape(W, H, 3), want, f"trace_rays_device d{depth}")
    rgb, hits = s.render_gbuffer(W, H, depth, 3, W - 5)
    assert_same_bits(rgb, want[3:W - 5], f"gbuffer colours d{depth}")
    assert kernel(s).endswith("_gbuffer_soft"), kernel(s)
    _, hits_plain = plain.render_gbuffer(W, H, depth, 3, W - 5)
    assert hits.tobytes() == hits_plain.tobytes()                  # the records do not change
    grgb = torch.zeros((W, H, 3), dtype=torch.float32, device="cuda")
    ghits = torch.zeros((W * H * 12,), dtype=torch.float32, device="cuda")
    s.render_gbuffer_device(W, H, depth, 0, W, grgb.data_ptr(), ghits.data_ptr(), stream)
    torch.cuda.synchronize()
    assert_same_bits(grgb.cpu().numpy(), want, f"gbuffer_device d{depth}")


def test_strips_equal_the_full_frame():
    host = HostScene.builtin()
    s = make(Desc(host), [(0, 4, 0.8), (1, 2, 0.4)], seed=11)
    W, H, depth = 96, 40, 3
    full = s.render(W, H, depth)
    o = oracle.OracleScene.builtin()
    want = soft_ref.render(ref_scene(o, [(0, 4, 0.8), (1, 2, 0.4)], 11), Desc(host).cam, W, H, depth)
    assert_same_bits(full, want, "full frame")
    for x0, x1 in ((0, 17), (17, 64), (64, 96), (5, 6)):
        assert_same_bits(s.render(W, H, depth, x0, x1), full[x0:x1], f"strip {x0}:{x1}")


def test_one_area_light_one_hard_light():
    host = HostScene.builtin()
    area = [(1, 2, 0.5)]
    s = make(Desc(host), area)
    o = oracle.OracleScene.builtin()
    W, H, depth = 48, 40, 4
    assert_same_bits(s.render(W, H, depth), soft_ref.render(ref_scene(o, area), Desc(host).cam, W, H, depth), "light 1 soft")


# ---- 2. clustered grids: SHADOW VOXELS, HELP ---------------------------------------------------------------------------------

@pytest.mark.parametrize("svox", [0, 800, 4096])
@pytest.mark.parametrize("name, W, H, depth", [("grid16", 64, 48, 4), ("grid32", 64, 48, 3)])
def test_grid_soft_shadow_voxels(name, W, H, depth, svox):
    host = HostScene.named(name)
    o = oracle.OracleScene.named(name)
    area = [(k, 2, 0.5) for k in lights_of(o)]
    s = make(Desc(host), area, options={"svox": svox})
    want = soft_ref.render(ref_scene(o, area), Desc(host).cam, W, H, depth)
    assert_same_bits(s.render(W, H, depth), want, f"{name} svox {svox}")
    assert "clusters" in kernel(s) and kernel(s).endswith("_soft"), kernel(s)


def test_grid_soft_help_forced_and_timed_out():
    name, W, H, depth = "grid16", 64, 48, 5
    host = HostScene.named(name)
    o = oracle.OracleScene.named(name)
    area = [(k, 2, 0.7) for k in lights_of(o)]
    want = soft_ref.render(ref_scene(o, area), Desc(host).cam, W, H, depth)
    s = make(Desc(host), area, options={"help": 2, "block_threads": 256})
    assert_same_bits(s.render(W, H, depth), want, "HELP forced")
    lib = capi.load_library()
    s.set_option("help_spin_limit", -1)
    out = np.zeros((W, H, 3), dtype=np.float32)
    rc = lib.rt_render(s._scene, s._cam, W, H, 0, W, depth, out.ctypes.data)
    assert rc in (capi.RT_OK, capi.RT_ERR_HIP)
    assert_same_bits(out, want, "HELP timeout path")
    s.set_option("help_spin_limit", 1 << 22)
    assert_same_bits(s.render(W, H, depth), want, "usable afterwards")


# ---- 3. with image textures and glass ----------------------------------------------------------------------------------------

def test_soft_with_image_floor():
    host = HostScene.builtin()
    d = Desc(host)
    images = d.checker_images()
    rng = np.random.RandomState(5)
    floor_image = (rng.rand(7, 9, 3).astype(F), F(0.9), F(0.7), texture_ref.REPEAT)
    images.append(floor_image)
    d.objs[7].texture = d.n_textures + len(images) - 1
    area = [(0, 2, 0.5), (1, 3, 0.3)]
    s = make(d, area, images=images)
    o = oracle.OracleScene.builtin()
    W, H, depth = 48, 48, 3
    want = soft_ref.render(ref_scene(o, area, images={7: floor_image}), d.cam, W, H, depth)
    assert_same_bits(s.render(W, H, depth), want, "soft + image floor")


@pytest.mark.parametrize("call", ["render", "ssaa", "rays", "gbuffer"])
def test_soft_with_glass(call):
    host = HostScene.builtin()
    d = Desc(host)
    area = [(0, 2, 0.5), (1, 2, 0.5)]
    refr = [(4, 0.9, 1.5), (5, 0.5, 1.2)]
    s = make(d, area, refractive=refr, seed=5)
    o = oracle.OracleScene.builtin()
    rs = ref_scene(o, area, 5, refr)
    W, H, depth = 32, 32, 4
    if call == "render":
        assert_same_bits(s.render(W, H, depth), soft_ref.render(rs, d.cam, W, H, depth), "glass")
        assert kernel(s) == "rt_render_kernel_refract_soft", kernel(s)
    elif call == "ssaa":
        assert_same_bits(s.render_ssaa(W, H, depth, 2), soft_ref.render_ssaa(rs, d.cam, W, H, depth, 2), "glass ssaa")
        assert kernel(s) == "rt_render_kernel_ssaa_refract_soft", kernel(s)
    elif call == "rays":
        rays = np.ascontiguousarray(camera_rays(d.cam, W, H))
        assert_same_bits(s.trace_rays(rays, depth), soft_ref.render(rs, d.cam, W, H, depth), "glass rays")
        assert kernel(s) == "rt_render_kernel_rays_refract_soft", kernel(s)
    else:
        rgb, _ = s.render_gbuffer(W, H, depth)
        assert_same_bits(rgb, soft_ref.render(rs, d.cam, W, H, depth), "glass gbuffer")
        assert kernel(s) == "rt_render_kernel_gbuffer_refract_soft", kernel(s)


# ---- 4. seeds, depth, names, fall-back -----------------------------------------------------------------------------------------

def test_seeds():
    host = HostScene.builtin()
    area = [(0, 2, 0.6), (1, 2, 0.6)]
    s = make(Desc(host), area)
    W, H, depth = 48, 40, 2
    a0 = s.render(W, H, depth)
    s.set_shadow_seed(12345)
    a1 = s.render(W, H, depth)
    a1_again = s.render(W, H, depth)
    assert not np.array_equal(a0.view(np.uint32), a1.view(np.uint32))
    assert_same_bits(a1, a1_again, "same seed")
    o = oracle.OracleScene.builtin()
    assert_same_bits(a1, soft_ref.render(ref_scene(o, area, 12345), Desc(host).cam, W, H, depth), "seed 12345")
    s.set_shadow_seed(0)
    assert_same_bits(s.render(W, H, depth), a0, "back to seed 0")


@pytest.mark.parametrize("stack", [0, 2])
def test_deep_stack_in_hbm(stack):
    host = HostScene.builtin()
    area = [(0, 2, 0.5), (1, 1, 0.5)]
    s = make(Desc(host), area, options={"stack": stack})
    o = oracle.OracleScene.builtin()
    W, H, depth = 24, 24, 10
    assert_same_bits(s.render(W, H, depth), soft_ref.render(ref_scene(o, area), Desc(host).cam, W, H, depth), f"d10 stack {stack}")


def test_soft_kernel_names():
    host = HostScene.builtin()
    s = make(Desc(host), [(0, 2, 0.5)])
    s.render(16, 16, 2)
    assert kernel(s) == "rt_render_kernel_soft"
    s.render_ssaa(16, 16, 2, 2)
    assert kernel(s) == "rt_render_kernel_ssaa_soft"
    s.trace_rays(np.ascontiguousarray(camera_rays(Desc(host).cam, 4, 4)), 2)
    assert kernel(s) == "rt_render_kernel_rays_soft"
    s.render_gbuffer(16, 16, 2)
    assert kernel(s) == "rt_render_kernel_gbuffer_soft"
    s.intersect_rays(np.ascontiguousarray(camera_rays(Desc(host).cam, 4, 4)))
    assert kernel(s) == "rt_render_kernel_hits_image"          # the queries answer geometry
    s.set_option("fast", 0)
    s.render(16, 16, 2)
    assert kernel(s) == "rt_render_kernel_items_soft"
    s.set_option("tables", 2)
    s.render(16, 16, 2)
    assert kernel(s) == "rt_render_kernel_large_soft"


def test_radius_zero_is_the_old_create():
    host = HostScene.builtin()
    W, H, depth = 48, 40, 4
    plain = Desc(host).make()
    want = plain.render(W, H, depth)
    for area in ([], [(0, 4, 0.0)], [(0, 4, 0.0), (1, 8, 0.0)]):
        s = make(Desc(host), area)
        assert_same_bits(s.render(W, H, depth), want, f"area {area}")
        assert kernel(s) == kernel(plain)
    s = make(Desc(host), [(0, 4, 0.0)], refractive=[(4, 0.9, 1.5)])
    s.render(W, H, depth)
    assert kernel(s) == "rt_render_kernel_refract", kernel(s)


def test_counting_build_refuses_area_lights():
    host = HostScene.builtin()
    s = make(Desc(host), [(0, 2, 0.5)])
    with pytest.raises(RtError) as e:
        s.render_stats(16, 16, 2)
    assert e.value.code == capi.RT_ERR_INVALID and "area lights" in str(e.value)
    with pytest.raises(RtError) as e:
        s.learn_tile_order(16, 16, 2)
    assert e.value.code == capi.RT_ERR_INVALID and "area lights" in str(e.value)


# ---- 5. host model and the drop-in executable -------------------------------------------------------------------------------

def test_host_scene_area_lights_equal_desc_scene():
    host = HostScene.builtin()
    host.set_area_light(0, 2)                        # its own radius, 0.15
    host.set_area_light(1, 3, 0.9)
    r = Renderer(host)
    r.set_shadow_seed(9)
    W, H, depth = 48, 40, 4
    got = r.render(W, H, depth)
    assert kernel(r) == "rt_render_kernel_soft"
    want = make(Desc(HostScene.builtin()), [(0, 2, F(0.15)), (1, 3, 0.9)], seed=9).render(W, H, depth)
    assert_same_bits(got, want, "HostScene area lights")


def test_raytracer_soft(tmp_path):
    exe = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
    W, H, depth = 40, 32, 3
    common = [exe, "--width", str(W), "--height", str(H), "--depth", str(depth), "--no-txt"]
    p = subprocess.run(common + ["--gpus", "2", "--soft", "0:2:0.5"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode != 0 and "soft shadows render on one GPU" in p.stderr, (p.returncode, p.stderr)
    common = [exe, "--width", str(W), "--height", str(H), "--depth", str(depth)]
    out = tmp_path / "soft.txt"
    p = subprocess.run(common + ["--gpus", "1", "--soft", "0:2:0.5", "--soft", "1:4", "--out", str(out)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    o = oracle.OracleScene.builtin()
    want = soft_ref.render(ref_scene(o, [(0, 2, 0.5), (1, 4, F(0.15))]), Desc(HostScene.builtin()).cam, W, H, depth)
    ref_txt = tmp_path / "want.txt"
    write_screen_txt(str(ref_txt), want)
    # the pixel lines (the ten header lines carry timings)
    got_lines, want_lines = out.read_text().splitlines()[10:], ref_txt.read_text().splitlines()[10:]
    assert len(got_lines) == W * H and got_lines == want_lines
    hard_txt = tmp_path / "hard.txt"
    write_screen_txt(str(hard_txt), o.render(W, H, depth))
    assert hard_txt.read_text().splitlines()[10:] != want_lines      # (the soft frame is not the hard one)
