"""The denoiser (include/rt_capi_denoise.h) on the GPU, every comparison bit-exact against denoise_ref over every pixel: rendered
one-sample soft-shadow G-buffer frames of the built-in scene, a clustered sphere field and an image-textured floor at sizes that
fit no tile, a frame of more than 1024 x 1024, every iteration count, with and without the colour term, three normal exponents;
synthetic records and colours with NaN, infinities, denormals and signed zeros; the device entry point behind the G-buffer render
on one stream; the Python wrappers; the drop-in executable."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import scene_gen
from test_soft_gpu import make
from test_texture_gpu import Desc, image_planes
from tilecoderaytracer_amd import HostScene, Renderer, capi, denoise
from tilecoderaytracer_amd.host import write_screen_txt
from tilecoderaytracer_amd.renderer import HIT_DTYPE

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_denoised(rgb, hits, iterations, sigma, squarings, what):
    got = denoise(rgb, hits, iterations, sigma, squarings)
    want = denoise_ref.denoise(rgb, hits, iterations, sigma, squarings)
    if not denoise_ref.same_bits(got, want):
        bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))
        x, z, c = bad[0]
        raise AssertionError(f"{what} it{iterations} sigma{sigma} k{squarings}: {len(bad)} values differ, first at {(x, z, c)}: "
                             f"{got[x, z, c]!r} != {want[x, z, c]!r}")
    return got


# ---- 5. rendered frames -------------------------------------------------------------------------------------------------------

def lights_of(d):
    return [i for i in range(d.n) if d.objs[i].is_light]


def soft_renderer(name):
    """the scene with every light an area light of one sample and radius 1.0"""
    if name == "builtin":
        d, images = Desc(HostScene.builtin()), None
    elif name == "field":
        d, images = Desc(scene_gen.build_sphere_field(HostScene.empty(), 3)), None
    else:
        host, floor, wall = image_planes(HostScene.empty())
        d = Desc(host)
        d.objs[floor].texture = 0
        texels = np.random.RandomState(11).uniform(0, 1, (16, 16, 3)).astype(F)
        images = [(texels, F(24.0), F(24.0), capi.RT_TEX_WRAP_REPEAT)]        # texels of 1.5 world units: several pixels each
    return make(d, [(k, 1, 1.0) for k in lights_of(d)], images=images, seed=1)


@functools.lru_cache(maxsize=None)
def frame(name, W, H, depth=3):
    rgb, hits = soft_renderer(name).render_gbuffer(W, H, depth)
    return rgb, hits


@pytest.mark.parametrize("name", ["builtin", "field", "image"])
def test_rendered_frames_every_iteration_count_sigma_and_exponent(name):
    rgb, hits = frame(name, 97, 61)
    assert (hits["object"] >= 0).mean() > 0.3
    changed = 0
    for iterations in range(1, 6):
        for sigma in (0.0, 0.8):
            for squarings in (0, 3, 6):
                got = assert_denoised(rgb, hits, iterations, sigma, squarings, name)
                changed += int((got != rgb).any())
    assert changed == 30                                     # (every one of them filtered something)


@pytest.mark.parametrize("W, H", [(1, 1), (1, 300), (300, 1), (5, 5), (2, 67), (67, 3)])
def test_sizes_smaller_than_a_tile_and_the_footprint(W, H):
    rgb, hits = frame("builtin", W, H)
    for iterations in range(1, 6):
        for sigma in (0.0, 1.0):
            assert_denoised(rgb, hits, iterations, sigma, 3, f"{W}x{H}")


def test_a_frame_of_more_than_1024_squared():
    rgb, hits = frame("builtin", 1100, 1030)
    assert_denoised(rgb, hits, 5, 1.0, 3, "1100x1030")
    assert_denoised(rgb, hits, 2, 0.0, 0, "1100x1030")


def test_a_strip_differs_from_the_frame_only_near_its_edges():
    """the header: within 2 * (2^iterations - 1) columns of the strip's edges, and nowhere else"""
    rgb, hits = frame("builtin", 97, 61)
    for iterations in (1, 3):
        full = denoise(rgb, hits, iterations, 1.0, 3)
        strip = denoise(rgb[20:80], hits[20:80], iterations, 1.0, 3)
        m = 2 * (2 ** iterations - 1)
        assert denoise_ref.same_bits(strip[m:60 - m], full[20 + m:80 - m])
        assert not denoise_ref.same_bits(strip, full[20:80])


# ---- 6. synthetic records and colours -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(20))
def test_synthetic_records_and_special_values(seed):
    rng = np.random.default_rng(1000 + seed)
    Wn, H = int(rng.integers(1, 150)), int(rng.integers(1, 150))
    special = np.array([np.nan, np.inf, -np.inf, 1e-40, -1e-45, -0.0, 0.0, 3e38, -3e38, 1e-38], dtype=F)
    rgb = rng.random((Wn, H, 3), dtype=F)
    where = rng.random((Wn, H, 3)) < 0.03
    rgb[where] = special[rng.integers(0, len(special), int(where.sum()))]
    hits = np.zeros((Wn, H), dtype=HIT_DTYPE)
    hits["object"] = rng.integers(-2, 4, (Wn, H))
    palette = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5000001], [0.0, 0.0, 0.0], [0.0, -0.0, 0.0], [np.nan, 1.0, 1.0]], dtype=F)
    hits["color"] = palette[rng.integers(0, len(palette), (Wn, H))]
    n = rng.normal(size=(Wn, H, 3)).astype(F) + np.array([0, 2, 0], dtype=F)
    scale = np.array([1.0, 1e-3, 50.0, 1e10, 1e-20], dtype=F)[rng.integers(0, 5, (Wn, H))]      # 1e10: the squarings overflow
    n = n * scale[..., None]
    n[rng.random((Wn, H)) < 0.05] = 0.0
    n[rng.random((Wn, H, 3)) < 0.01] = np.nan
    hits["normal"] = n
    hits["flags"] = np.where(rng.random((Wn, H)) < 0.9, rng.integers(0, 2, (Wn, H)), rng.integers(0, 4, (Wn, H)))
    hits["distance"] = rng.random((Wn, H), dtype=F)
    hits["point"] = rng.random((Wn, H, 3), dtype=F)
    iterations = 1 + seed % 5
    sigma = [0.0, 0.5, 1.0, 1e-30, 1e25][seed % 5 if seed < 10 else (seed // 2) % 5]
    squarings = [0, 3, 6, 1][seed % 4]
    got = assert_denoised(rgb, hits, iterations, sigma, squarings, f"seed {seed} {Wn}x{H}")
    assert_denoised(rgb, hits, 2, 1.0, 3, f"seed {seed} {Wn}x{H}")
    passthrough = (hits["object"] < 0) | ((hits["flags"] & 2) != 0)
    assert np.array_equal(got.view(np.uint32)[passthrough], rgb.view(np.uint32)[passthrough])


# ---- 7. the device entry point and the wrappers --------------------------------------------------------------------------------

@pytest.mark.parametrize("iterations", [1, 2, 3])
def test_device_path_behind_the_gbuffer_render_on_one_stream(iterations):
    import torch
    lib = capi.load_library()
    W, H, depth = 203, 131, 3
    r = soft_renderer("builtin")
    rgb, hits = r.render_gbuffer(W, H, depth)
    want = denoise(rgb, hits, iterations, 1.0, 3)
    params = capi.RtDenoiseParams(iterations, 3, 1.0)
    nbytes = lib.rt_denoise_scratch_bytes(C.byref(params), W, H)
    assert nbytes >= 32 * W * H
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_rgb = torch.zeros((W, H, 3), dtype=torch.float32, device="cuda")
        d_hits = torch.zeros((W * H * 12,), dtype=torch.int32, device="cuda")
        d_out = torch.full((W, H, 3), -1.0, dtype=torch.float32, device="cuda")
        d_scratch = torch.zeros((nbytes // 4 + 4,), dtype=torch.int32, device="cuda")
        assert stream.cuda_stream != 0 and d_hits.data_ptr() % 16 == 0 and d_scratch.data_ptr() % 16 == 0
        r.render_gbuffer_device(W, H, depth, 0, W, d_rgb.data_ptr(), d_hits.data_ptr(), stream.cuda_stream)
        capi.check(lib.rt_denoise_device(0, C.byref(params), W, H, d_rgb.data_ptr(), d_hits.data_ptr(), d_out.data_ptr(),
                                         d_scratch.data_ptr(), stream.cuda_stream))      # (no host wait in between)
    stream.synchronize()
    assert denoise_ref.same_bits(d_out.cpu().numpy(), want)
    assert np.array_equal(d_rgb.cpu().numpy().view(np.uint32), rgb.view(np.uint32))      # the inputs are only read
    assert d_hits.cpu().numpy().tobytes() == hits.tobytes()
    # the device checks that need a device to matter: a device index out of range
    assert lib.rt_denoise_device(99, C.byref(params), W, H, d_rgb.data_ptr(), d_hits.data_ptr(), d_out.data_ptr(),
                                 d_scratch.data_ptr(), None) == capi.RT_ERR_INVALID


def test_render_denoised_is_denoise_of_render_gbuffer():
    r = soft_renderer("builtin")
    W, H, depth = 150, 90, 3
    rgb, hits = r.render_gbuffer(W, H, depth)
    for args in ((2, 1.0, 3), (3, 0.0, 0)):
        got_rgb, got_hits, ms = r.render_denoised(W, H, depth, *args)
        assert denoise_ref.same_bits(got_rgb, denoise(rgb, hits, *args))
        assert got_hits.tobytes() == hits.tobytes() and ms > 0.0
    out = denoise(rgb, hits)
    assert denoise_ref.same_bits(out, denoise_ref.denoise(rgb, hits))
    in_place, ms = rgb.copy(), C.c_double(0.0)               # the host call may filter in place; it reports its kernels' time
    params = capi.RtDenoiseParams(2, 3, 1.0)
    capi.check(capi.load_library().rt_denoise(0, C.byref(params), W, H, in_place.ctypes.data, hits.ctypes.data,
                                              in_place.ctypes.data, C.byref(ms)))
    assert denoise_ref.same_bits(in_place, out) and ms.value > 0.0


# ---- 8. the drop-in executable ------------------------------------------------------------------------------------------------

def test_raytracer_denoise_writes_the_reference_filter_of_its_own_frame(tmp_path):
    exe = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
    W, H, depth = 64, 48, 3
    common = [exe, "--width", str(W), "--height", str(H), "--depth", str(depth), "--soft", "0:1:1.0"]
    noisy_txt, hits_bin, out_txt, want_txt = (tmp_path / n for n in ("noisy.txt", "hits.bin", "out.txt", "want.txt"))
    p = subprocess.run(common + ["--out", str(noisy_txt), "--hits", str(hits_bin)], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    p = subprocess.run(common + ["--out", str(out_txt), "--denoise", "2:1.0:3"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0 and "Denoise kernels (ms)" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    # its own undenoised frame: the same scene through the library (the .txt rounds the colours, so the frame is rendered here
    # and checked against the executable's .txt)
    host = HostScene.builtin()
    host.set_area_light(0, 1, 1.0)
    rgb, hits = Renderer(host).render_gbuffer(W, H, depth)
    assert hits.tobytes() == hits_bin.read_bytes()
    write_screen_txt(str(want_txt), rgb)
    assert noisy_txt.read_text().splitlines()[10:] == want_txt.read_text().splitlines()[10:]
    write_screen_txt(str(want_txt), denoise_ref.denoise(rgb, hits, 2, 1.0, 3))
    got_lines, want_lines = out_txt.read_text().splitlines()[10:], want_txt.read_text().splitlines()[10:]
    assert len(got_lines) == W * H and got_lines == want_lines
    assert got_lines != noisy_txt.read_text().splitlines()[10:]
