"""The image encoder (include/rt_capi_image.h) on the GPU, every comparison over every output byte against image_ref: sizes that
fit no tile, every threshold and its two neighbours, a sweep of the fp32 bit patterns, custom tables, the bytes that must stay
untouched at every alignment, strips into a wider image, rendered frames through the wrappers and the device entry point on a
stream, and the executable's --ppm."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import image_ref
from tilecoderaytracer_amd import HostScene, Renderer, capi, encode_image
from tilecoderaytracer_amd.renderer import image_params

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
SPECIAL = np.array([np.nan, np.inf, -np.inf, 1e-40, -1e-45, -0.0, 0.0, 3e38, -3e38, 1e-38, 1.0, 0.5], dtype=F)


def random_frame(seed, Wn, H):
    """colours uniform in [-0.1, 1.2] with 3 % special values"""
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(-0.1, 1.2, (Wn, H, 3)).astype(F)
    where = rng.random((Wn, H, 3)) < 0.03
    rgb[where] = SPECIAL[rng.integers(0, len(SPECIAL), int(where.sum()))]
    return rgb


def assert_same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        at = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {got.size} bytes differ, first at {at}: got {got[at]}, want {want[at]}")


def assert_encoded(rgb, what, transfer="srgb", thresholds=None, **kw):
    """the host entry point, through the wrapper, against image_ref"""
    T = np.asarray(thresholds, dtype=F) if thresholds is not None else image_ref.table(transfer)
    got = encode_image(rgb, transfer=transfer, thresholds=thresholds, **kw)
    assert_same_bytes(got, image_ref.encode(rgb, T, kw.get("channels", 3), kw.get("exposure", 1.0), kw.get("bottom_up", False)),
                      f"{what} {kw}")
    return got


def device_encode(rgb, pitch, before, total, x0=0, into=None, **kw):
    """rt_encode_image_device into `total` bytes of device memory pre-filled with FILL, the image's first row `before` bytes
    after the (256-byte aligned) start of the buffer, the strip's first column x0 -> all `total` bytes"""
    import torch
    params, table = image_params(**kw)
    Wn, H = rgb.shape[:2]
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda") if into is None else into
    assert buf.data_ptr() % 256 == 0
    d_rgb = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
    capi.check(capi.load_library().rt_encode_image_device(0, C.byref(params), Wn, H, d_rgb.data_ptr(),
                                                          buf.data_ptr() + before + x0 * params.channels, pitch, None))
    torch.cuda.synchronize()
    return buf if into is not None else buf.cpu().numpy()


# ---- 1. sizes that fit no tile ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Wn, H", [(1, 1), (1, 300), (300, 1), (5, 5), (2, 67), (67, 3), (65, 129), (130, 63), (1100, 1030)])
def test_sizes_that_fit_no_tile(Wn, H):
    rgb = random_frame(Wn * 7919 + H, Wn, H)
    seen = set()
    for channels in (3, 4):
        for bottom_up in (False, True):
            for exposure in (1.0, 0.37):
                got = assert_encoded(rgb, f"{Wn}x{H}", channels=channels, bottom_up=bottom_up, exposure=exposure)
                seen |= set(np.unique(got[..., :3]).tolist())
    if Wn * H >= 4000:
        assert len(seen) == 256                             # (the frames exercise every code)


# ---- 2. every threshold and its two neighbours ------------------------------------------------------------------------------------

@pytest.mark.parametrize("transfer", ["srgb", "linear"])
def test_every_threshold_and_its_neighbours(transfer):
    T = image_ref.table(transfer)
    values = np.stack([np.nextafter(T, F(-np.inf)), T, np.nextafter(T, F(np.inf))], axis=1)     # (255, 3): code k-1, k, k
    want_codes = np.stack([np.arange(0, 255), np.arange(1, 256), np.arange(1, 256)], axis=1).astype(np.uint8)
    assert np.array_equal(image_ref.codes(values, T), want_codes)
    frame = values.reshape(15, 17, 3)
    for channels in (3, 4):
        got = assert_encoded(frame, transfer, transfer=transfer, channels=channels, bottom_up=True)
        assert np.array_equal(got[..., :3].transpose(1, 0, 2).reshape(255, 3), want_codes)
        for exposure in (2.0, 0.5):                         # the same values divided by the exposure: both exact
            scaled = frame / F(exposure)
            assert np.array_equal(scaled * F(exposure), frame)
            got = assert_encoded(scaled, f"{transfer} / {exposure}", transfer=transfer, channels=channels, bottom_up=True,
                                 exposure=exposure)
            assert np.array_equal(got[..., :3].transpose(1, 0, 2).reshape(255, 3), want_codes)


# ---- 3. a sweep of the fp32 bit patterns --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pattern_frame():
    """every 1365th fp32 bit pattern of the whole 2^32 range: 1024 x 1024 x 3 of them"""
    bits = np.arange(1024 * 1024 * 3, dtype=np.uint64) * np.uint64(1365)
    assert int(bits[-1]) < 1 << 32
    frame = bits.astype(np.uint32).view(F).reshape(1024, 1024, 3)
    frame.setflags(write=False)
    return frame


@pytest.mark.parametrize("exposure", [1.0, 1e-3, 3e38])
def test_a_sweep_of_bit_patterns(exposure):
    """exposure 3e38 overflows most products to infinity, 1e-3 takes small ones into the denormals"""
    frame = pattern_frame()
    with np.errstate(all="ignore"):
        v = frame * F(exposure)
    assert np.isnan(v).sum() > 10000
    if exposure > 1:
        assert np.isinf(v).sum() > 100000
    else:
        assert ((v != 0) & (np.abs(v) < np.finfo(F).tiny)).sum() > 1000
    got = assert_encoded(frame, "patterns", exposure=exposure, channels=3)
    # (under 3e38 the inputs that land in [0, 1] are denormals, 1365 x 2^-149 x 3e38 = 5.7e-4 apart: wider than the lowest codes)
    assert len(np.unique(got)) == 256 if exposure <= 1 else len(np.unique(got)) > 200


# ---- 4. custom tables ---------------------------------------------------------------------------------------------------------

def custom_tables():
    gamma = (((np.arange(1, 256) - 0.5) / 255.0) ** 2.0).astype(F)
    runs = np.repeat(np.linspace(0.05, 0.95, 51, dtype=F), 5)
    edges = image_ref.linear_formula()
    edges[0], edges[199:] = -np.inf, np.inf
    return {"gamma2": gamma, "runs": runs, "infinite": edges}


@pytest.mark.parametrize("name", ["gamma2", "runs", "infinite"])
def test_custom_tables(name):
    T = custom_tables()[name]
    rgb = random_frame(31, 131, 70)
    rgb[:9, :5] = np.stack([np.nextafter(T[:45], F(-np.inf)), T[:45], np.nextafter(T[:45], F(np.inf))], axis=1).reshape(9, 5, 3)
    for channels, exposure in ((3, 1.0), (4, 0.37), (3, 2.0)):
        got = assert_encoded(rgb, name, thresholds=T, channels=channels, exposure=exposure)
    codes = set(np.unique(got[..., :3]).tolist())
    if name == "runs":
        assert codes == set(range(0, 256, 5))               # codes inside a run never occur
    if name == "infinite":
        assert codes == set(range(1, 200)) | {0, 255}       # 0: NaN alone; 255: +inf alone; 200..254 never
    # a table is copied by the call: the host entry point, the thresholds in a buffer freed right after
    params, table = image_params(thresholds=T.copy())
    out = np.empty((70, 131, 3), dtype=np.uint8)
    capi.check(capi.load_library().rt_encode_image(0, C.byref(params), 131, 70, rgb.ctypes.data, out.ctypes.data, 131 * 3, None))
    assert_same_bytes(out, image_ref.encode(rgb, T), name)


# ---- 5. untouched bytes and alignment -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("Wn", [1, 2, 3, 5, 67, 131, 300])
@pytest.mark.parametrize("channels", [3, 4])
def test_untouched_bytes_at_every_alignment(Wn, channels):
    """out pre-filled with 0xA5, a pitch 7 (or 8) bytes wider than a row, the image anywhere inside a larger allocation: the bytes
    before the first row, between the rows and after the last are still 0xA5, and the rows are image_ref's"""
    H, guard = 37, 512
    T = image_ref.table("srgb")
    rgb = random_frame(100 + Wn, Wn, H)
    pitch = Wn * channels + (7 if channels == 3 else 8)
    total = 2 * guard + H * pitch
    for offset in ((0, 1, 2, 3) if channels == 3 else (0, 4)):
        for bottom_up in (False, True):
            got = device_encode(rgb, pitch, guard + offset, total, channels=channels, bottom_up=bottom_up)
            want = np.full(total, FILL, dtype=np.uint8)
            image_ref.encode_into(want[guard + offset:], pitch, 0, rgb, T, channels, 1.0, bottom_up)
            assert_same_bytes(got, want, f"Wn {Wn} C {channels} offset {offset} bottom_up {bottom_up}")
    # the host entry point leaves the same bytes alone
    params, _ = image_params(channels=channels)
    out = np.full(total, FILL, dtype=np.uint8)
    capi.check(capi.load_library().rt_encode_image(0, C.byref(params), Wn, H, rgb.ctypes.data, out.ctypes.data + guard, pitch, None))
    want = np.full(total, FILL, dtype=np.uint8)
    image_ref.encode_into(want[guard:], pitch, 0, rgb, T, channels)
    assert_same_bytes(out, want, f"host Wn {Wn} C {channels}")


# ---- 6. strips ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [3, 4])
def test_strips_into_a_wider_image_equal_the_whole_frame(channels):
    import torch
    W, H = 97, 61
    rgb = random_frame(5, W, H)
    pitch = W * channels + (5 if channels == 3 else 12)
    total = H * pitch
    whole = device_encode(rgb, pitch, 0, total, channels=channels)
    buf = torch.full((total,), FILL, dtype=torch.uint8, device="cuda")
    for x0, x1 in ((0, 20), (20, 80), (80, 97)):
        device_encode(rgb[x0:x1], pitch, 0, total, x0=x0, into=buf, channels=channels)
    assert_same_bytes(buf.cpu().numpy(), whole, f"strips C {channels}")
    want = np.full(total, FILL, dtype=np.uint8)
    assert_same_bytes(whole, image_ref.encode_into(want, pitch, 0, rgb, image_ref.table("srgb"), channels), "whole")
    dense = encode_image(rgb, channels=channels)
    assert_same_bytes(whole[np.add.outer(np.arange(H) * pitch, np.arange(W * channels))].reshape(H, W, channels), dense,
                      "pitch against dense")


# ---- 7. rendered frames -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def builtin_renderer():
    return Renderer(HostScene.builtin())


def test_rendered_frame_and_render_image():
    r = builtin_renderer()
    W, H, depth = 97, 61, 3
    rgb = r.render(W, H, depth)
    T = image_ref.table("srgb")
    want = image_ref.encode(rgb, T)
    assert len(np.unique(want)) > 50                         # (a picture, not a flat field)
    assert_same_bytes(encode_image(rgb), want, "encode_image(render)")
    assert_same_bytes(r.render_image(W, H, depth), want, "render_image")
    assert_same_bytes(r.render_image(W, H, depth, channels=4, bottom_up=True, exposure=0.5, transfer="linear"),
                      image_ref.encode(rgb, image_ref.table("linear"), 4, 0.5, True), "render_image, 4 channels")
    ssaa = r.render_ssaa(W, H, depth, 2)
    assert not np.array_equal(ssaa, rgb)
    assert_same_bytes(r.render_image(W, H, depth, samples=2), image_ref.encode(ssaa, T), "render_image, 2 x 2 samples")


def test_device_path_behind_the_render_on_one_stream():
    import torch
    lib = capi.load_library()
    r = builtin_renderer()
    W, H, depth = 203, 131, 3
    rgb = r.render(W, H, depth)
    params, _ = image_params(channels=4)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_rgb = torch.zeros((W, H, 3), dtype=torch.float32, device="cuda")
        d_out = torch.full((H, W, 4), FILL, dtype=torch.uint8, device="cuda")
        assert stream.cuda_stream != 0
        r.render_device(W, H, depth, 0, W, d_rgb.data_ptr(), stream.cuda_stream)
        capi.check(lib.rt_encode_image_device(0, C.byref(params), W, H, d_rgb.data_ptr(), d_out.data_ptr(), W * 4,
                                              stream.cuda_stream))                   # (no host wait in between)
    stream.synchronize()
    assert_same_bytes(d_out.cpu().numpy(), image_ref.encode(rgb, image_ref.table("srgb"), 4), "device path")
    assert np.array_equal(d_rgb.cpu().numpy().view(np.uint32), rgb.view(np.uint32))                # the input is only read
    # the check that needs a device to matter: a device index out of range
    assert lib.rt_encode_image_device(99, C.byref(params), W, H, d_rgb.data_ptr(), d_out.data_ptr(), W * 4,
                                      None) == capi.RT_ERR_INVALID
    assert "device index" in lib.rt_last_error().decode()
    ms = C.c_double(0.0)
    out = np.empty((H, W, 4), dtype=np.uint8)
    capi.check(lib.rt_encode_image(0, C.byref(params), W, H, rgb.ctypes.data, out.ctypes.data, W * 4, C.byref(ms)))
    assert ms.value > 0.0


# ---- 8. the drop-in executable ------------------------------------------------------------------------------------------------

def test_raytracer_ppm_is_the_reference_encode_of_its_own_frame(tmp_path):
    exe = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
    W, H, depth = 64, 48, 3
    common = [exe, "--width", str(W), "--height", str(H), "--depth", str(depth), "--no-txt"]
    T = image_ref.table("srgb")
    header = b"P6\n64 48\n255\n"
    p = subprocess.run(common + ["--ppm", "f.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Encode kernel (ms)" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    r = Renderer(HostScene.builtin())
    rgb = r.render(W, H, depth)
    assert (tmp_path / "f.ppm").read_bytes() == header + image_ref.encode(rgb, T).tobytes()
    assert not (tmp_path / "raytracer_screen.txt").exists()
    p = subprocess.run(common + ["--ppm", "e.ppm", "--exposure", "0.25"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    assert (tmp_path / "e.ppm").read_bytes() == header + image_ref.encode(rgb, T, exposure=0.25).tobytes()
    # --denoise 2 (sigma 1.0, 3 squarings): the reference filter of the G-buffer frame, then the reference encode
    p = subprocess.run(common + ["--ppm", "d.ppm", "--denoise", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    rgb_g, hits = r.render_gbuffer(W, H, depth)
    want = image_ref.encode(denoise_ref.denoise(rgb_g, hits, 2, 1.0, 3), T)
    assert (tmp_path / "d.ppm").read_bytes() == header + want.tobytes()
    assert want.tobytes() != image_ref.encode(rgb, T).tobytes()
