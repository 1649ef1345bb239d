"""The thin-lens camera (include/rt_capi_lens.h) without a GPU: the header, the exported symbols, the struct sizes, every
argument check in the header's order (none touches a device), lens_ref -- the tests' restatement of the definition -- on its own,
the conditions on the oracle frames the GPU tests compare, and the executable's --lens usage."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_frames
import cameras
import lens_ref
import rays_ref
from tilecoderaytracer_amd import HostScene, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_capi_lens.h")
EXE = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
FUNCTIONS = ["rt_capi_lens_version", "rt_get_lens_info", "rt_lens_rays", "rt_lens_rays_device", "rt_render_lens",
             "rt_render_lens_device"]
F = np.float32


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t|const char \*)\s*(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    assert '#include "rt_capi_rays.h"' in text
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    assert int(re.search(r"#define RT_CAPI_LENS_VERSION (\d+)", text).group(1)) == lib.rt_capi_lens_version() == 1


def test_the_other_headers_versions_are_unchanged():
    lib = capi.load_library()
    assert (lib.rt_capi_version(), lib.rt_capi_tuning_version(), lib.rt_capi_ssaa_version(), lib.rt_capi_rays_version(),
            lib.rt_capi_query_version(), lib.rt_capi_gbuffer_version(), lib.rt_capi_texture_version(),
            lib.rt_capi_refract_version(), lib.rt_capi_soft_version(), lib.rt_capi_denoise_version(),
            lib.rt_capi_image_version(), lib.rt_capi_ao_version(), lib.rt_capi_launch_version(),
            lib.rt_capi_adaptive_version()) == (4,) + (1,) * 13


def test_struct_sizes_match_the_header(tmp_path):
    assert C.sizeof(capi.RtLensParams) == 20
    assert C.sizeof(capi.RtLensInfo) == 48 and capi.RtLensInfo.chunks.offset == 16 and capi.RtLensInfo.raygen_ms.offset == 24
    if not shutil.which("gcc"):
        return
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_capi_lens.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d\\n", (int)sizeof(rt_lens_params), (int)sizeof(rt_lens_info),\n'
                   "  (int)offsetof(rt_lens_info, chunks), (int)offsetof(rt_lens_info, raygen_ms),\n"
                   "  (int)offsetof(rt_lens_info, resolve_ms), (int)offsetof(rt_lens_params, focus)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(capi.RtLensParams), C.sizeof(capi.RtLensInfo), capi.RtLensInfo.chunks.offset,
                                     capi.RtLensInfo.raygen_ms.offset, capi.RtLensInfo.resolve_ms.offset,
                                     capi.RtLensParams.focus.offset]


def test_header_is_plain_c99_with_every_other_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    headers = sorted(h for h in os.listdir(INCLUDE) if h.endswith(".h"))
    assert "rt_capi_lens.h" in headers and len(headers) >= 15
    src = tmp_path / "lens.c"
    src.write_text('#include "rt_capi_lens.h"\n' + "".join(f'#include "{h}"\n' for h in headers) +
                   "int main(void) { rt_lens_params p = {4, 0, 7u, 0.25f, 8.0f}; rt_lens_info i; (void)i;\n"
                   "  return (RT_CAPI_LENS_VERSION == 1 && sizeof p == 20 && p.samples == 4) ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_gained_two_kernels_and_no_render_kernel():
    """the new kernels are rt_lens_*, neither of them a render kernel, and the catalogue of rt_tables.h does not name them"""
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    names = [line.split()[-1] for line in r.stdout.splitlines() if line.split()]
    for kernel in ("rt_lens_raygen_kernel", "rt_lens_resolve_kernel"):
        assert any(kernel in n and "__device_stub__" not in n for n in names), kernel
    render = [n for n in names if "rt_render_kernel" in n and "__device_stub__" not in n]
    assert len(render) == 117 and not [n for n in render if "lens" in n]
    assert not [n for n in names if "rt_ao_kernel" in n and "lens" in n]
    assert "lens" not in open(os.path.join(ROOT, "tilecoderaytracer_amd", "csrc", "rt_tables.h")).read()


# ---- 2. the argument checks, in the header's order, without a device ---------------------------------------------------------

GOOD = (2, 0, 0, 0.25, 8.0)             # samples, chunk_columns, seed, aperture, focus
NAN, INF = float("nan"), float("inf")
BAD_PARAMS = [((0, 0, 0, 0.25, 8.0), "samples"), ((9, 0, 0, 0.25, 8.0), "samples"), ((-1, 0, 0, 0.25, 8.0), "samples"),
              ((2, -1, 0, 0.25, 8.0), "chunk_columns"),
              ((2, 0, 0, -0.5, 8.0), "aperture"), ((2, 0, 0, NAN, 8.0), "aperture"), ((2, 0, 0, INF, 8.0), "aperture"),
              ((2, 0, 0, 0.25, 0.0), "focus"), ((2, 0, 0, 0.25, -1.0), "focus"), ((2, 0, 0, 0.25, NAN), "focus"),
              ((2, 0, 0, 0.25, INF), "focus")]
ORDER = ["samples", "chunk_columns", "aperture", "focus"]
WORST = {"samples": 9, "chunk_columns": -2, "aperture": -1.0, "focus": 0.0}
FIELD = {"samples": 0, "chunk_columns": 1, "aperture": 3, "focus": 4}


def params_bad_from(first):
    """GOOD with every field of ORDER from `first` on bad"""
    values = list(GOOD)
    for name in ORDER[first:]:
        values[FIELD[name]] = WORST[name]
    return capi.RtLensParams(*values)


def _rays_call(cam, W, H, x0, x1, params, out, device=False):
    lib = capi.load_library()
    ptr = (out if isinstance(out, int) else out.ctypes.data) if out is not None else None
    p = C.byref(params) if params is not None else None
    c = C.byref(cam) if cam is not None else None
    if device:
        rc = lib.rt_lens_rays_device(c, W, H, x0, x1, p, 0, ptr, None)
    else:
        rc = lib.rt_lens_rays(c, W, H, x0, x1, p, 0, ptr)
    return rc, lib.rt_last_error().decode()


def test_every_argument_check_of_the_ray_generation_comes_before_the_device_in_the_headers_order(have_gpu):
    """each bad argument alone is RT_ERR_INVALID with its message; a bad argument together with every later one is still reported
    as the earlier one; the valid call reaches the device question -- RT_ERR_NO_DEVICE on a machine without one"""
    P = capi.RtLensParams
    cam = lens_ref.camera_copy(HostScene.builtin())
    out = np.zeros((4, 3, 4, 6), F)
    worst = params_bad_from(0)
    for device in (False, True):
        ptr = 0x10002 if device else out                                   # (misaligned: the last check before the device)
        # (1) rt_render's, in rt_render's order, everything later bad as well
        for (W, H, x0, x1), word in (((0, 3, 0, 0), "W,H > 0"), ((4, 0, 0, 4), "W,H > 0"), ((4, 3, -1, 4), "x0 <= x1"),
                                     ((4, 3, 0, 5), "x0 <= x1"), ((4, 3, 3, 2), "x0 <= x1")):
            rc, msg = _rays_call(None, W, H, x0, x1, worst, None, device)
            assert rc == capi.RT_ERR_INVALID and word in msg, (W, H, x0, x1, msg)
        rc, msg = _rays_call(None, 4, 3, 0, 4, worst, None, device)
        assert rc == capi.RT_ERR_INVALID and "NULL" in msg and "camera" not in msg            # the output before the camera
        rc, msg = _rays_call(None, 4, 3, 0, 4, worst, ptr, device)
        assert rc == capi.RT_ERR_INVALID and "camera" in msg
        # (2) .. (6)
        rc, msg = _rays_call(cam, 4, 3, 0, 4, None, ptr, device)
        assert rc == capi.RT_ERR_INVALID and "params" in msg
        for bad, word in BAD_PARAMS:
            rc, msg = _rays_call(cam, 4, 3, 0, 4, P(*bad), ptr, device)
            assert rc == capi.RT_ERR_INVALID and word in msg, (bad, msg)
        for first, word in enumerate(ORDER):
            rc, msg = _rays_call(cam, 1 << 30, 3, 0, 1, params_bad_from(first), ptr, device)     # (7) fails too
            assert rc == capi.RT_ERR_INVALID and word in msg, (first, msg)
        # (7) the virtual size, then the strip's rays, then the alignment
        for W, H in ((1 << 30, 3), (3, 1 << 30)):
            rc, msg = _rays_call(cam, W, H, 0, 1, P(*GOOD), ptr, device)
            assert rc == capi.RT_ERR_INVALID and "2^31" in msg, (W, H, msg)
        rc, msg = _rays_call(cam, 1 << 15, 1 << 15, 0, 1 << 15, P(8, 0, 0, 0.25, 8.0), ptr, device)   # 2^36 rays
        assert rc == capi.RT_ERR_INVALID and "rays" in msg
    rc, msg = _rays_call(cam, 4, 3, 0, 4, P(*GOOD), 0x10002, True)
    assert rc == capi.RT_ERR_INVALID and "4-byte" in msg
    assert _rays_call(cam, 4, 3, 2, 2, P(*GOOD), None)[0] in (capi.RT_OK, capi.RT_ERR_NO_DEVICE)   # an empty strip needs no output
    if have_gpu:
        return
    assert _rays_call(cam, 4, 3, 0, 4, P(*GOOD), out)[0] == capi.RT_ERR_NO_DEVICE
    assert _rays_call(cam, 4, 3, 0, 4, P(*GOOD), 0x10000, True)[0] == capi.RT_ERR_NO_DEVICE
    for ends in ((1, 0, 0, 0.0, 1e-30), (8, 2 ** 31 - 1, 2 ** 32 - 1, 3.0e38, 3.0e38)):              # the ranges' ends are valid
        assert _rays_call(cam, 4, 3, 0, 1, P(*ends), np.zeros((3, 64, 6), F))[0] == capi.RT_ERR_NO_DEVICE, ends


def test_a_render_without_a_scene_is_rt_renders_failure():
    """rt_render's checks come first: whatever else is wrong, a NULL scene is reported as rt_render reports it, and
    rt_get_lens_info refuses NULL"""
    lib = capi.load_library()
    out = np.zeros((4, 4, 3), F)
    assert lib.rt_render(None, None, 4, 4, 0, 4, 1, out.ctypes.data) == capi.RT_ERR_INVALID
    want = lib.rt_last_error().decode()
    for params in (None, params_bad_from(0), capi.RtLensParams(*GOOD)):
        p = C.byref(params) if params is not None else None
        assert lib.rt_render_lens(None, None, 4, 4, 0, 4, 1, p, out.ctypes.data) == capi.RT_ERR_INVALID
        assert lib.rt_last_error().decode() == want == "scene is NULL"
        assert lib.rt_render_lens_device(None, None, 4, 4, 0, 4, 1, p, 0x10002, None) == capi.RT_ERR_INVALID
        assert lib.rt_last_error().decode() == want
    assert lib.rt_get_lens_info(None, C.byref(capi.RtLensInfo())) == capi.RT_ERR_INVALID


# ---- 3. lens_ref on its own ----------------------------------------------------------------------------------------------------

def some_cameras():
    cat = cameras.catalogue("builtin")
    return [lens_ref.camera_copy(HostScene.builtin()), cat["pitched_down"], cat["rolled_1p45"], cat["left_handed"]]


@pytest.mark.parametrize("n", [1, 2, 4])
def test_a_pinhole_focused_on_the_screen_traces_the_virtual_frames_rays(n):
    W, H = 61, 37
    for cam in some_cameras():
        got = lens_ref.rays(cam, W, H, 0, W, n, 12345, 0.0, 1.0)
        virtual = rays_ref.camera_rays(cam, n * W, n * H)                  # [n x + i, n z + j] -> [x, z, i n + j]
        want = virtual.reshape(W, n, H, n, 6).transpose(0, 2, 1, 3, 4).reshape(W, H, n * n, 6)
        assert np.array_equal(rays_ref.positive_zeros(got).view(np.uint32), rays_ref.positive_zeros(want).view(np.uint32))
        assert np.array_equal(got[..., :3].view(np.uint32), want[..., :3].view(np.uint32))      # the eye itself


@pytest.mark.parametrize("n", [3, 8])
def test_each_pixels_lens_strata_are_occupied_exactly_once(n):
    W, H, S = 61, 37, n * n
    for seed in (0, 0xDEADBEEF):
        h, sp = lens_ref.strata(W, H, 0, W, n, seed)
        assert sp.shape == (W, H, S) and np.array_equal(np.sort(sp, axis=-1), np.broadcast_to(np.arange(S), (W, H, S)))
        assert len(np.unique(sp[..., 0])) == S                             # the rotation differs between pixels
        u, v = lens_ref.lens_points(W, H, 0, W, n, seed)
        # the sample lies in its stratum's image: its square coordinates (a, b) fall in cell (li, lj)
        r2 = u.astype(np.float64) ** 2 + v.astype(np.float64) ** 2
        assert r2.max() <= 1.0 + 2.0 ** -23, r2.max()                      # u^2 + v^2 <= 1 up to one ulp


def test_the_lens_points_lie_on_the_lens_and_the_targets_on_the_focal_plane():
    W, H, n, aperture, focus = 61, 37, 4, 0.37, 7.3
    for cam in some_cameras():
        rays = lens_ref.rays(cam, W, H, 0, W, n, 3, aperture, focus).astype(np.float64)
        eye, so = (np.array(list(v), np.float64) for v in (cam.eye_origin, cam.screen_origin))
        ch, cv = (np.array(list(v), np.float64) for v in (cam.vector_horizontal, cam.vector_vertical))
        off = rays[..., :3] - eye
        u, v = off @ ch / aperture, off @ cv / aperture                    # (orthonormal screen vectors)
        assert (u * u + v * v).max() <= 1.0 + 1e-5 and np.abs(off @ (so - eye)).max() < 1e-5
        assert 0.2 < (u * u + v * v).mean() < 0.8                          # spread over the disc, not collapsed
        axis = (so - eye) / np.linalg.norm(so - eye)
        depth = (rays[..., 3:] - eye) @ axis
        assert np.abs(depth / (focus * np.linalg.norm(so - eye)) - 1.0).max() < 1e-5


def test_strips_of_the_reference_concatenate_to_the_frame():
    W, H = 61, 37
    cam = cameras.catalogue("builtin")["pitched_down"]
    for n in (2, 3):
        whole = lens_ref.rays(cam, W, H, 0, W, n, 9, 0.3, 5.0)
        parts = [lens_ref.rays(cam, W, H, x0, x1, n, 9, 0.3, 5.0) for x0, x1 in ((0, 20), (20, 21), (21, 61))]
        assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
        assert whole.shape == (W, H, n * n, 6)


def test_resolve_sums_in_order():
    big, one = F(2.0 ** 24), F(1.0)
    colours = np.zeros((1, 4, 3), F)
    colours[0, :, 0] = (big, one, one, one)          # ((2^24 + 1) + 1) + 1 = 2^24 in fp32; any pairwise order gives more
    colours[0, :, 1] = (one, one, one, big)          # ((1 + 1) + 1) + 2^24 = 2^24 + 4 (3 rounds up to even)
    out = lens_ref.resolve(colours, 2)
    assert out.dtype == F and out[0, 0] == big / F(4.0) and out[0, 1] == (F(3.0) + big) / F(4.0)


# ---- 4. the oracle frames the GPU tests compare ----------------------------------------------------------------------------------

@pytest.mark.parametrize("key,W,H,depth,n,seed,point", lens_ref.FRAMES)
def test_the_compared_frames_are_not_pinhole_frames(key, W, H, depth, n, seed, point):
    """a lens frame must not pass by being a pinhole frame: each holds at least 200 distinct colours and differs from the
    aperture-0 frame of the same focus in at least 5 % of its pixels"""
    aperture, focus = lens_ref.lens_of(key, point)
    assert aperture > 0 and focus > 1
    frame = lens_ref.oracle_frame(key, W, H, depth, n, seed, aperture, focus)
    pinhole = lens_ref.oracle_frame(key, W, H, depth, n, seed, 0.0, focus)
    assert frame.shape == (W, H, 3) and np.isfinite(frame).all()
    assert lens_ref.distinct_colours(frame) >= 200, lens_ref.distinct_colours(frame)
    assert lens_ref.changed_share(frame, pinhole) >= 0.05, lens_ref.changed_share(frame, pinhole)
    so = np.array(list(adaptive_frames.host_scene(key).camera.contents.screen_origin), dtype=F)
    assert not (np.signbit(so) & (so == 0)).any(), so


# ---- 5. the executable refuses bad --lens values before any device work ------------------------------------------------------------

@pytest.mark.parametrize("args", [["--lens", "0"], ["--lens", "9"], ["--lens", "2:-1"], ["--lens", "2:x"], ["--lens", "2:0.1:0"],
                                  ["--lens", "2:0.1:nan"], ["--lens", "2:inf:2"], ["--lens", "2:0.1:2:-3"],
                                  ["--lens", "2:0.1:2:4294967296"], ["--lens", "2:0.1:2:3:4"], ["--lens", "2:"], ["--lens"],
                                  ["--lens", "2:0.1:2", "--ssaa", "2"], ["--lens", "2:0.1:2", "--adaptive", "2"],
                                  ["--lens", "2:0.1:2", "--gpus", "2"], ["--lens", "2:0.1:2", "--hits", "hits.bin"]])
def test_the_executable_refuses_bad_lens_values_with_a_usage_error(args, tmp_path):
    r = subprocess.run([EXE, "--width", "8", "--height", "8", "--no-txt"] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "usage:" in r.stderr and "--lens" in r.stderr, (args, r.stderr)
    assert "Start Ray Tracing" not in r.stdout and not os.listdir(tmp_path)
