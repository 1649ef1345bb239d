"""G-buffer frames (include/rt_capi_gbuffer.h) without a GPU: the header, the exported symbols, the argument checks that come
before any device is touched -- rt_render's, in rt_render's order, then the records' -- and the executable's --hits option."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tilecoderaytracer_amd import HostScene, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_capi_gbuffer.h")
EXE = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
FUNCTIONS = ["rt_capi_gbuffer_version", "rt_render_gbuffer", "rt_render_gbuffer_device"]


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char \*)\s*(rt_\w+)\s*\(", text, flags=re.M)))


def test_header_declares_exactly_its_functions():
    assert declared_functions(HEADER) == FUNCTIONS
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert text.count("(") == 3                              # three prototypes, one parenthesis each
    assert '#include "rt_capi_query.h"' in text              # rt_hit comes from there


def test_header_is_plain_c99_with_the_other_headers(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "gbuffer.c"
    src.write_text('#include "rt_capi.h"\n'
                   '#include "rt_capi_tuning.h"\n'
                   '#include "rt_capi_ssaa.h"\n'
                   '#include "rt_capi_rays.h"\n'
                   '#include "rt_capi_query.h"\n'
                   '#include "rt_capi_gbuffer.h"\n'
                   '#include "rt_capi_gbuffer.h"\n'                  # (the include guard)
                   "#include <stddef.h>\n"
                   "static int (*const f)(rt_scene *, const rt_camera_desc *, int, int, int, int, int, float *, rt_hit *) =\n"
                   "    rt_render_gbuffer;\n"
                   "static int (*const g)(rt_scene *, const rt_camera_desc *, int, int, int, int, int, void *, void *, void *) =\n"
                   "    rt_render_gbuffer_device;\n"
                   "static int (*const v)(void) = rt_capi_gbuffer_version;\n"
                   "int main(void) { return (RT_CAPI_GBUFFER_VERSION == 1 && RT_CAPI_QUERY_VERSION == 1 && f && g && v) ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_symbols_and_the_version():
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
    macro = int(re.search(r"#define RT_CAPI_GBUFFER_VERSION (\d+)", open(HEADER).read()).group(1))
    assert lib.rt_capi_gbuffer_version() == macro == 1
    assert lib.rt_capi_version() == 4 and lib.rt_capi_tuning_version() == 1 and lib.rt_capi_query_version() == 1


def test_null_scene_fails_as_rt_render_does():
    """Without a GPU no handle exists (test_no_gpu_means_no_render): the call fails with rt_render's code and text."""
    lib = capi.load_library()
    cam = HostScene.builtin().camera
    rgb = np.zeros((8, 8, 3), dtype=np.float32)
    hits = np.zeros((8, 8), dtype=HIT_DTYPE)
    want = lib.rt_render(None, cam, 8, 8, 0, 8, 3, rgb.ctypes.data)
    want_text = lib.rt_last_error()
    assert want == capi.RT_ERR_INVALID
    assert lib.rt_render_gbuffer(None, cam, 8, 8, 0, 8, 3, rgb.ctypes.data, hits.ctypes.data) == want
    assert lib.rt_last_error() == want_text
    assert lib.rt_render_gbuffer(None, cam, 8, 8, 0, 8, 3, rgb.ctypes.data, None) == capi.RT_ERR_INVALID
    assert lib.rt_render_gbuffer(None, None, -1, 0, 5, 2, -1, None, None) == capi.RT_ERR_INVALID    # the scene first
    assert b"scene" in lib.rt_last_error()
    assert lib.rt_render_gbuffer_device(None, cam, 8, 8, 0, 8, 3, None, None, None) == capi.RT_ERR_INVALID
    assert b"scene" in lib.rt_last_error()
    assert not rgb.any() and not hits.view(np.uint8).any()


# Each case fails one check and passes every check before it, so the text names the FIRST failing check.  The handle is a
# stand-in (zeroed memory, never a scene): every check comes before the handle is used, and a failing one returns at once.
def _order_cases(rgb, hits):
    r, h = rgb.ctypes.data, hits.ctypes.data
    return [
        ((0, 8, 0, 8, 3, r, h), b"W,H > 0"),
        ((8, -1, 0, 8, 3, r, h), b"W,H > 0"),
        ((8, 8, 5, 4, 3, r, h), b"x0 <= x1"),
        ((8, 8, 0, 9, 3, r, h), b"x0 <= x1"),
        ((8, 8, -1, 8, 3, r, h), b"x0 <= x1"),
        ((8, 8, 0, 8, -1, None, None), b"out_rgb"),           # out_rgb before the camera, the depth and out_hits
        ((8, 8, 0, 8, -1, r, None), b"max_depth"),            # the depth before out_hits
        ((8, 8, 0, 8, 3, r, None), b"out_hits"),
        ((1 << 30, 8, 0, 1 << 30, 3, r, h), b"strip too large"),                 # rt_render's limit on the colours
        ((1 << 27, 4, 0, 1 << 27, 3, r, h), b"strip too large for its colours and records"),
    ]


def test_checks_come_in_rt_renders_order_before_the_handle_is_used():
    lib = capi.load_library()
    cam = HostScene.builtin().camera
    stand_in = C.create_string_buffer(1 << 20)
    rgb = np.zeros((8, 8, 3), dtype=np.float32)
    hits = np.zeros((8, 8), dtype=HIT_DTYPE)
    for (W, H, x0, x1, depth, r, h), text in _order_cases(rgb, hits):
        assert lib.rt_render_gbuffer(stand_in, cam, W, H, x0, x1, depth, r, h) == capi.RT_ERR_INVALID, (W, H, x0, x1, depth)
        assert text in lib.rt_last_error(), (text, lib.rt_last_error())
        assert lib.rt_render_gbuffer_device(stand_in, cam, W, H, x0, x1, depth, r, h, None) == capi.RT_ERR_INVALID
        assert text in lib.rt_last_error(), (text, lib.rt_last_error())
    # the camera after the strip and out_rgb, before the depth (check_launch_args())
    assert lib.rt_render_gbuffer(stand_in, None, 8, 8, 0, 8, -1, rgb.ctypes.data, None) == capi.RT_ERR_INVALID
    assert b"camera" in lib.rt_last_error()
    # the device variant: the records 16-byte aligned
    assert lib.rt_render_gbuffer_device(stand_in, cam, 8, 8, 0, 8, 3, rgb.ctypes.data, hits.ctypes.data + 4, None) == \
        capi.RT_ERR_INVALID
    assert b"aligned" in lib.rt_last_error()
    assert not rgb.any() and not hits.view(np.uint8).any() and not any(stand_in.raw)


@pytest.mark.parametrize("args", [["--hits", "h.bin", "--gpus", "2"], ["--gpus", "3", "--hits", "h.bin"],
                                  ["--hits", "h.bin", "--ssaa", "2"], ["--ssaa", "4", "--hits", "h.bin"], ["--hits"]])
def test_executable_refuses_hits_it_cannot_give_before_touching_a_device(args, tmp_path):
    r = subprocess.run([EXE, "--width", "16", "--height", "16", *args], capture_output=True, text=True, cwd=tmp_path,
                       timeout=60)
    assert r.returncode == 1
    assert "usage:" in r.stderr and "--ssaa" in r.stderr and "--hits" in r.stderr
    assert r.stdout == ""                                   # nothing rendered, nothing printed
    assert not (tmp_path / "raytracer_screen.txt").exists() and not (tmp_path / "h.bin").exists()
