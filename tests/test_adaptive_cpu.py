"""Adaptive supersampling (include/rt_capi_adaptive.h) without a GPU: the header, the exported symbols, the struct sizes, every
argument check in the header's order (none touches a device), adaptive_ref -- the tests' restatement of FLAGS -- on hand-built
rectangles, one per clause, the share condition of the frames the GPU tests compare, and the executable's --adaptive usage."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_frames
import adaptive_ref
from tilecoderaytracer_amd import capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_capi_adaptive.h")
EXE = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
FUNCTIONS = ["rt_adaptive_flags", "rt_adaptive_flags_device", "rt_capi_adaptive_version", "rt_get_adaptive_info",
             "rt_render_adaptive", "rt_render_adaptive_device"]
F = np.float32


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t|const char \*)\s*(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    assert '#include "rt_capi_gbuffer.h"' in text
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    assert int(re.search(r"#define RT_CAPI_ADAPTIVE_VERSION (\d+)", text).group(1)) == lib.rt_capi_adaptive_version() == 1


def test_the_other_headers_versions_are_unchanged():
    lib = capi.load_library()
    assert (lib.rt_capi_version(), lib.rt_capi_tuning_version(), lib.rt_capi_ssaa_version(), lib.rt_capi_rays_version(),
            lib.rt_capi_query_version(), lib.rt_capi_gbuffer_version(), lib.rt_capi_texture_version(),
            lib.rt_capi_refract_version(), lib.rt_capi_soft_version(), lib.rt_capi_denoise_version(),
            lib.rt_capi_image_version(), lib.rt_capi_ao_version(), lib.rt_capi_launch_version()) == (4,) + (1,) * 12


def test_struct_sizes_match_the_header(tmp_path):
    assert C.sizeof(capi.RtAdaptiveParams) == 20
    assert C.sizeof(capi.RtAdaptiveInfo) == 64 and capi.RtAdaptiveInfo.first_pass_ms.offset == 32
    if not shutil.which("gcc"):
        return
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_capi_adaptive.h"\n'
                   'int main(void) { printf("%d %d %d %d\\n", (int)sizeof(rt_adaptive_params), (int)sizeof(rt_adaptive_info),\n'
                   "  (int)offsetof(rt_adaptive_info, chunks), (int)offsetof(rt_adaptive_info, first_pass_ms)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(capi.RtAdaptiveParams), C.sizeof(capi.RtAdaptiveInfo),
                                     capi.RtAdaptiveInfo.chunks.offset, capi.RtAdaptiveInfo.first_pass_ms.offset]


def test_header_is_plain_c99_with_every_other_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    headers = sorted(h for h in os.listdir(INCLUDE) if h.endswith(".h"))
    assert "rt_capi_adaptive.h" in headers and len(headers) >= 14
    src = tmp_path / "adaptive.c"
    src.write_text('#include "rt_capi_adaptive.h"\n' + "".join(f'#include "{h}"\n' for h in headers) +
                   "int main(void) { rt_adaptive_params p = {2, 0, 0, 0.03125f, 0.9f}; rt_adaptive_info i; rt_hit h; (void)h; (void)i;\n"
                   "  return (RT_CAPI_ADAPTIVE_VERSION == 1 && sizeof p == 20 && p.samples == 2) ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_gained_no_render_kernel():
    """the new kernels are rt_adaptive_*, none of them a render kernel, and the catalogue of rt_tables.h does not name them"""
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    names = [line.split()[-1] for line in r.stdout.splitlines() if line.split()]
    for kernel in ("rt_adaptive_flag_kernel", "rt_adaptive_scan_kernel", "rt_adaptive_list_kernel", "rt_adaptive_resolve_kernel"):
        assert any(kernel in n for n in names), kernel
    assert not [n for n in names if n.startswith("rt_render_kernel") and "adaptive" in n]
    assert "adaptive" not in open(os.path.join(ROOT, "tilecoderaytracer_amd", "csrc", "rt_tables.h")).read()


# ---- 2. the argument checks, in the header's order, without a device ---------------------------------------------------------

GOOD = (2, 0, 0, 1 / 32, 0.9)
BAD_PARAMS = [((3, 0, 0, 1 / 32, 0.9), "samples"), ((0, 0, 0, 1 / 32, 0.9), "samples"), ((8, 0, 0, 1 / 32, 0.9), "samples"),
              ((2, 2, 0, 1 / 32, 0.9), "flag_all"), ((2, -1, 0, 1 / 32, 0.9), "flag_all"),
              ((2, 0, -1, 1 / 32, 0.9), "chunk_pixels"),
              ((2, 0, 0, -0.5, 0.9), "color_threshold"), ((2, 0, 0, float("nan"), 0.9), "color_threshold"),
              ((2, 0, 0, float("inf"), 0.9), "color_threshold"),
              ((2, 0, 0, 1 / 32, float("nan")), "normal_cos"), ((2, 0, 0, 1 / 32, 1.5), "normal_cos"),
              ((2, 0, 0, 1 / 32, -1.25), "normal_cos")]


def _flags_call(params, Wn, H, rgb, hits, out, device=False):
    lib = capi.load_library()
    ptr = lambda a: (a if isinstance(a, int) else a.ctypes.data) if a is not None else None
    p = C.byref(params) if params is not None else None
    if device:
        rc = lib.rt_adaptive_flags_device(0, p, Wn, H, ptr(rgb), ptr(hits), ptr(out), None)
    else:
        rc = lib.rt_adaptive_flags(0, p, Wn, H, ptr(rgb), ptr(hits), ptr(out))
    return rc, lib.rt_last_error().decode()


def test_every_argument_check_of_the_flag_pass_comes_before_the_device_in_the_headers_order(have_gpu):
    """each bad argument alone is RT_ERR_INVALID with its message; a bad argument together with every later one is still reported
    as the earlier one; the valid call reaches the device question -- RT_ERR_NO_DEVICE on a machine without one"""
    P = capi.RtAdaptiveParams
    rgb, hits, out = np.zeros((4, 3, 3), F), np.zeros((4, 3), HIT_DTYPE), np.zeros((4, 3), np.uint8)
    for device in (False, True):
        rc, msg = _flags_call(None, 0, 0, None, None, None, device)
        assert rc == capi.RT_ERR_INVALID and "params" in msg
        for bad, word in BAD_PARAMS:
            rc, msg = _flags_call(P(*bad), 0, 0, None, None, None, device)      # (the later checks would fail too)
            assert rc == capi.RT_ERR_INVALID and word in msg, (bad, msg)
    order = ["samples", "flag_all", "chunk_pixels", "color_threshold", "normal_cos"]
    worst = [3, 5, -2, -1.0, 7.0]
    for first in range(len(order)):                                             # every field from `first` on is bad
        values = list(GOOD[:first]) + worst[first:]
        rc, msg = _flags_call(P(*values), 0, 0, None, None, None)
        assert rc == capi.RT_ERR_INVALID and order[first] in msg, (values, msg)
    for Wn, H in ((0, 3), (4, 0), (-1, 3), (4, -2)):
        rc, msg = _flags_call(P(*GOOD), Wn, H, None, None, None)
        assert rc == capi.RT_ERR_INVALID and "Wn, H" in msg, (Wn, H, msg)
    rc, msg = _flags_call(P(*GOOD), 1 << 15, 1 << 15, None, None, None)         # 2^30 pixels > 533 333 333
    assert rc == capi.RT_ERR_INVALID and "too large" in msg
    assert "NULL" in _flags_call(P(*GOOD), 533333333, 1, None, None, None)[1]   # the limit itself is allowed
    assert "too large" in _flags_call(P(*GOOD), 533333334, 1, None, None, None)[1]
    for missing in range(3):
        args = [rgb, hits, out]
        args[missing] = None
        rc, msg = _flags_call(P(*GOOD), 4, 3, *args)
        assert rc == capi.RT_ERR_INVALID and "NULL" in msg, missing
    A, HITS, OUT = 0x10000, 0x40000, 0x50000                                    # fake addresses, never dereferenced
    rc, msg = _flags_call(P(*GOOD), 4, 3, A + 2, HITS + 8, OUT, True)           # records before colours
    assert rc == capi.RT_ERR_INVALID and "16-byte" in msg
    rc, msg = _flags_call(P(*GOOD), 4, 3, A + 2, HITS, OUT + 1, True)
    assert rc == capi.RT_ERR_INVALID and "4-byte" in msg
    if have_gpu:
        return
    assert _flags_call(P(*GOOD), 4, 3, rgb, hits, out)[0] == capi.RT_ERR_NO_DEVICE
    assert _flags_call(P(*GOOD), 4, 3, A, HITS, OUT + 1, True)[0] == capi.RT_ERR_NO_DEVICE      # the flags need no alignment
    for ends in ((1, 1, 0, 0.0, -1.0), (4, 0, 2 ** 31 - 1, 3.0e38, 1.0)):        # the ranges' ends are valid
        assert _flags_call(P(*ends), 1, 1, rgb, hits, out)[0] == capi.RT_ERR_NO_DEVICE, ends


def test_a_render_without_a_scene_is_rt_renders_failure():
    """rt_render's checks come first: whatever else is wrong, a NULL scene is reported as rt_render reports it, and
    rt_get_adaptive_info refuses NULL"""
    lib = capi.load_library()
    out = np.zeros((4, 4, 3), F)
    assert lib.rt_render(None, None, 4, 4, 0, 4, 1, out.ctypes.data) == capi.RT_ERR_INVALID
    want = lib.rt_last_error().decode()
    for params in (None, capi.RtAdaptiveParams(3, 5, -2, -1.0, 7.0), capi.RtAdaptiveParams(*GOOD)):
        p = C.byref(params) if params is not None else None
        assert lib.rt_render_adaptive(None, None, 4, 4, 0, 4, 1, p, out.ctypes.data, None) == capi.RT_ERR_INVALID
        assert lib.rt_last_error().decode() == want == "scene is NULL"
        assert lib.rt_render_adaptive_device(None, None, 4, 4, 0, 4, 1, p, 0x10002, None, None) == capi.RT_ERR_INVALID
        assert lib.rt_last_error().decode() == want
    assert lib.rt_get_adaptive_info(None, C.byref(capi.RtAdaptiveInfo())) == capi.RT_ERR_INVALID


# ---- 3. adaptive_ref on hand-built rectangles: every clause of FLAGS ------------------------------------------------------------

def rect(Wn, H, obj=3, normal=(0.0, 0.0, 1.0), colour=(0.5, 0.5, 0.5)):
    rgb = np.empty((Wn, H, 3), F)
    rgb[...] = np.asarray(colour, F)
    hits = np.zeros((Wn, H), HIT_DTYPE)
    hits["object"] = obj
    hits["normal"] = np.asarray(normal, F)
    return rgb, hits


ONLY = dict(color_threshold=1e30, normal_cos=-1.0)      # neither the colours nor the normals can flag (short of a NaN)


def footprint(x, z, Wn, H):
    """the pixels whose footprint has (x, z) as another corner, and (x, z) itself is not among them unless it differs from
    its own neighbours: (x-1, z), (x, z-1), (x-1, z-1)"""
    out = np.zeros((Wn, H), bool)
    for a, b in ((x - 1, z), (x, z - 1), (x - 1, z - 1)):
        if a >= 0 and b >= 0:
            out[a, b] = True
    return out


def clause_rectangles():
    """name -> (rgb, hits, keywords, the expected flags): the hand-built rectangles, shared with the GPU test"""
    cases = {}
    rgb, hits = rect(5, 4)
    cases["uniform"] = (rgb, hits, {}, np.zeros((5, 4), bool))
    rgb, hits = rect(5, 4)
    hits["object"][2, 2] = 7
    want = footprint(2, 2, 5, 4)
    want[2, 2] = True                                    # (its own neighbours differ from it as well)
    cases["an object change"] = (rgb, hits, ONLY, want)
    rgb, hits = rect(5, 4, obj=-1, normal=(0.0, 0.0, 0.0))
    cases["a miss beside a miss: no normal test"] = (rgb, hits, dict(color_threshold=1e30, normal_cos=1.0), np.zeros((5, 4), bool))
    rgb, hits = rect(5, 4, normal=(0.0, 0.0, 0.0))       # a hit with that normal: t = 0 < 1 flags wherever a neighbour exists
    want = np.ones((5, 4), bool)
    want[4, 3] = False
    cases["a hit beside a hit: the normal test"] = (rgb, hits, dict(color_threshold=1e30, normal_cos=1.0), want)
    c = F(0.75)                                          # t = 0.75 exactly against normal (0, 0, 1)
    rgb, hits = rect(5, 4)
    hits["normal"][2, 2] = (F(0.5), F(0.25), c)
    cases["a normal exactly at the threshold"] = (rgb, hits, dict(color_threshold=1e30, normal_cos=float(c)), np.zeros((5, 4), bool))
    want = footprint(2, 2, 5, 4)
    want[2, 2] = True
    cases["a normal one ulp below the threshold"] = (rgb, hits, dict(color_threshold=1e30, normal_cos=float(np.nextafter(c, F(1)))),
                                                     want)
    thr = F(1 / 32)
    rgb, hits = rect(5, 4, colour=(0.5, 0.5, 0.5))
    rgb[2, 2, 1] = F(0.5) + thr                          # exact: both are multiples of 2^-5
    cases["a colour difference exactly at the threshold"] = (rgb, hits, dict(color_threshold=float(thr), normal_cos=-1.0),
                                                             np.zeros((5, 4), bool))
    rgb, hits = rect(5, 4, colour=(0.5, 0.5, 0.5))
    rgb[2, 2, 1] = np.nextafter(F(0.5) + thr, F(1))
    want = footprint(2, 2, 5, 4)
    want[2, 2] = True
    cases["a colour difference one ulp above"] = (rgb, hits, dict(color_threshold=float(thr), normal_cos=-1.0), want)
    rgb, hits = rect(5, 4)
    hits["normal"][2, 2, 0] = np.nan
    cases["a NaN normal"] = (rgb, hits, ONLY, want)
    rgb, hits = rect(5, 4)
    rgb[2, 2, 2] = np.nan
    cases["a NaN colour"] = (rgb, hits, ONLY, want)
    rgb, hits = rect(5, 4, colour=(np.inf, 0.5, 0.5))    # inf - inf everywhere a neighbour exists
    want = np.ones((5, 4), bool)
    want[4, 3] = False
    cases["inf - inf"] = (rgb, hits, ONLY, want)
    rgb, hits = rect(5, 4)
    hits["object"][4, :] = 9                             # the last column differs: column 3 sees it, column 4 has no (x+1, .)
    want = np.zeros((5, 4), bool)
    want[3, :] = True
    cases["the last column has no neighbour to the right"] = (rgb, hits, ONLY, want)
    rgb, hits = rect(5, 4)
    hits["object"][:, 3] = 9
    want = np.zeros((5, 4), bool)
    want[:, 2] = True
    cases["the last row has no neighbour above"] = (rgb, hits, ONLY, want)
    rgb, hits = rect(1, 1)
    rgb[0, 0, 0] = np.nan                                # no neighbour at all: nothing is compared
    cases["1 x 1"] = (rgb, hits, {}, np.zeros((1, 1), bool))
    cases["1 x 1, flag_all"] = (rgb, hits, dict(flag_all=True), np.ones((1, 1), bool))
    rgb, hits = rect(5, 4)
    cases["flag_all"] = (rgb, hits, dict(flag_all=True), np.ones((5, 4), bool))
    return cases


@pytest.mark.parametrize("name", sorted(clause_rectangles()))
def test_the_reference_on_a_hand_built_rectangle(name):
    rgb, hits, kw, want = clause_rectangles()[name]
    got = adaptive_ref.flags(rgb, hits, **kw)
    assert got.dtype == np.bool_ and np.array_equal(got, want), (name, np.argwhere(got != want).tolist())


def test_expected_frame_keeps_bits():
    flags = np.array([[True, False], [False, True]])
    a = np.full((2, 2, 3), np.nan, F)
    b = np.full((2, 2, 3), -0.0, F)
    out = adaptive_ref.expected_frame(flags, a, b)
    assert np.isnan(out[0, 0]).all() and np.isnan(out[1, 1]).all()
    assert (out[0, 1].view(np.uint32) == 0x80000000).all() and (out[1, 0].view(np.uint32) == 0x80000000).all()


# ---- 4. the share condition of the frames the GPU tests compare ----------------------------------------------------------------

@pytest.mark.parametrize("key,W,H,depth,table", adaptive_frames.FRAMES)
def test_the_compared_frames_hold_flagged_and_unflagged_pixels(key, W, H, depth, table):
    """where(flags, ...) tests both branches only on a frame with both kinds of pixels: the flagged share of each frame at the
    suggested thresholds lies within 5 % .. 75 %, and is the tabulated one"""
    rgb, hits = adaptive_frames.first_pass(key, W, H, depth)
    flags = adaptive_ref.flags(rgb, hits)
    share = adaptive_ref.assert_share(flags, f"{key} {W}x{H} d{depth}")
    assert abs(share - table) < 0.0006, (key, share, table)
    edges = adaptive_ref.flags(rgb, hits, color_threshold=1e30, normal_cos=-1.0)       # object edges only: a subset
    assert not (edges & ~flags).any() and 0.02 <= edges.mean() <= 0.22


# ---- 5. the executable refuses bad --adaptive values before any device work ------------------------------------------------------

@pytest.mark.parametrize("args", [["--adaptive", "3"], ["--adaptive", "0"], ["--adaptive", "2:-1"], ["--adaptive", "2:x"],
                                  ["--adaptive", "2:0.1:2"], ["--adaptive", "2:0.1:0.5:7"], ["--adaptive"],
                                  ["--adaptive", "2", "--ssaa", "2"], ["--adaptive", "2", "--gpus", "2"],
                                  ["--adaptive-mask", "mask.pgm"], ["--adaptive", "2", "--hits", "hits.bin"]])
def test_the_executable_refuses_bad_adaptive_values_with_a_usage_error(args, tmp_path):
    r = subprocess.run([EXE, "--width", "8", "--height", "8", "--no-txt"] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "usage:" in r.stderr and "--adaptive" in r.stderr, (args, r.stderr)
    assert "Start Ray Tracing" not in r.stdout and not os.listdir(tmp_path)
