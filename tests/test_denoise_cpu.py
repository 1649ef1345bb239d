"""The denoiser (include/rt_capi_denoise.h) without a GPU: the header, the exported symbols, every argument check in the header's
order (none touches a device), the properties of denoise_ref -- the tests' restatement of the definition -- and the point of the
feature: a one-sample soft-shadow frame comes closer to the 64-sample frame by filtering, and closer than by a plain blur."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import denoise_ref
import oracle_lib
import query_ref
import soft_ref
from rays_ref import camera_rays
from tilecoderaytracer_amd import capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_capi_denoise.h")
EXE = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
FUNCTIONS = ["rt_capi_denoise_version", "rt_denoise", "rt_denoise_device", "rt_denoise_scratch_bytes"]
F = np.float32


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t)\s+(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    assert '#include "rt_capi_query.h"' in text              # rt_hit comes from there
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    assert int(re.search(r"#define RT_CAPI_DENOISE_VERSION (\d+)", text).group(1)) == lib.rt_capi_denoise_version() == 1
    assert C.sizeof(capi.RtDenoiseParams) == 12


def test_header_is_plain_c99_with_the_other_headers(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "denoise.c"
    src.write_text('#include "rt_capi_denoise.h"\n'
                   '#include "rt_capi.h"\n'
                   '#include "rt_capi_gbuffer.h"\n'
                   '#include "rt_capi_soft.h"\n'
                   "int main(void) { rt_denoise_params p = {2, 3, 1.0f}; rt_hit h; (void)h;\n"
                   "  return (RT_CAPI_DENOISE_VERSION == 1 && sizeof p == 12 && p.iterations == 2) ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_gained_no_render_kernel():
    """the filter's kernels are not render kernels: none of its symbols starts with rt_render_kernel, and the catalogue of
    rt_tables.h does not name it"""
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    names = [line.split()[-1] for line in r.stdout.splitlines() if line.split()]
    assert any("rt_denoise_atrous_kernel" in n for n in names) and any("rt_denoise_pack_kernel" in n for n in names)
    assert not [n for n in names if n.startswith("rt_render_kernel") and "denoise" in n]
    assert "denoise" not in open(os.path.join(ROOT, "tilecoderaytracer_amd", "csrc", "rt_tables.h")).read()


# ---- 2. the argument checks, in the header's order, without a device ---------------------------------------------------------

def _buffers(Wn=4, H=3):
    rgb = np.zeros((Wn, H, 3), dtype=F)
    hits = np.zeros((Wn, H), dtype=HIT_DTYPE)
    return rgb, hits, np.zeros_like(rgb)


def _host_call(params, Wn, H, rgb, hits, out):
    lib = capi.load_library()
    ptr = lambda a: a.ctypes.data if a is not None else None
    rc = lib.rt_denoise(0, C.byref(params) if params is not None else None, Wn, H, ptr(rgb), ptr(hits), ptr(out), None)
    return rc, lib.rt_last_error().decode()


def _device_call(params, Wn, H, d_rgb, d_hits, d_out, d_scratch):
    lib = capi.load_library()
    rc = lib.rt_denoise_device(0, C.byref(params) if params is not None else None, Wn, H, d_rgb, d_hits, d_out, d_scratch, None)
    return rc, lib.rt_last_error().decode()


GOOD = (2, 3, 1.0)
BAD_PARAMS = [((0, 3, 1.0), "iterations"), ((6, 3, 1.0), "iterations"), ((2, -1, 1.0), "squarings"), ((2, 7, 1.0), "squarings"),
              ((2, 3, -0.5), "sigma"), ((2, 3, float("nan")), "sigma"), ((2, 3, float("inf")), "sigma")]


def test_every_argument_check_comes_before_the_device_in_the_headers_order(have_gpu):
    """each bad argument alone is RT_ERR_INVALID with its message; a bad argument together with every later one is still reported
    as the earlier one; the valid call reaches the device question -- RT_ERR_NO_DEVICE on a machine without one"""
    rgb, hits, out = _buffers()
    P = capi.RtDenoiseParams
    rc, msg = _host_call(None, 0, 0, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "params" in msg
    for bad, word in BAD_PARAMS:
        rc, msg = _host_call(P(*bad), 0, 0, None, None, None)          # (the later checks would fail too)
        assert rc == capi.RT_ERR_INVALID and word in msg, (bad, msg)
        rc, msg = _device_call(P(*bad), 0, 0, None, None, None, None)
        assert rc == capi.RT_ERR_INVALID and word in msg, (bad, msg)
    rc, msg = _host_call(P(0, 9, -1.0), 4, 3, rgb, hits, out)           # iterations before squarings before sigma
    assert rc == capi.RT_ERR_INVALID and "iterations" in msg
    rc, msg = _host_call(P(2, 9, -1.0), 4, 3, rgb, hits, out)
    assert rc == capi.RT_ERR_INVALID and "squarings" in msg
    for Wn, H in ((0, 3), (4, 0), (-1, 3), (4, -2)):
        rc, msg = _host_call(P(*GOOD), Wn, H, None, None, None)
        assert rc == capi.RT_ERR_INVALID and "Wn, H" in msg, (Wn, H, msg)
    rc, msg = _host_call(P(*GOOD), 1 << 15, 1 << 15, None, None, None)   # 2^30 pixels > 533 333 333
    assert rc == capi.RT_ERR_INVALID and "too large" in msg
    assert _host_call(P(*GOOD), 533333333, 1, None, None, None)[1].count("NULL") == 1       # the limit itself is allowed
    assert "too large" in _host_call(P(*GOOD), 533333334, 1, None, None, None)[1]
    for missing in range(3):
        args = [rgb, hits, out]
        args[missing] = None
        rc, msg = _host_call(P(*GOOD), 4, 3, *args)
        assert rc == capi.RT_ERR_INVALID and "NULL" in msg, missing
    # the device variant: fake addresses, never dereferenced -- NULL, then alignment, then overlap
    A, B, S, HITS = 0x10000, 0x20000, 0x30000, 0x40000
    for missing in range(4):
        args = [A, HITS, B, S]
        args[missing] = None
        rc, msg = _device_call(P(*GOOD), 4, 3, *args)
        assert rc == capi.RT_ERR_INVALID and "NULL" in msg, missing
    rc, msg = _device_call(P(*GOOD), 4, 3, A, HITS + 8, A, S)           # misaligned records, and overlapping too
    assert rc == capi.RT_ERR_INVALID and "16-byte" in msg
    rc, msg = _device_call(P(*GOOD), 4, 3, A, HITS, A, S + 4)
    assert rc == capi.RT_ERR_INVALID and "16-byte" in msg
    rc, msg = _device_call(P(*GOOD), 4, 3, A + 2, HITS, A + 2, S)
    assert rc == capi.RT_ERR_INVALID and "4-byte" in msg
    for d_out in (A, A + 4 * 3 * 12 - 4, A - 4 * 3 * 12 + 4):
        rc, msg = _device_call(P(*GOOD), 4, 3, A, HITS, d_out, S)
        assert rc == capi.RT_ERR_INVALID and "overlap" in msg, hex(d_out)
    lib = capi.load_library()
    assert lib.rt_denoise_scratch_bytes(None, 4, 3) == 0 and lib.rt_denoise_scratch_bytes(C.byref(P(0, 3, 1.0)), 4, 3) == 0
    one = lib.rt_denoise_scratch_bytes(C.byref(P(1, 3, 1.0)), 100, 100)
    two = lib.rt_denoise_scratch_bytes(C.byref(P(2, 3, 1.0)), 100, 100)
    assert 32 * 10000 <= one < two                            # the packed guide; more than one iteration needs more
    if have_gpu:
        return
    assert _host_call(P(*GOOD), 4, 3, rgb, hits, out)[0] == capi.RT_ERR_NO_DEVICE
    assert _device_call(P(*GOOD), 4, 3, A, HITS, A + 4 * 3 * 12, S)[0] == capi.RT_ERR_NO_DEVICE      # adjacent is not overlapping
    assert _host_call(P(5, 6, 0.0), 1, 1, rgb, hits, out)[0] == capi.RT_ERR_NO_DEVICE               # the ranges' ends are valid
    assert _host_call(P(1, 0, 0.0), 1, 1, rgb, hits, out)[0] == capi.RT_ERR_NO_DEVICE


def test_python_wrapper_refuses_without_a_device(have_gpu):
    if have_gpu:
        pytest.skip("a GPU is present")
    from tilecoderaytracer_amd import RtError, denoise
    rgb, hits, _ = _buffers()
    with pytest.raises(RtError) as e:
        denoise(rgb, hits)
    assert e.value.code == capi.RT_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        denoise(rgb, hits[:2])


def test_executable_refuses_denoise_with_several_gpus_or_supersampling():
    for extra in (["--gpus", "2"], ["--ssaa", "2"]):
        r = subprocess.run([EXE, "--denoise", "2:1.0:3", "--no-txt"] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and "usage" in r.stderr
    for bad in ("0", "6", "2:-1", "2:1.0:7", "x", "2:nan"):
        r = subprocess.run([EXE, "--denoise", bad, "--no-txt"], capture_output=True, text=True)
        assert r.returncode == 1 and "usage" in r.stderr, bad


# ---- 3. denoise_ref: the definition's properties -----------------------------------------------------------------------------

def r32(x):
    """a Python float rounded to fp32 (the exact double product, sum or quotient of two fp32 values rounds to fp32 as the fp32
    operation does)"""
    return float(F(x))


def by_hand(inp, hits, x, z, i, sigma, squarings):
    """pixel (x, z) of iteration i of the header's definition, in Python floats rounded to fp32 step by step"""
    Wn, H = inp.shape[:2]
    h = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    s = 1 << i
    lum = lambda c: r32(r32(r32(0.25 * float(c[0])) + r32(0.5 * float(c[1]))) + r32(0.25 * float(c[2])))
    hp = hits[x, z]
    if hp["object"] < 0 or (hp["flags"] & 2):
        return [float(v) for v in inp[x, z]]
    if sigma > 0:
        sc = r32(r32(sigma) * 2.0 ** -i)
        inv = r32(1.0 / r32(sc * sc))
    acc, wsum = [0.0, 0.0, 0.0], 0.0
    for a in range(-2, 3):
        for b in range(-2, 3):
            xq, zq = x + a * s, z + b * s
            if not (0 <= xq < Wn and 0 <= zq < H):
                continue
            hq = hits[xq, zq]
            if hq["object"] != hp["object"] or hq["color"].tobytes() != hp["color"].tobytes():
                continue
            n_p, n_q = [float(v) for v in hp["normal"]], [float(v) for v in hq["normal"]]
            t = r32(r32(r32(n_p[0] * n_q[0]) + r32(n_p[1] * n_q[1])) + r32(n_p[2] * n_q[2]))
            wn = t if t > 0 else 0.0
            for _ in range(squarings):
                wn = r32(wn * wn)
            w = r32(r32(h[a + 2] * h[b + 2]) * wn)
            if sigma > 0:
                d = r32(lum(inp[xq, zq]) - lum(inp[x, z]))
                u = r32(1.0 - r32(r32(d * d) * inv))
                w = r32(w * (u if u > 0 else 0.0))
            if not w > 0:
                continue
            acc = [r32(acc[c] + r32(w * float(inp[xq, zq, c]))) for c in range(3)]
            wsum = r32(wsum + w)
    return [r32(acc[c] / wsum) for c in range(3)] if wsum > 0 else [float(v) for v in inp[x, z]]


def random_frame(seed, Wn, H, n_objects=3, palette=2, unit_normals=True):
    rng = np.random.default_rng(seed)
    rgb = rng.random((Wn, H, 3), dtype=F)
    hits = np.zeros((Wn, H), dtype=HIT_DTYPE)
    hits["object"] = rng.integers(-1, n_objects, (Wn, H))
    colours = rng.random((palette, 3), dtype=F)
    hits["color"] = colours[rng.integers(0, palette, (Wn, H))]
    n = rng.normal(size=(Wn, H, 3)).astype(F) + F(2.0) * np.array([0, 1, 0], dtype=F)
    hits["normal"] = n / np.linalg.norm(n, axis=-1, keepdims=True).astype(F) if unit_normals else n
    hits["flags"] = rng.integers(0, 4, (Wn, H)) & np.where(rng.random((Wn, H)) < 0.8, 1, 3)
    return rgb, hits


@pytest.mark.parametrize("shape", [(1, 23), (23, 1), (7, 9)])
@pytest.mark.parametrize("sigma, squarings", [(0.0, 0), (0.7, 3)])
def test_ref_equals_the_hand_computation_where_taps_fall_outside(shape, sigma, squarings):
    """a one-column, a one-row and a small frame: every pixel's window leaves the rectangle, and those taps do not exist"""
    Wn, H = shape
    rgb, hits = random_frame(5, Wn, H, n_objects=1, palette=1)
    hits["object"][Wn // 2, H // 2] = -1                     # one miss among them
    cur = rgb
    for i in range(3):
        nxt = denoise_ref.iterate(cur, hits, i, sigma, squarings)
        for x, z in {(0, 0), (Wn - 1, H - 1), (Wn // 2, H // 2), (Wn // 3, H // 3), (0, H - 1), (Wn - 1, 0), (Wn // 2, 0)}:
            want = np.array(by_hand(cur, hits, x, z, i, sigma, squarings), dtype=F)
            assert denoise_ref.same_bits(nxt[x, z], want), (i, x, z, nxt[x, z], want)
        cur = nxt
    assert denoise_ref.same_bits(cur, denoise_ref.denoise(rgb, hits, 3, sigma, squarings))
    inner = (hits["object"] >= 0) & ((hits["flags"] & 2) == 0)
    assert (cur[inner] != rgb[inner]).any()                   # (it did filter)


def test_ref_passes_misses_and_lights_through_bit_for_bit():
    rgb, hits = random_frame(1, 40, 33)
    rgb[3, 4] = [np.nan, np.inf, -0.0]
    rgb[5, 6] = [1e-42, -1e-45, 3e38]
    hits["object"][3, 4] = -1
    hits["flags"][5, 6] |= 2
    out = denoise_ref.denoise(rgb, hits, 3, 1.0, 3)
    passthrough = (hits["object"] < 0) | ((hits["flags"] & 2) != 0)
    assert passthrough.sum() > 100 and (~passthrough).sum() > 100
    assert np.array_equal(out.view(np.uint32)[passthrough], rgb.view(np.uint32)[passthrough])
    assert (out[~passthrough] != rgb[~passthrough]).any()


def test_ref_never_crosses_an_object_or_an_albedo():
    """every neighbour another object, or the same object with another albedo (one bit apart, or +0.0 against -0.0): the frame
    comes back unchanged.  A pixel whose only tap is itself is (w * c) / w with w = 9/64 times its normal and colour weights: two
    roundings, so it equals c within 2^-23 |c| and is bit-equal for most pixels, not all (9 c is not always an fp32 number).
    What is exact: it depends on no other pixel's colour."""
    rng = np.random.default_rng(2)
    Wn, H = 19, 17
    rgb = rng.random((Wn, H, 3), dtype=F) + F(0.01)
    other = rng.random((Wn, H, 3), dtype=F)

    def unchanged(hits, sigma):
        out = denoise_ref.iterate(rgb, hits, 0, sigma, 2)
        assert (np.abs(out.astype(np.float64) - rgb) <= 2.0 ** -23 * rgb).all()
        assert (out.view(np.uint32) == rgb.view(np.uint32)).mean() > 0.8
        for x, z in ((0, 0), (9, 8), (18, 16), (4, 11)):           # with every other pixel's colour replaced: the same bits
            mixed = other.copy()
            mixed[x, z] = rgb[x, z]
            assert denoise_ref.same_bits(denoise_ref.iterate(mixed, hits, 0, sigma, 2)[x, z], out[x, z])
        full = denoise_ref.denoise(rgb, hits, 5, sigma, 2)
        assert (np.abs(full.astype(np.float64) - rgb) <= 5 * 2.0 ** -23 * rgb).all()

    hits = np.zeros((Wn, H), dtype=HIT_DTYPE)
    hits["normal"] = [0, 1, 0]
    hits["color"] = 0.5
    hits["object"] = np.arange(Wn * H).reshape(Wn, H)
    for sigma in (0.0, 1.0):
        unchanged(hits, sigma)
    hits["object"] = 7
    albedo = np.full((Wn, H, 3), 0.5, dtype=F)
    albedo.view(np.uint32)[..., 1] += np.arange(Wn * H, dtype=np.uint32).reshape(Wn, H)      # one ulp apart, each its own
    hits["color"] = albedo
    for sigma in (0.0, 1.0):
        unchanged(hits, sigma)
    hits["color"] = 0.0                                      # a 5-periodic pattern of one -0.0 word: no tap at step 1 matches
    xs, zs = np.meshgrid(np.arange(Wn), np.arange(H), indexing="ij")
    for k in range(5):
        for c in range(3):
            for j in range(5):
                sel = ((xs % 5) == k) & ((zs % 5) == j)
                hits["color"][..., c][sel] = [0.0, -0.0][(k * 5 + j) >> c & 1] if (k * 5 + j) < 8 else F(k * 5 + j)
    assert denoise_ref.same_bits(denoise_ref.iterate(other, hits, 0, 0.0, 0)[2, 2],
                                 np.array(by_hand(other, hits, 2, 2, 0, 0.0, 0), dtype=F))
    out = denoise_ref.iterate(rgb, hits, 0, 0.0, 0)
    assert (np.abs(out.astype(np.float64) - rgb) <= 2.0 ** -23 * rgb).all()


@pytest.mark.parametrize("sigma", [0.0, 1.0])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_ref_a_nan_or_infinite_colour_does_not_spread_beyond_its_pixel(bad, sigma):
    """with the colour term the bad pixel's luminance makes u NaN or -inf: the tap is dropped everywhere, and the bad pixel
    itself has no tap left and keeps its input.  Without the colour term a weight never sees a colour -- there the bad colour
    enters its neighbours' sums as in[q], so the header promises containment for the weights only; this test pins both."""
    rgb, hits = random_frame(3, 21, 21, n_objects=1, palette=1)
    hits["object"], hits["flags"] = 0, 0
    clean = denoise_ref.denoise(rgb, hits, 2, sigma, 2)
    assert np.isfinite(clean).all()
    dirty_in = rgb.copy()
    dirty_in[10, 10, 1] = bad
    dirty = denoise_ref.denoise(dirty_in, hits, 2, sigma, 2)
    changed = ~((dirty.view(np.uint32) == clean.view(np.uint32)).all(axis=-1))
    xs, zs = np.nonzero(changed)
    if sigma > 0:
        assert np.isfinite(np.delete(dirty.reshape(-1, 3), 10 * 21 + 10, axis=0)).all()
        assert denoise_ref.same_bits(dirty[10, 10], dirty_in[10, 10])
        # its neighbours lost one tap (their sums changed) but stay finite; nothing further than the two footprints moved
        assert (abs(xs - 10) <= 6).all() and (abs(zs - 10) <= 6).all()
    else:
        assert not np.isfinite(dirty[10, 10]).all()
        assert (abs(xs - 10) <= 6).all() and (abs(zs - 10) <= 6).all()
        assert np.isfinite(dirty[:, :, [0, 2]]).all()        # the other channels never see it


def test_ref_zero_and_opposed_normals_drop_the_tap():
    rgb, hits = random_frame(4, 9, 9, n_objects=1, palette=1)
    hits["object"], hits["flags"] = 0, 0
    hits["normal"] = 0.0
    assert denoise_ref.same_bits(denoise_ref.denoise(rgb, hits, 2, 0.0, 3), rgb)       # every weight 0: wsum 0, out = in
    hits["normal"] = [0, 1, 0]
    hits["normal"][::2, ::2] = [0, -1, 0]
    out = denoise_ref.denoise(rgb, hits, 1, 0.0, 0)
    flat = hits.copy()
    flat["normal"] = [0, 1, 0]
    assert not denoise_ref.same_bits(out, denoise_ref.denoise(rgb, flat, 1, 0.0, 0))


# ---- 4. quality: what the filter is for ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def soft_frames():
    """the built-in scene, 96 x 96, depth 3, both lights area lights of radius 1.0: A = 1 x 1 samples (seed 1), B = 8 x 8 (seed 2),
    and the camera rays' records"""
    W = H = 96
    o = oracle_lib.OracleScene.builtin()
    lights = [i for i in range(o.object_count) if o.get_object(i).is_light]
    assert len(lights) == 2
    A = soft_ref.render(soft_ref.Scene(o, {k: (1, 1.0) for k in lights}, seed=1), o.cam, W, H, 3)
    B = soft_ref.render(soft_ref.Scene(o, {k: (8, 1.0) for k in lights}, seed=2), o.cam, W, H, 3)
    hits = query_ref.intersect(query_ref.Scene(o), camera_rays(o.cam, W, H))
    return A, B, hits


def test_one_sample_plus_the_filter_comes_6_dB_closer_to_64_samples_and_beats_a_plain_blur():
    """PSNR against the n = 8 frame (peak 1.0, every pixel).  Measured by this test: n = 1 alone 18.25 dB; filtered (2 iterations,
    sigma 1.0, 3 squarings) 27.32 dB, +9.07; the same kernels with every guide term off (one object, one albedo, one normal, sigma
    0) +6.39 dB at 1 iteration and +4.49 dB at 2.  The bound of 6 dB at 2 iterations rejects a no-op (0 dB) and the plain blur
    at 2 iterations; the guided figure must also beat the plain blur at either count."""
    A, B, hits = soft_frames()
    assert np.isfinite(A).all() and np.isfinite(B).all()
    base = denoise_ref.psnr(A, B)
    guided = denoise_ref.denoise(A, hits, 2, 1.0, 3)
    assert np.isfinite(guided).all()
    unguided_hits = np.zeros(hits.shape, dtype=HIT_DTYPE)
    unguided_hits["normal"] = [0, 1, 0]
    blur1 = denoise_ref.psnr(denoise_ref.denoise(A, unguided_hits, 1, 0.0, 0), B)
    blur2 = denoise_ref.psnr(denoise_ref.denoise(A, unguided_hits, 2, 0.0, 0), B)
    got = denoise_ref.psnr(guided, B)
    print(f"PSNR vs n=8: n=1 {base:.2f} dB, guided {got:.2f} dB (+{got - base:.2f}), "
          f"unguided 1 it +{blur1 - base:.2f}, 2 it +{blur2 - base:.2f}")
    assert got >= base + 6.0, (base, got)
    assert got > blur2 and got > blur1, (got, blur1, blur2)
    passthrough = (hits["object"] < 0) | ((hits["flags"] & 2) != 0)
    assert np.array_equal(guided.view(np.uint32)[passthrough], A.view(np.uint32)[passthrough])
