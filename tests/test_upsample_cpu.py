"""Guided upsampling (include/rt_capi_upsample.h) without a GPU: the header, the exported symbols, every argument check in the
header's order (none touches a device), upsample_ref -- the tests' restatement of the definition -- one clause at a time against
a per-pixel computation in Python floats, the conditions on the frames test_upsample_gpu.py compares, and the executable's usage
errors."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_frames
import indirect_ref
import upsample_ref
from tilecoderaytracer_amd import capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_capi_upsample.h")
EXE = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
FUNCTIONS = ["rt_capi_upsample_version", "rt_subsample_hits", "rt_subsample_hits_device", "rt_upsample_guided",
             "rt_upsample_guided_device"]
F = np.float32

# The frames whose real gather test_upsample_gpu.py upsamples and compares: (key, W, H, depth, scale, normal_squarings,
# sigma_plane, n, seed, gather_depth).  A normal rejects a tap of the pixel's own object only where two visible points of one
# sphere face more than 78 degrees apart (0.2^64 underflows to 0; at 3 squarings only a right angle does), which needs spheres
# about a cell across: of the oracle's scenes at sizes the suite can afford only scale 8 has 50 such pixels.  Counted by
# test_conditions_on_the_compared_frames (pixels with a tap rejected by object / normal / plane; holes; live; distinct colours):
#     builtin 61 x 37    1400 / 52 / 338    443 holes of 2254 live    964 distinct colours
#     random3 61 x 37    1221 / 92 / 324    510 holes of 2257 live   1638 distinct colours
GATHER_FRAMES = [("builtin", 61, 37, 4, 8, 6, 0.02, 2, 0, 1), ("random3", 61, 37, 4, 8, 6, 0.02, 2, 1, 1)]


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t)\s+(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    includes = re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)
    assert includes == ["rt_capi_query.h"]
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    exported = sorted(line.split()[-1] for line in r.stdout.splitlines() if line.split() and line.split()[-2] == "T"
                      and re.fullmatch(r"rt_\w*(upsample|subsample)\w*", line.split()[-1]))
    assert exported == FUNCTIONS                              # and nothing else of this unit
    assert int(re.search(r"#define RT_CAPI_UPSAMPLE_VERSION (\d+)", text).group(1)) == lib.rt_capi_upsample_version() == 1
    assert C.sizeof(capi.RtUpsampleParams) == 28


def test_header_is_plain_c99_with_every_other_header_and_the_struct_is_28_bytes(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    others = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
    assert "rt_capi_upsample.h" in others and len(others) >= 17
    src = tmp_path / "upsample.c"
    src.write_text('#include "rt_capi_upsample.h"\n' + "".join(f'#include "{h}"\n' for h in others) +
                   "#include <stddef.h>\n"
                   "int main(void) { rt_upsample_params p = {4, 3, 3, 0, 1, 0.0f, 0.0f}; rt_hit h; (void)h;\n"
                   "  return (RT_CAPI_UPSAMPLE_VERSION == 1 && sizeof p == 28 && offsetof(rt_upsample_params, sigma_plane) == 20\n"
                   "          && offsetof(rt_upsample_params, dead_value) == 24 && p.scale == 4) ? 0 : 1; }\n")
    exe = tmp_path / "upsample"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0


def test_every_other_headers_version_is_unchanged():
    want = {"": 4, "_tuning": 1, "_launch": 1, "_ssaa": 1, "_rays": 1, "_query": 1, "_gbuffer": 1, "_texture": 1, "_refract": 1,
            "_soft": 1, "_denoise": 1, "_image": 1, "_ao": 1, "_adaptive": 1, "_lens": 1, "_indirect": 1}
    lib = capi.load_library()
    seen = {}
    for name in sorted(os.listdir(INCLUDE)):
        m = re.fullmatch(r"rt_capi(_\w+)?\.h", name)
        if not m or name == "rt_capi_upsample.h":
            continue
        suffix = m.group(1) or ""
        text = open(os.path.join(INCLUDE, name)).read()
        macro = re.search(r"#define RT_CAPI%s_VERSION (\d+)" % suffix.upper(), text)
        assert macro, name
        fn = getattr(lib, "rt_capi%s_version" % suffix)
        fn.restype = C.c_int
        seen[suffix] = int(macro.group(1))
        assert fn() == seen[suffix], name
    assert seen == want


def test_the_library_gained_no_render_kernel():
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    names = [line.split()[-1] for line in r.stdout.splitlines() if line.split()]
    assert any("rt_upsample_kernel" in n for n in names) and any("rt_subsample_kernel" in n for n in names)
    kernels = {n for n in names if n.startswith("rt_render_kernel")}
    assert len(kernels) == 117, len(kernels)
    assert not [n for n in kernels if "upsample" in n or "subsample" in n]
    assert "upsample" not in open(os.path.join(ROOT, "tilecoderaytracer_amd", "csrc", "rt_tables.h")).read()


# ---- 2. the argument checks, in the header's order, without a device ---------------------------------------------------------

P = capi.RtUpsampleParams
GOOD = (4, 3, 3, 0, 1, 0.5, 0.0)
# each bad value with every later field bad too, and the word of the message that names the first
BAD_PARAMS = [((1, 2, 9, 2, 2, -1.0, np.inf), "scale"), ((9, 2, 9, 2, 2, -1.0, np.inf), "scale"),
              ((4, 2, 9, 2, 2, -1.0, np.inf), "channels"), ((4, 0, 9, 2, 2, -1.0, np.inf), "channels"),
              ((4, 3, -1, 2, 2, -1.0, np.inf), "squarings"), ((4, 3, 7, 2, 2, -1.0, np.inf), "squarings"),
              ((4, 3, 3, 2, 2, -1.0, np.inf), "match_color"), ((4, 3, 3, -1, 2, -1.0, np.inf), "match_color"),
              ((4, 3, 3, 1, 2, -1.0, np.inf), "modulate must"), ((4, 1, 3, 1, 1, -1.0, np.inf), "modulate needs"),
              ((4, 3, 3, 1, 1, -1.0, np.inf), "sigma_plane"), ((4, 3, 3, 1, 1, np.nan, np.inf), "sigma_plane"),
              ((4, 3, 3, 1, 1, np.inf, np.inf), "sigma_plane"), ((4, 3, 3, 1, 1, 0.0, np.inf), "dead_value"),
              ((4, 3, 3, 1, 1, 0.0, np.nan), "dead_value")]


def _up(params, Wn, H, hits, lo, base, out, flags, device_call=False):
    lib = capi.load_library()
    ptr = lambda a: (a if isinstance(a, int) else a.ctypes.data) if a is not None else None
    p = C.byref(params) if params is not None else None
    if device_call:
        rc = lib.rt_upsample_guided_device(0, p, Wn, H, ptr(hits), ptr(lo), ptr(base), ptr(out), ptr(flags), None)
    else:
        rc = lib.rt_upsample_guided(0, p, Wn, H, ptr(hits), ptr(lo), ptr(base), ptr(out), ptr(flags), None)
    return rc, lib.rt_last_error().decode()


def _sub(scale, white, Wn, H, hits, out, device_call=False):
    lib = capi.load_library()
    ptr = lambda a: (a if isinstance(a, int) else a.ctypes.data) if a is not None else None
    if device_call:
        rc = lib.rt_subsample_hits_device(0, scale, white, Wn, H, ptr(hits), ptr(out), None)
    else:
        rc = lib.rt_subsample_hits(0, scale, white, Wn, H, ptr(hits), ptr(out))
    return rc, lib.rt_last_error().decode()


def test_every_argument_check_comes_before_the_device_in_the_headers_order(have_gpu):
    INV = capi.RT_ERR_INVALID
    hits = np.zeros((8, 6), dtype=HIT_DTYPE)
    lo, out = np.zeros((2, 2, 3), dtype=F), np.zeros((8, 6, 3), dtype=F)
    for device_call in (False, True):
        rc, msg = _up(None, 0, 0, None, None, None, None, None, device_call)
        assert rc == INV and "params" in msg
        for bad, word in BAD_PARAMS:
            rc, msg = _up(P(*bad), 0, 0, None, None, None, None, None, device_call)       # (the later checks would fail too)
            assert rc == INV and word in msg, (bad, msg)
        for Wn, H in ((0, 3), (4, 0), (-1, 3), (4, -2)):
            rc, msg = _up(P(*GOOD), Wn, H, None, None, None, None, None, device_call)
            assert rc == INV and "Wn, H" in msg, (Wn, H, msg)
        assert "too large" in _up(P(*GOOD), 1 << 15, 1 << 15, None, None, None, None, None, device_call)[1]
        assert "too large" in _up(P(*GOOD), 533333334, 1, None, None, None, None, None, device_call)[1]
        assert "NULL" in _up(P(*GOOD), 23094, 23094, None, None, None, None, None, device_call)[1]       # 533 332 836: allowed
        # a launch has fewer than 2^32 work-items and a 4 x 64 tile costs 256 of them: 2^24 tiles are refused, one fewer is not
        assert "too thin" in _up(P(*GOOD), 533333333, 1, None, None, None, None, None, device_call)[1]
        assert "NULL" in _up(P(*GOOD), 1, 533333333, None, None, None, None, None, device_call)[1]       # (8 333 334 tiles)
        assert "too thin" in _up(P(*GOOD), 4 << 24, 1, None, None, None, None, None, device_call)[1]
        assert "NULL" in _up(P(*GOOD), (4 << 24) - 4, 1, None, None, None, None, None, device_call)[1]
    for missing in range(3):
        args = [hits, lo, out]
        args[missing] = None
        rc, msg = _up(P(*GOOD), 8, 6, args[0], args[1], None, args[2], None)
        assert rc == INV and "NULL" in msg, missing
    # the device variant: fake addresses, never dereferenced -- NULL, records' alignment, floats' alignment, overlap
    HITS, LO, BASE, OUT = 0x40000, 0x10000, 0x20000, 0x30000
    for missing in range(3):
        args = [HITS, LO, OUT]
        args[missing] = None
        rc, msg = _up(P(*GOOD), 8, 6, args[0], args[1], BASE, args[2], None, True)
        assert rc == INV and "NULL" in msg, missing
    rc, msg = _up(P(*GOOD), 8, 6, HITS + 8, LO + 2, BASE, LO, None, True)                 # misaligned floats and overlapping too
    assert rc == INV and "16-byte" in msg
    for lo_, base_, out_ in ((LO + 2, BASE, OUT), (LO, BASE + 1, OUT), (LO, BASE, OUT + 2)):
        rc, msg = _up(P(*GOOD), 8, 6, HITS, lo_, base_, out_, None, True)
        assert rc == INV and "4-byte" in msg
    lo_bytes, out_bytes = 2 * 2 * 3 * 4, 8 * 6 * 3 * 4
    for d_out in (LO, LO + lo_bytes - 4, LO - out_bytes + 4):
        rc, msg = _up(P(*GOOD), 8, 6, HITS, LO, BASE, d_out, None, True)
        assert rc == INV and "overlap" in msg, hex(d_out)
    # the subsample: scale, white, the rectangle, NULL, alignment
    for device_call in (False, True):
        for scale in (1, 9, 0, -2):
            rc, msg = _sub(scale, 2, 0, 0, None, None, device_call)
            assert rc == INV and "scale" in msg
        for white in (2, -1):
            rc, msg = _sub(4, white, 0, 0, None, None, device_call)
            assert rc == INV and "white" in msg
        assert "Wn, H" in _sub(4, 1, 0, 5, None, None, device_call)[1]
        assert "too large" in _sub(4, 1, 1 << 15, 1 << 15, None, None, device_call)[1]
        assert "too thin" in _sub(4, 1, 4 << 24, 1, None, None, device_call)[1]
        assert "NULL" in _sub(4, 1, 8, 6, None, 0x1000, device_call)[1] and "NULL" in _sub(4, 1, 8, 6, 0x1000, None, device_call)[1]
    for a, b in ((HITS + 8, OUT), (HITS, OUT + 4)):
        rc, msg = _sub(4, 1, 8, 6, a, b, True)
        assert rc == INV and "16-byte" in msg
    if have_gpu:
        return
    NODEV = capi.RT_ERR_NO_DEVICE
    assert _up(P(*GOOD), 8, 6, hits, lo, None, out, None)[0] == NODEV
    assert _up(P(*GOOD), 8, 6, HITS, LO, OUT, OUT, None, True)[0] == NODEV                # in place; adjacent is not overlapping
    assert _up(P(*GOOD), 8, 6, HITS, LO, None, LO + lo_bytes, 0x50001, True)[0] == NODEV
    assert _up(P(2, 1, 0, 1, 0, 0.0, -1.5), 1, 1, hits, lo, None, out, None)[0] == NODEV   # the ranges' ends are valid
    assert _up(P(8, 3, 6, 0, 1, 3e38, 3e38), 1, 1, hits, lo, None, out, None)[0] == NODEV
    assert _sub(2, 0, 8, 6, hits, out)[0] == NODEV and _sub(8, 1, 8, 6, HITS, OUT, True)[0] == NODEV


def test_python_wrappers_refuse_without_a_device(have_gpu):
    if have_gpu:
        pytest.skip("a GPU is present")
    from tilecoderaytracer_amd import RtError, subsample_hits, upsample_guided
    hits = np.zeros((8, 6), dtype=HIT_DTYPE)
    with pytest.raises(RtError) as e:
        subsample_hits(hits, 4)
    assert e.value.code == capi.RT_ERR_NO_DEVICE
    with pytest.raises(RtError) as e:
        upsample_guided(hits, np.zeros((2, 2), dtype=F), 4)
    assert e.value.code == capi.RT_ERR_NO_DEVICE
    with pytest.raises(RtError) as e:
        subsample_hits(hits, 9)
    assert e.value.code == capi.RT_ERR_INVALID and "scale" in e.value.message
    with pytest.raises(ValueError):
        upsample_guided(hits, np.zeros((3, 2), dtype=F), 4)
    with pytest.raises(ValueError):
        upsample_guided(hits, np.zeros((2, 2), dtype=F), 4, base=np.zeros((8, 6, 3), dtype=F))


def test_executable_refuses_bad_gather_scales():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert "--gather-scale S[:SIGMA_PLANE[:refine]]" in r.stdout + r.stderr
    for bad in ("1", "9", "x", "2:-1", "2:nan", "2:0.1:refined", "2:0.1:refine:1", ""):
        r = subprocess.run([EXE, "--indirect", "2", "--gather-scale", bad, "--no-txt"], capture_output=True, text=True)
        assert r.returncode == 1 and "usage" in r.stderr, bad
    r = subprocess.run([EXE, "--gather-scale", "2", "--no-txt"], capture_output=True, text=True)       # neither --indirect nor --ao
    assert r.returncode == 1 and "usage" in r.stderr
    r = subprocess.run([EXE, "--ao", "2", "--gather-scale"], capture_output=True, text=True)           # the value is missing
    assert r.returncode == 1 and "usage" in r.stderr


# ---- 3. upsample_ref: the definition, one clause at a time ---------------------------------------------------------------------

def r32(x):
    """a Python float rounded to fp32 (the exact double product, sum or quotient of two fp32 values rounds to fp32 as the fp32
    operation does)"""
    with np.errstate(all="ignore"):
        return float(F(x))


def by_hand(hits, lo, s, x, z, squarings=0, match_color=False, modulate=False, sigma=0.0, dead_value=0.0, base=None):
    """pixel (x, z) of the header's definition, in Python floats rounded to fp32 step by step -> (values, flag)"""
    Wn, H = hits.shape
    Wl, Hl = -(-Wn // s), -(-H // s)
    lo = lo.reshape(Wl, Hl, -1)
    Cn = lo.shape[2]
    h = hits[x, z]
    flag = 0
    if h["object"] < 0 or (h["flags"] & 2):
        v = [r32(dead_value)] * Cn
    else:
        i0, j0 = x // s, z // s
        fx, fz = x - i0 * s, z - j0 * s
        if fx == 0 and fz == 0:
            v = [float(c) for c in lo[i0, j0]]
        else:
            n_p, p_p = [float(c) for c in h["normal"]], [float(c) for c in h["point"]]
            acc, wsum, fall, tsum = [0.0] * Cn, 0.0, [0.0] * Cn, 0.0
            if sigma > 0:
                inv = r32(1.0 / r32(r32(sigma) * r32(sigma)))
            for a in (0, 1):
                for b in (0, 1):
                    i, j = i0 + a, j0 + b
                    if i >= Wl or j >= Hl:
                        continue
                    tent = float((fx if a else s - fx) * (fz if b else s - fz))
                    if tent == 0:
                        continue
                    l = [float(c) for c in lo[i, j]]
                    fall = [r32(fall[c] + r32(tent * l[c])) for c in range(Cn)]
                    tsum = r32(tsum + tent)
                    g = hits[i * s, j * s]
                    if g["object"] != h["object"] or (g["flags"] & 3) != (h["flags"] & 3):
                        continue
                    if match_color and g["color"].tobytes() != h["color"].tobytes():
                        continue
                    n_q = [float(c) for c in g["normal"]]
                    t = r32(r32(r32(n_p[0] * n_q[0]) + r32(n_p[1] * n_q[1])) + r32(n_p[2] * n_q[2]))
                    wn = t if t > 0 else 0.0
                    for _ in range(squarings):
                        wn = r32(wn * wn)
                    w = r32(tent * wn)
                    if sigma > 0:
                        e = [r32(float(g["point"][c]) - p_p[c]) for c in range(3)]
                        d = r32(r32(r32(e[0] * n_p[0]) + r32(e[1] * n_p[1])) + r32(e[2] * n_p[2]))
                        u = r32(1.0 - r32(r32(d * d) * inv))
                        w = r32(w * (u if u > 0 else 0.0))
                    if not w > 0:
                        continue
                    acc = [r32(acc[c] + r32(w * l[c])) for c in range(Cn)]
                    wsum = r32(wsum + w)
            if wsum > 0:
                v = [r32(acc[c] / wsum) for c in range(Cn)]
            else:
                flag, v = 1, [r32(fall[c] / tsum) for c in range(Cn)]
        if modulate:
            v = [r32(v[c] * float(h["color"][c])) for c in range(Cn)]
    if base is not None:
        v = [r32(float(base.reshape(Wn, H, -1)[x, z, c]) + v[c]) for c in range(Cn)]
    return v, flag


def flat_frame(Wn=9, H=6, seed=3):
    """one plane seen head-on: object 0, normal +y, points on y = 0 a unit apart, one albedo"""
    hits = np.zeros((Wn, H), dtype=HIT_DTYPE)
    hits["normal"] = [0, 1, 0]
    hits["color"] = [0.25, 0.5, 0.75]
    hits["distance"] = 5
    xs, zs = np.meshgrid(np.arange(Wn), np.arange(H), indexing="ij")
    hits["point"][..., 0], hits["point"][..., 2] = xs, zs
    return hits


def check_all_pixels(hits, lo, s, **kw):
    ref_kw = dict(normal_squarings=kw.get("squarings", 0), match_color=kw.get("match_color", False),
                  modulate=kw.get("modulate", False), sigma_plane=kw.get("sigma", 0.0), dead_value=kw.get("dead_value", 0.0),
                  base=kw.get("base"))
    out, flags = upsample_ref.upsample(hits, lo, s, **ref_kw)
    Wn, H = hits.shape
    for x in range(Wn):
        for z in range(H):
            v, flag = by_hand(hits, lo, s, x, z, **kw)
            got = np.atleast_1d(out[x, z])
            assert upsample_ref.same_bits(got, np.array(v, dtype=F)), (x, z, got, v)
            assert int(flags[x, z]) == flag, (x, z)
    return out, flags


S4 = 4
# pixel (1, 1) at s = 4: its cells are pixels (0, 0), (0, 4), (4, 0), (4, 4), with tents 9, 3, 3, 1
CLAUSES = {
    "other object": lambda h: h["object"].__setitem__((4, 4), 1),
    "inside against outside": lambda h: h["flags"].__setitem__((4, 4), 1),
    "normal at 90 degrees": lambda h: h["normal"].__setitem__((4, 4), [1, 0, 0]),
    "normal beyond 90 degrees": lambda h: h["normal"].__setitem__((4, 4), [0.6, -0.8, 0]),
    "a NaN normal": lambda h: h["normal"].__setitem__((4, 4), [0, np.nan, 0]),
}


@pytest.mark.parametrize("clause", sorted(CLAUSES))
@pytest.mark.parametrize("channels", [1, 3])
def test_ref_a_tap_the_clause_rejects_counts_for_nothing(clause, channels):
    """the tap at cell (1, 1) is rejected: the pixels it alone would have reached are unchanged by its value, every pixel equals
    the hand computation, and the result differs from the unmodified frame's"""
    rng = np.random.default_rng(7)
    hits = flat_frame()
    lo = rng.random((3, 2, channels), dtype=F).reshape((3, 2, 3) if channels == 3 else (3, 2))
    plain, _ = upsample_ref.upsample(hits, lo, S4, 0)
    CLAUSES[clause](hits)
    out, flags = check_all_pixels(hits, lo, S4, squarings=2 if "NaN" in clause else 0)
    other = lo.copy()
    other[1, 1] = 77.0
    out2, _ = upsample_ref.upsample(hits, other, S4, 2 if "NaN" in clause else 0)
    inner = np.zeros(hits.shape, dtype=bool)
    inner[1:4, 1:4] = True                                   # pixels whose four cells are (0,0), (0,1), (1,0), (1,1)
    assert upsample_ref.same_bits(out[inner], out2[inner])   # the rejected tap's value is never read into them
    assert not upsample_ref.same_bits(out[inner], plain[inner])
    assert not flags[inner].any()                            # three taps are left
    assert np.isfinite(out[inner]).all()


def test_ref_colour_bits_with_and_without_match_color():
    hits = flat_frame()
    lo = np.random.default_rng(8).random((3, 2, 3), dtype=F)
    hits["color"][4, 4] = [0.25, 0.5, np.nextafter(F(0.75), F(1))]         # one bit apart
    off, _ = check_all_pixels(hits, lo, S4, match_color=False)
    on, _ = check_all_pixels(hits, lo, S4, match_color=True)
    same = flat_frame()
    assert upsample_ref.same_bits(off, upsample_ref.upsample(same, lo, S4, 0)[0])       # without: the colour is not looked at
    assert not upsample_ref.same_bits(on[1:4, 1:4], off[1:4, 1:4])
    hits["color"] = [0.0, 0.5, 0.75]
    hits["color"][0, 0, 0] = -0.0                                           # +0.0 against -0.0: equal as floats, not as bits
    on, _ = check_all_pixels(hits, lo, S4, match_color=True, modulate=True)
    v, _ = by_hand(hits, lo, S4, 1, 1, match_color=True, modulate=True)
    w, _ = by_hand(hits, lo, S4, 1, 1, match_color=False, modulate=True)
    assert v != w


def test_ref_plane_distance_just_inside_and_just_outside_sigma():
    hits = flat_frame()
    lo = np.random.default_rng(9).random((3, 2), dtype=F)
    hits["point"][4, 4, 1] = 0.5                             # the tap's point half a unit off the pixels' tangent plane
    plain, _ = upsample_ref.upsample(flat_frame(), lo, S4, 0, sigma_plane=0.5)
    for sigma, rejected in ((0.5, True), (float(np.nextafter(F(0.5), F(1))), False), (0.49, True), (0.75, False)):
        out, flags = check_all_pixels(hits, lo, S4, sigma=sigma)
        other = lo.copy()
        other[1, 1] = 77.0
        out2, _ = upsample_ref.upsample(hits, other, S4, 0, sigma_plane=sigma)
        assert upsample_ref.same_bits(out[1:4, 1:4], out2[1:4, 1:4]) == rejected, sigma
    out, _ = check_all_pixels(hits, lo, S4, sigma=0.0)       # no plane term: the point is not looked at
    assert upsample_ref.same_bits(out, upsample_ref.upsample(flat_frame(), lo, S4, 0)[0])
    hits["point"][4, 4, 1] = np.nan                          # a NaN point: u is NaN, the tap is dropped
    out, flags = check_all_pixels(hits, lo, S4, sigma=0.5)
    assert np.isfinite(out[1:4, 1:4]).all() and not flags[1:4, 1:4].any()


def test_ref_a_nan_value_enters_only_through_a_positive_weight():
    hits = flat_frame()
    lo = np.random.default_rng(10).random((3, 2, 3), dtype=F)
    lo[1, 1, 1] = np.nan
    out, flags = check_all_pixels(hits, lo, S4)
    assert np.isnan(out[1:4, 1:4, 1]).all() and np.isfinite(out[..., [0, 2]]).all()
    assert np.isfinite(out[:, 0, 1]).all()                   # z = 0: fz = 0, the b = 1 tents are 0 and the NaN is never multiplied
    hits["object"][4, 4] = 3                                 # rejected: the NaN stays out, except at its own pixel
    out, flags = check_all_pixels(hits, lo, S4)
    # (pixels beyond (4, 4) have it as their cell (0, 0) of another object and may become holes, whose unguided tent reads it)
    assert np.isfinite(out[:4, :4]).all() and np.isnan(out[4, 4, 1])


def test_ref_own_samples_dead_pixels_holes_and_cells_beyond_the_frame():
    rng = np.random.default_rng(11)
    hits = flat_frame(9, 6)                                  # s = 4: Wl = 3, Hl = 2 -- column 8 is cell 2's own, rows 4, 5 cell 1's
    lo = rng.random((3, 2, 3), dtype=F)
    lo.view(np.uint32)[2, 1, 0] = 0x7FC12345                 # a NaN with a payload: own samples are copied word for word
    base = rng.random((9, 6, 3), dtype=F)
    hits["object"][2, 2] = -1                                # a miss
    hits["flags"][3, 1] = 2                                  # a light
    hits["object"][5, 1] = 9                                 # a pixel none of whose cells is its object: a hole
    hits["color"][5, 1] = [2.0, 3.0, 4.0]
    out, flags = check_all_pixels(hits, lo, S4, dead_value=0.125)
    assert np.array_equal(out.view(np.uint32)[::4, ::4], lo.view(np.uint32))
    assert (out[2, 2] == F(0.125)).all() and (out[3, 1] == F(0.125)).all()
    assert flags.sum() == 1 and flags[5, 1]
    # the hole's fallback: the plain tent over its four cells (4,0) 9, (4,4) 3, (8,0) 3, (8,4) 1
    mod, flags = check_all_pixels(hits, lo, S4, dead_value=0.125, modulate=True, base=base)
    assert upsample_ref.same_bits(mod[5, 1], base[5, 1] + out[5, 1] * hits["color"][5, 1])
    assert upsample_ref.same_bits(mod[2, 2], base[2, 2] + F(0.125))                      # modulate does not apply to a dead pixel
    assert upsample_ref.same_bits(mod[4, 4], base[4, 4] + lo[1, 1] * hits["color"][4, 4])
    # cells beyond Wl and Hl: pixel (8, 5) has cell (2, 1) alone, tent 4 * 3 (fx = 0: the a = 1 tents are 0; row j = 2 does not exist)
    v, flag = by_hand(hits, lo, S4, 8, 5)
    want = [r32(r32(12.0 * float(c)) / 12.0) for c in lo[2, 1]]
    assert flag == 0 and all(a == b or (a != a and b != b) for a, b in zip(v, want))
    for shape, s in (((7, 1), 2), ((1, 9), 3), ((3, 3), 8), ((8, 8), 8), ((5, 11), 5)):
        hits = flat_frame(*shape)
        hits["object"][shape[0] // 2, shape[1] // 2] = 2
        lo = rng.random((-(-shape[0] // s), -(-shape[1] // s)), dtype=F)
        out, flags = check_all_pixels(hits, lo, s, squarings=1, sigma=0.7, dead_value=1.0)
        assert np.isfinite(out).all()
    out, flags = check_all_pixels(flat_frame(3, 3), np.array([[F(0.3)]]), 8)               # Wl = Hl = 1: every pixel is lo's
    assert (np.abs(out - F(0.3)) <= 2.0 ** -24).all() and not flags.any()


def test_ref_subsample():
    hits = np.array(adaptive_frames.first_pass("builtin", 61, 37, 4)[1])
    hits["object"][24, 24] = -1                              # dead records that every scale picks
    hits["flags"][48, 0] |= 2
    for s in (2, 3, 4, 8):
        plain, white = upsample_ref.subsample(hits, s), upsample_ref.subsample(hits, s, True)
        assert plain.shape == (-(-61 // s), -(-37 // s)) and plain.tobytes() == np.ascontiguousarray(hits[::s, ::s]).tobytes()
        dead = upsample_ref.dead_records(plain)
        assert dead.any() and (~dead).any()
        assert (white["color"][~dead] == 1).all() and white[dead].tobytes() == plain[dead].tobytes()
        for name in HIT_DTYPE.names:
            if name != "color":
                assert white[name].tobytes() == plain[name].tobytes()


# ---- 4. the conditions on the frames the GPU tests compare -----------------------------------------------------------------------

def gather_case(frame):
    """-> (hits, white cells, lo: the oracle's indirect term of the cells without albedo) of a frame of GATHER_FRAMES"""
    key, W, H, depth, s, squarings, sigma, n, seed, gather_depth = frame
    hits = adaptive_frames.first_pass(key, W, H, depth)[1]
    cells = upsample_ref.subsample(hits, s, True)
    lo = indirect_ref.indirect(adaptive_frames.oracle_scene(key), cells, n, gather_depth, 1.0, seed, 0)
    return hits, cells, lo


@pytest.mark.parametrize("frame", GATHER_FRAMES, ids=lambda f: f"{f[0]}{f[1]}x{f[2]}s{f[4]}")
def test_conditions_on_the_compared_frames(frame):
    """Each compared frame, at its scale, by the reference alone: at least 50 pixels with a tap rejected by the object clause,
    50 by the normal clause and 50 by the plane clause; at least 20 holes, at most a quarter of the live pixels; at least 200
    distinct output colours.  Found: builtin 1400 / 52 / 338, 443 holes of 2254 live, 964 distinct colours; random3 1221 / 92 /
    324, 510 holes of 2257 live, 1638 distinct colours."""
    key, W, H, depth, s, squarings, sigma, n, seed, gather_depth = frame
    hits, cells, lo = gather_case(frame)
    out, flags, rejected = upsample_ref.upsample(hits, lo, s, squarings, False, True, sigma, 0.0, None, True)
    live = int((~upsample_ref.dead_records(hits)).sum())
    counts = {k: int(v.sum()) for k, v in rejected.items()}
    distinct = upsample_ref.distinct_colours(out)
    print(f"{key} {W}x{H} s{s}: rejected {counts}, holes {int(flags.sum())} of {live} live, distinct colours {distinct}")
    assert np.isfinite(out).all()
    for clause in ("object", "normal", "plane"):
        assert counts[clause] >= 50, (clause, counts)
    assert 20 <= flags.sum() <= 0.25 * live, (int(flags.sum()), live)
    assert distinct >= 200, distinct
