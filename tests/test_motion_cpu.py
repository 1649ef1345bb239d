"""Temporal accumulation that follows moving objects (include/rt_motion.h) without a GPU: the header, the exported symbols, every
argument check in the header's order (none touches a device), motion_ref -- the tests' restatement of the definition -- against
temporal_ref where no record moves and against a per-pixel restatement in np.float32 scalars, the conditions on the pose pairs
test_motion_gpu.py compares, counted on the oracle's records, and object_motions()."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import motion_ref
import motion_scenes
import temporal_ref
from test_temporal_cpu import PAIRS, made_up_history, pair_records
from test_upsample_gpu import random_frame
from tilecoderaytracer_amd import capi, object_motions
from tilecoderaytracer_amd.renderer import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_motion.h")
FUNCTIONS = ["rt_capi_motion_version", "rt_motion_accumulate", "rt_motion_accumulate_device"]
F = np.float32
NAMES = ("value", "moments", "length", "variance", "flags")
NORMAL_COS, PLANE_EPS = 0.9, 0.05


def same_words(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), f"{what}: {name}"


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t)\s+(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    assert re.findall(r'#include\s+[<"]([^>"]+)[>"]', text) == ["rt_capi_query.h"]
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    lines = [line.split() for line in r.stdout.splitlines() if line.split()]
    exported = sorted(p[-1] for p in lines if p[-2] == "T" and re.fullmatch(r"rt_\w*motion\w*", p[-1]))
    assert exported == FUNCTIONS                              # and nothing else of this unit
    assert int(re.search(r"#define RT_CAPI_MOTION_VERSION (\d+)", text).group(1)) == lib.rt_capi_motion_version() == 1
    assert C.sizeof(capi.RtObjectMotion) == 48
    # no render kernel came with the unit, and the catalogue does not know it
    kernels = {p[-1] for p in lines if p[-1].startswith("rt_render_kernel")}
    assert len(kernels) == 117 and not [n for n in kernels if "motion" in n]
    assert "motion" not in open(os.path.join(ROOT, "tilecoderaytracer_amd", "csrc", "rt_tables.h")).read()
    # rt_temporal.h still declares its three functions and points here for moving objects
    temporal = open(os.path.join(INCLUDE, "rt_temporal.h")).read()
    assert "rt_motion.h" in temporal and "moving objects (records carry no motion)" not in temporal


def test_header_is_plain_c99_with_every_other_header_and_the_struct_is_48_bytes(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    others = sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))
    assert "rt_motion.h" in others and len(others) >= 19
    for first in ('#include "rt_motion.h"\n', ""):               # on its own before rt_temporal.h, and after it
        src = tmp_path / "motion.c"
        src.write_text(first + "".join(f'#include "{h}"\n' for h in others) +
                       "#include <stddef.h>\n"
                       "int main(void) { rt_object_motion m = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}}; rt_temporal_params p; (void)p;\n"
                       "  return (RT_CAPI_MOTION_VERSION == 1 && sizeof m == 48 && sizeof m.m == 48 && offsetof(rt_object_motion, m) == 0\n"
                       "          && sizeof(rt_object_motion[3]) == 144 && m.m[10] == 1.0f) ? 0 : 1; }\n")
        exe = tmp_path / "motion"
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert subprocess.run([str(exe)]).returncode == 0


# ---- 2. the argument checks, in the header's order, without a device ---------------------------------------------------------

P = capi.RtTemporalParams
GOOD = (3, 0, 32, 0.9, 0.05, 0.0, 0.0)
CAM, CAM_PREV = 0x7000, 0x7100                                  # fake addresses: no check dereferences a camera or a buffer
CUR, CUR_HITS, PREV_HITS, PREV_VALUE, PREV_MOMENTS, PREV_LEN = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
OUT_VALUE, OUT_MOMENTS, OUT_LEN, OUT_VARIANCE, OUT_FLAGS = 0x700000, 0x800000, 0x900000, 0xA00000, 0xB00001
TABLE = 0xC00000
FIRST = (None, CAM, CUR, CUR_HITS, None, None, None, None, OUT_VALUE, OUT_MOMENTS, OUT_LEN, OUT_VARIANCE, OUT_FLAGS)
LATER = (CAM_PREV, CAM, CUR, CUR_HITS, PREV_HITS, PREV_VALUE, PREV_MOMENTS, PREV_LEN, OUT_VALUE, OUT_MOMENTS, OUT_LEN, OUT_VARIANCE,
         OUT_FLAGS)
NONE = (None,) * 13


def _call(params, W, H, x0, x1, table, n, pointers, device_call, device=0):
    """pointers: (cam_prev, cam, cur, cur_hits, prev_hits, prev_value, prev_moments, prev_len, the five outputs), addresses"""
    lib = capi.load_library()
    p = C.byref(params) if params is not None else None
    cams = [C.cast(a, C.POINTER(capi.RtCameraDesc)) if a else None for a in pointers[:2]]
    fn = lib.rt_motion_accumulate_device if device_call else lib.rt_motion_accumulate
    rc = fn(device, p, cams[0], cams[1], W, H, x0, x1, table, n, *pointers[2:], None)
    return rc, lib.rt_last_error().decode()


def test_every_argument_check_comes_before_the_device_in_the_headers_order(have_gpu):
    from test_temporal_cpu import BAD_PARAMS, EDGE_PARAMS
    INV = capi.RT_ERR_INVALID
    for device_call in (False, True):
        # rt_temporal_accumulate's checks, in its order, each with the table's checks failing too (n_motions -1)
        rc, msg = _call(None, 0, 0, -1, -1, None, -1, NONE, device_call)
        assert rc == INV and "params" in msg
        for bad, word in BAD_PARAMS:
            rc, msg = _call(P(*bad), 0, 0, -1, -1, None, -1, NONE, device_call)
            assert rc == INV and word in msg, (bad, msg)
        for W, H in ((0, 3), (4, 0), (-1, 3), (4, -2)):
            rc, msg = _call(P(*GOOD), W, H, -1, W + 1, None, -1, NONE, device_call)
            assert rc == INV and "W, H" in msg, (W, H, msg)
        for x0, x1 in ((-1, 4), (0, 9), (4, 4), (5, 4), (8, 8)):
            rc, msg = _call(P(*GOOD), 8, 1 << 30, x0, x1, None, -1, NONE, device_call)
            assert rc == INV and "x0" in msg, (x0, x1, msg)
        for W, H in ((1 << 15, 1 << 15), (533333334, 1), (23095, 23094)):
            assert "too large" in _call(P(*GOOD), W, H, 0, 1, None, -1, NONE, device_call)[1]
        for W, H, x0, x1 in ((23094, 23094, 0, 23094), (533333333, 1, 533333332, 533333333)):
            rc, msg = _call(P(*GOOD), W, H, x0, x1, None, -1, NONE, device_call)  # allowed: the next check speaks
            assert rc == INV and "NULL" in msg and "first frame" not in msg
        for edge in EDGE_PARAMS:
            assert "is NULL" in _call(P(*edge), 8, 6, 0, 8, None, -1, NONE, device_call)[1]
        for missing in (1, 2, 3, 8, 9, 10):
            for base in (FIRST, LATER):
                args = list(base)
                args[missing] = None
                args[5] = None if base is LATER else PREV_VALUE                    # (the first-frame rule is broken too)
                rc, msg = _call(P(*GOOD), 8, 6, 0, 8, None, -1, args, device_call)
                assert rc == INV and "is NULL" in msg, (missing, msg)
        for k in range(1, 32 - 1):                                               # every mix of the five but none and all
            given = [(k >> b) & 1 for b in range(5)]
            args = list(LATER)
            for slot, g in zip((0, 4, 5, 6, 7), given):
                args[slot] = args[slot] if g else None
            rc, msg = _call(P(*GOOD), 8, 6, 0, 8, None, 4097, args, device_call)   # (the table is too long as well)
            assert rc == INV and "first frame" in msg, (given, msg)
        # the new checks, after the first-frame rule: the count's range, then the table's presence; on a first frame as well
        for base in (FIRST, LATER):
            misaligned = list(base)
            misaligned[3] = CUR_HITS + 8                                         # (a misaligned record buffer too)
            for n in (-1, 4097, -(1 << 31), (1 << 31) - 1):
                rc, msg = _call(P(*GOOD), 8, 6, 0, 8, None, n, misaligned, device_call)
                assert rc == INV and "n_motions must" in msg, (n, msg)
            for n in (1, 4096):
                rc, msg = _call(P(*GOOD), 8, 6, 0, 8, None, n, misaligned, device_call)
                assert rc == INV and "motions is NULL" in msg, (n, msg)
    # the device variant: the records' and the table's alignment in one clause, the floats' alignment, the overlaps
    for slot in (3, 4):
        for off in (4, 8):
            args = list(LATER)
            args[slot] += off
            args[2] += 2                                                         # (a misaligned float too)
            rc, msg = _call(P(*GOOD), 8, 6, 0, 8, TABLE, 14, args, True)
            assert rc == INV and "16-byte" in msg, slot
    for off in (4, 8, 12):
        for n in (0, 1, 4096):                                                   # (the table's alignment does not wait for a length)
            args = list(LATER)
            args[2] += 2
            rc, msg = _call(P(*GOOD), 8, 6, 0, 8, TABLE + off, n, args, True)
            assert rc == INV and "16-byte" in msg and "d_motions" in msg, (off, n)
    for slot in (2, 5, 6, 7, 8, 9, 10, 11):
        args = list(LATER)
        args[slot] += 2
        args[12] = TABLE                                                         # (an overlapping output too)
        rc, msg = _call(P(*GOOD), 8, 6, 0, 8, TABLE, 14, args, True)
        assert rc == INV and "4-byte" in msg, slot
    outs = {8: 4 * 6 * 12, 9: 4 * 6 * 8, 10: 4 * 6 * 4, 11: 4 * 6 * 4, 12: 4 * 6}    # a strip [2, 6)'s bytes
    for n in (1, 14, 4096):
        for o, ob in outs.items():
            step = 1 if o == 12 else 4
            for address, refused in ((TABLE, True), (TABLE + n * 48 - step, True), (TABLE - ob + step, True), (TABLE + n * 48, False),
                                     (TABLE - ob, False)):
                args = list(LATER)
                args[o] = address
                rc, msg = _call(P(*GOOD), 8, 6, 2, 6, TABLE, n, args, True, device=-1)
                # (adjacent is not overlapping: the call goes on to the device, whose index is bad or which there is none of)
                assert rc != capi.RT_OK and ("overlaps the motion table" in msg) == refused and (rc == INV or not refused), (n, o, msg)
    args = list(LATER)
    args[8] = PREV_LEN                                                           # rt_temporal.h's overlap rule still holds
    assert "overlaps a prev_" in _call(P(*GOOD), 8, 6, 2, 6, TABLE, 14, args, True)[1]
    if have_gpu:
        return
    NODEV = capi.RT_ERR_NO_DEVICE                                                # every admitted edge reaches the device check
    for n, table in ((0, None), (0, TABLE), (1, TABLE), (4096, TABLE)):
        assert _call(P(*GOOD), 8, 6, 0, 8, table, n, FIRST, True)[0] == NODEV
        assert _call(P(*GOOD), 8, 6, 2, 6, table, n, LATER, True)[0] == NODEV
    hits, cur = np.zeros((8, 6), dtype=HIT_DTYPE), np.zeros((8, 6, 3), dtype=F)
    out = [np.zeros((8, 6, k), dtype=F) for k in (3, 2, 1, 1)]
    cam = motion_scenes.camera_pair("equal")[0]
    host = (0, C.addressof(cam), cur.ctypes.data, hits.ctypes.data, None, None, None, None) + tuple(a.ctypes.data for a in out) + (None,)
    table = np.tile(motion_ref.IDENTITY, (4096, 1))
    assert _call(P(*GOOD), 8, 6, 0, 8, table.ctypes.data, 4096, host, False)[0] == NODEV
    assert _call(P(*GOOD), 8, 6, 0, 8, None, 0, host, False)[0] == NODEV


def test_python_wrappers_refuse_without_a_device(have_gpu):
    if have_gpu:
        pytest.skip("a GPU is present")
    from tilecoderaytracer_amd import RtError, motion_accumulate
    cam = motion_scenes.camera_pair("equal")[0]
    hits = np.zeros((8, 6), dtype=HIT_DTYPE)
    with pytest.raises(RtError) as e:
        motion_accumulate(np.zeros((8, 6, 3), dtype=F), hits, cam, motions=np.zeros((3, 12), dtype=F))
    assert e.value.code == capi.RT_ERR_NO_DEVICE
    with pytest.raises(RtError) as e:
        motion_accumulate(np.zeros((8, 6), dtype=F), hits, cam, motions=np.zeros((4097, 12), dtype=F))
    assert e.value.code == capi.RT_ERR_INVALID and "n_motions" in e.value.message
    with pytest.raises(ValueError):
        motion_accumulate(np.zeros((8, 6), dtype=F), hits, cam, motions=np.zeros((3, 9), dtype=F))
    with pytest.raises(ValueError):
        motion_accumulate(np.zeros((8, 5), dtype=F), hits, cam)


# ---- 3. motion_ref: the definition ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PAIRS)
def test_ref_without_a_moving_record_is_temporal_ref_word_for_word(name):
    """no table, an all-identity table and a table shorter than every object index that occurs (whatever it holds)"""
    W, H = 61, 37
    cam_prev, cam, prev_hits, hits = pair_records(name, W, H)
    live = ~temporal_ref.dead_records(hits)
    lowest = int(hits["object"][live].min())
    assert lowest >= 1                                           # a table of `lowest` entries names no object of the frame
    rng = np.random.default_rng(len(name))
    short = rng.random((lowest, 12), dtype=F)
    for channels, kw in ((3, dict()), (1, dict(match_color=True, plane_eps=0.0, alpha=0.2, max_history=4))):
        cur = rng.random((W, H, 3) if channels == 3 else (W, H), dtype=F)
        prev = (cam_prev, prev_hits) + made_up_history(H + channels, W, H, channels)
        want = temporal_ref.accumulate(cur, hits, cam, prev, **kw)
        for what, motions in (("no table", None), ("empty", np.zeros((0, 12), dtype=F)), ("identity", np.tile(motion_ref.IDENTITY, (4096, 1))),
                              ("short", short)):
            same_words(motion_ref.accumulate(cur, hits, cam, prev, motions, **kw), want, f"{name} {what}")
        # a table that moves is another result (the pairs have live pixels with history)
        moved = motion_ref.accumulate(cur, hits, cam, prev, np.tile(motion_ref.IDENTITY + F(0.25), (4096, 1)), **kw)
        assert moved[4].sum() > want[4].sum()
    same_words(motion_ref.accumulate(cur, hits, cam, None, rng.random((4096, 12), dtype=F)), temporal_ref.accumulate(cur, hits, cam, None),
               "first frame")


def made_up_table(seed, n=4096):
    """identity entries, small rigid motions, a mirror, a non-rigid matrix, entries holding NaN, infinity and -0.0"""
    rng = np.random.default_rng(seed)
    table = np.tile(motion_ref.IDENTITY, (n, 1))
    kinds = rng.integers(0, 8, n)
    for o, kind in ((0, 3), (5, 0), (6, 3), (169, 4), (170, 3), (171, 4)):      # the objects spread_objects() always has
        if o < n:
            kinds[o] = kind
    for o in np.flatnonzero(kinds >= 3):                         # three in eight stay the identity
        R = motion_scenes.rotation(rng.normal(size=3), rng.normal() * 0.05)
        t = rng.normal(size=3) * 0.08
        if kinds[o] == 5:
            R = R @ np.diag([1.0, -1.0, 1.0])                    # a mirror
        if kinds[o] == 6:
            R = R + rng.normal(size=(3, 3)) * 0.05               # not rigid
        table[o] = np.concatenate([R, t[:, None]], axis=1).reshape(12).astype(F)
        if kinds[o] == 7:
            table[o, rng.integers(0, 12)] = [np.nan, np.inf, -np.inf][rng.integers(0, 3)]
    table[1::16, 1] = F(-0.0)                                    # the identity but for a sign: moving, by the bits
    table.setflags(write=False)
    return table


def spread_objects(hits, seed, n=4096):
    """the live records' object indices spread over 0..n-1, in runs so that neighbours still share objects: six indices on
    either side of the table lengths the tests cut at, and six anywhere"""
    rng = np.random.default_rng(seed)
    out = hits.copy()
    pick = np.concatenate([[0, 5, 6, 169, 170, 171], rng.integers(0, n, 6)])
    live = out["object"] >= 0
    Wn, H = out.shape
    x, z = np.meshgrid(np.arange(Wn), np.arange(H), indexing="ij")
    out["object"][live] = pick[(out["object"] * 4 + (x // 9) + 2 * (z // 16))[live] % 12]
    return out


def by_hand(cur, hits, cam, prev, motions, x, z, x0=0, match_color=False, max_history=32, normal_cos=0.9, plane_eps=0.05, alpha=0.0,
            alpha_moments=0.0):
    """pixel (x, z) of the strip by the header's definition, every operation on np.float32 scalars ->
    (value list, m1, m2, len, variance, flag)"""
    one, zero = F(1.0), F(0.0)
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    h = hits[x, z]
    c = [F(v) for v in np.atleast_1d(cur[x, z])]
    l = (F(0.25) * c[0] + F(0.5) * c[1]) + F(0.25) * c[2] if len(c) == 3 else c[0]
    none = (c, l, l * l, one, zero, 1)
    if prev is None or h["object"] < 0 or (h["flags"] & 2):
        return none
    cam_prev, g_all, p_value, p_moments, p_len = prev
    W, H = g_all.shape
    o = int(h["object"])
    Pp, Np = [F(v) for v in h["point"]], [F(v) for v in h["normal"]]
    moving = motions is not None and o < len(motions) and motions[o].tobytes() != motion_ref.IDENTITY.tobytes()
    if moving:
        m, P, N = [F(v) for v in motions[o]], Pp, Np
        Pp = [((m[4 * k] * P[0] + m[4 * k + 1] * P[1]) + m[4 * k + 2] * P[2]) + m[4 * k + 3] for k in range(3)]
        Np = [(m[4 * k] * N[0] + m[4 * k + 1] * N[1]) + m[4 * k + 2] * N[2] for k in range(3)]
    if temporal_ref.camera_words(cam_prev).tobytes() == temporal_ref.camera_words(cam).tobytes() and not moving:
        taps = [(x0 + x, z, one)]
    else:
        w = [F(v) for v in temporal_ref.camera_words(cam_prev)]
        sw, sh, shw, shh, so, hv, vv, eye = w[0], w[1], w[2], w[3], w[4:7], w[7:10], w[10:13], w[13:16]
        O = [so[k] - eye[k] for k in range(3)]
        nh, na, nb = cross(hv, vv), cross(vv, O), cross(O, hv)
        D = [Pp[k] - eye[k] for k in range(3)]
        s, q = dot(D, nh), dot(O, nh)
        if not s * q > 0:
            return none
        a, b = dot(D, na) / s, dot(D, nb) / s
        px = ((a + shw) / sw) * F(W)
        pz = ((b + shh) / sh) * F(H)
        if not (px > -1 and px < F(W) and pz > -1 and pz < F(H)):
            return none
        i0, j0 = int(np.floor(px)), int(np.floor(pz))
        fx, fz = px - F(i0), pz - F(j0)
        taps = []
        for a in (0, 1):
            for b in (0, 1):
                bw = (fx if a else one - fx) * (fz if b else one - fz)
                if 0 <= i0 + a < W and 0 <= j0 + b < H and bw > 0:
                    taps.append((i0 + a, j0 + b, bw))
    n_words = len(c) + 3
    acc, wsum = [zero] * n_words, zero
    for i, j, bw in taps:
        g = g_all[i, j]
        if g["object"] != h["object"] or (g["flags"] & 3) != (h["flags"] & 3):
            continue
        if match_color and g["color"].tobytes() != h["color"].tobytes():
            continue
        if not dot(Np, [F(v) for v in g["normal"]]) >= F(normal_cos):
            continue
        if F(plane_eps) > 0:
            e = [F(g["point"][k]) - Pp[k] for k in range(3)]
            d = dot(e, Np)
            if not d * d <= F(plane_eps) * F(plane_eps):
                continue
        words = [F(v) for v in np.atleast_1d(p_value[i, j])] + [F(p_moments[i, j, 0]), F(p_moments[i, j, 1]), F(p_len[i, j])]
        acc = [acc[k] + bw * words[k] for k in range(n_words)]
        wsum = wsum + bw
    if not wsum > 0:
        return none
    hk = [a / wsum for a in acc]
    N = hk[-1] + one
    if not N <= F(max_history):
        N = F(max_history)
    ac = am = one / N
    if not ac >= F(alpha):
        ac = F(alpha)
    if not am >= F(alpha_moments):
        am = F(alpha_moments)
    value = [hk[k] + ac * (c[k] - hk[k]) for k in range(len(c))]
    m1 = hk[-3] + am * (l - hk[-3])
    m2 = hk[-2] + am * (l * l - hk[-2])
    v = m2 - m1 * m1
    return value, m1, m2, N, v if v > 0 else zero, 0


def made_up_case(Wn, H, seed):
    """made-up records with objects over 0..4095 under a moved camera, as test_temporal_gpu.py's made-up test has them"""
    import cameras
    hits, prev_hits = spread_objects(random_frame(seed, Wn, H), seed + 5), spread_objects(random_frame(seed, Wn, H), seed + 5)
    changed = np.random.default_rng(seed + 1).random((Wn, H)) < 0.3
    prev_hits[changed] = spread_objects(random_frame(seed + 2, Wn, H), seed + 5)[changed]
    centre = np.array([Wn * 0.125, 0.0, H * 0.125])
    cam = cameras.camera(centre + [0.0, -12.0, 0.0], centre, up=(0.0, 0.0, 1.0), screen=(1.5, 1.5))
    cam_prev = cameras.camera(centre + [0.4, -12.0, -0.3], centre + [0.2, 0.0, 0.1], up=(0.0, 0.0, 1.0), screen=(1.5, 1.5), roll=0.05)
    return cam_prev, cam, prev_hits, hits


def test_ref_equals_the_definition_in_float32_scalars_on_made_up_records():
    Wn, H = 5, 67
    cam_prev, cam, prev_hits, hits = made_up_case(Wn, H, 21)
    table = made_up_table(3)
    rng = np.random.default_rng(4)
    seen_moving = 0
    for channels, cams, kw in ((3, (cam_prev, cam), dict(normal_cos=0.3, plane_eps=0.5)), (3, (cam, cam), dict(normal_cos=0.3, plane_eps=0.5)),
                               (1, (cam_prev, cam), dict(normal_cos=-1.0, plane_eps=0.0, match_color=True, max_history=3, alpha=0.5))):
        cur = rng.random((Wn, H, 3) if channels == 3 else (Wn, H), dtype=F)
        prev = (cams[0], prev_hits) + made_up_history(5, Wn, H, channels)
        out = motion_ref.accumulate(cur, hits, cams[1], prev, table, details=True, **kw)
        info = out[5]
        assert info["moving"].sum() >= 60 and (~info["moving"] & ~temporal_ref.dead_records(hits)).sum() >= 60
        assert (~out[4]).sum() >= 40 and out[4][info["moving"]].sum() >= 10 and (~out[4][info["moving"]]).sum() >= 10
        seen_moving += int(info["moving"].sum())
        with np.errstate(all="ignore"):
            for x in range(Wn):
                for z in range(H):
                    value, m1, m2, n, var, flag = by_hand(cur, hits, cams[1], prev, table, x, z, **kw)
                    got = [np.atleast_1d(out[0][x, z]), out[1][x, z], out[2][x, z], out[3][x, z]]
                    want = [np.array(value, dtype=F), np.array([m1, m2], dtype=F), F(n), F(var)]
                    for g, w, what in zip(got, want, NAMES):
                        assert np.array_equal(np.asarray(g, dtype=F).view(np.uint32), np.asarray(w, dtype=F).view(np.uint32)) or \
                            (np.isnan(g).all() and np.isnan(w).all()), (x, z, what, g, w)
                    assert int(out[4][x, z]) == flag, (x, z)
    # a NaN anywhere in a motion gives that object's pixels no history
    objects = np.unique(hits["object"][info["moving"]])
    for o in objects:
        for word in (0, 3, 6, 11):
            broken = table.copy()
            broken[o, word] = np.nan
            flags = motion_ref.accumulate(cur, hits, cams[1], prev, broken, **kw)[4]
            assert flags[hits["object"] == o].all(), (o, word)


def test_refs_given_a_window_of_the_previous_frame_equal_the_whole_frames_columns_and_refuse_a_narrow_one():
    """prev_x0, which test_motion_large_gpu.py's reference rests on: temporal_ref and motion_ref given only the previous frame's
    columns that the taps of a few current columns reach (temporal_ref.tap_columns) equal, word for word, what they give with the
    whole 61 x 37 previous frame; a window one column narrower on either side raises, it is never a rejected tap"""
    W, H = 61, 37
    cases = [(temporal_ref.accumulate, pair_records("truck", W, H), None, 3)]
    cases.append((motion_ref.accumulate, motion_scenes.records("spheres_truck", W, H), motion_scenes.table("spheres_truck"), 1))
    windows = 0
    for accumulate, (cam_prev, cam, prev_hits, hits), table, channels in cases:
        rng = np.random.default_rng(channels)
        cur = rng.random((W, H, 3) if channels == 3 else (W, H), dtype=F)
        history = made_up_history(11, W, H, channels)
        more = dict(normal_cos=-1.0, plane_eps=0.0, max_history=4) if table is None else dict(motions=table)
        whole = accumulate(cur, hits, cam, (cam_prev, prev_hits) + history, **more)
        assert 50 <= whole[4].sum() <= W * H - 200
        for c0, c1 in ((0, 1), (20, 23), (31, 33), (60, 61), (0, 61)):
            part = np.ascontiguousarray(hits[c0:c1])
            before = part["point"] if table is None else motion_ref.moved(part, table, motion_ref.moving_records(part, table))[0]
            span = temporal_ref.tap_columns(cam_prev, part, W, H, before)
            lo, hi = span or (c0, c1)                             # (None: no point of the column is seen; any window does)
            assert 0 <= lo < hi <= W

            def windowed(a, b):
                prev = (cam_prev, np.ascontiguousarray(prev_hits[a:b])) + tuple(np.ascontiguousarray(t[a:b]) for t in history)
                return accumulate(np.ascontiguousarray(cur[c0:c1]), part, cam, prev, x0=c0, W=W, prev_x0=a, **more)

            same_words(windowed(lo, hi), [np.ascontiguousarray(w[c0:c1]) for w in whole], f"columns {c0}:{c1} from {lo}:{hi}")
            windows += int((lo, hi) != (0, W))
            for a, b in ((lo + 1, hi), (lo, hi - 1)):
                if a < b and span:
                    with pytest.raises(IndexError):
                        windowed(a, b)
    assert windows >= 6                                          # (most windows are a few columns, not the frame)


# ---- 4. the conditions on the pose pairs the GPU tests compare ----------------------------------------------------------------------

def classes(name, W, H):
    cam_prev, cam, prev_hits, hits = motion_scenes.records(name, W, H)
    table = motion_scenes.table(name)
    cur = np.zeros((W, H), dtype=F)
    prev = (cam_prev, prev_hits) + made_up_history(1, W, H, 1)
    kw = dict(normal_cos=NORMAL_COS, plane_eps=PLANE_EPS, details=True)
    with_table = motion_ref.accumulate(cur, hits, cam, prev, table, **kw)
    without = motion_ref.accumulate(cur, hits, cam, prev, np.zeros((0, 12), dtype=F), **kw)
    moving = with_table[5]["moving"]
    live = ~temporal_ref.dead_records(hits)
    return dict(movers=int(moving.sum()), movers_with=int((~with_table[4])[moving].sum()), movers_without=int((~without[4])[moving].sum()),
                movers_lost=int(with_table[4][moving].sum()), static_lost=int(with_table[4][live & ~moving].sum()),
                identity=int((with_table[5]["identity"] & ~with_table[4]).sum()), outside=int((with_table[5]["outside"] & moving).sum()))


@pytest.mark.parametrize("size", [(61, 37), (96, 80)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(motion_scenes.PAIRS))
def test_conditions_on_the_compared_pairs(name, size):
    got = classes(name, *size)
    print(name, size, got)
    assert got["movers"] >= 80, got
    assert 4 * got["movers_with"] >= 3 * got["movers"], got
    assert 3 * got["movers_without"] <= 2 * got["movers_with"], got      # the table does something
    assert got["movers_lost"] >= 3 and got["static_lost"] >= 5, got
    if motion_scenes.PAIRS[name][2] == "equal":
        assert got["identity"] >= 500, got
    if name == "sphere_leaves":
        assert got["outside"] >= 3, got                                  # mover pixels whose surface stood outside the frame


# ---- 5. object_motions ----------------------------------------------------------------------------------------------------------------

def surface_distance(obj, points):
    """float64 signed distance of points (n, 3) from the surface of an RtObjectDesc (a plane's: from its plane, along its normal)"""
    p = points.astype(np.float64)
    if obj.kind == 0:
        return np.linalg.norm(p - np.array(list(obj.origin), dtype=np.float64), axis=1) - float(obj.radius)
    n = np.array(list(obj.normal), dtype=np.float64)
    o = np.array(list(obj.plane_origin if obj.kind == 2 else obj.origin), dtype=np.float64)
    return ((p - o) @ n) / np.linalg.norm(n)


@pytest.mark.parametrize("name", sorted(motion_scenes.PAIRS))
def test_object_motions_carry_every_record_point_onto_the_previous_surface(name):
    """For every object and every record point P of the current pose, M P + t (the definition's fp32 operations) lies on the
    previous pose's surface within 16 * 2^-24 * L.  A record point is not on its surface exactly -- the oracle's sphere points
    stand up to 1.5 times that bound off their own sphere, an unmoved one's too, and a plane's stand 1e-3 before it -- and a
    rigid motion keeps a point's signed distance from the surface, so what is held to the bound is the change of that distance:
    for a point on the surface it is the distance from the previous surface itself."""
    W, H = 96, 80
    prev, cur = motion_scenes.host(motion_scenes.PAIRS[name][0]), motion_scenes.host(motion_scenes.PAIRS[name][1])
    table = object_motions(prev.desc, cur.desc)
    assert table.shape == (motion_scenes.N_OBJECTS, 12) and table.dtype == F
    d_prev, d_cur = prev.desc.contents, cur.desc.contents
    hits = motion_scenes.records(name, W, H)[3]
    L = float(max(np.abs(hits["point"]).max(), max(abs(v) for k in range(d_prev.n_objects) for v in d_prev.objects[k].origin)))
    bound = 16 * 2.0 ** -24 * L                                  # twelve rounded coefficients and four operations a component
    moved_objects = 0
    for o in range(motion_scenes.N_OBJECTS):
        mine = (hits["object"] == o) & ~temporal_ref.dead_records(hits)
        same = bytes(d_prev.objects[o]) == bytes(d_cur.objects[o])
        if same:
            assert table[o].tobytes() == motion_ref.IDENTITY.tobytes(), o
        else:
            moved_objects += 1
            assert table[o].tobytes() != motion_ref.IDENTITY.tobytes(), o
        if not mine.any():
            continue
        rec = np.ascontiguousarray(hits[mine])
        Pp, _ = motion_ref.moved(rec, table, np.full(len(rec), not same))
        change = np.abs(surface_distance(d_prev.objects[o], Pp) - surface_distance(d_cur.objects[o], rec["point"])).max()
        print(name, o, "change of the distance / bound", change / bound)
        assert change <= bound, (o, change, bound)
    assert moved_objects >= 2
    # a plane's matrix is a rotation to fp32, a sphere's the identity
    for o in range(motion_scenes.N_OBJECTS):
        R = table[o].reshape(3, 4)[:, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 8 * 2.0 ** -24
        if d_cur.objects[o].kind == 0:
            assert np.array_equal(R, np.eye(3))


def test_object_motions_refuse_mismatched_descs():
    from tilecoderaytracer_amd import HostScene
    a = motion_scenes.host(motion_scenes.REST)
    assert (object_motions(a.desc, a.desc).view(np.uint32) == np.tile(motion_ref.IDENTITY, (14, 1)).view(np.uint32)).all()
    b = motion_scenes.host(motion_scenes.REST)
    b.add_sphere((0.0, 0.0, 5.0), 0.5)
    with pytest.raises(ValueError):
        object_motions(a.desc, b.desc)
    c, d = HostScene.empty(), HostScene.empty()
    c.add_sphere((0.0, 0.0, 5.0), 0.5)
    d.add_infinite_plane((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    with pytest.raises(ValueError):
        object_motions(c.desc, d.desc)
