"""Mirror records (include/rt_mirror.h) without a GPU: the header, the exported symbols, the struct sizes, every argument check
in the header's order (none touches a device or the handle), and mirror_ref -- the tests' restatement of the definition -- held
to what the header says follows from it, so that the GPU tests, which compare against it, cannot pass vacuously: the room of
mirror_scenes.py has chains of every length, the guide of a planar chain is the float64 reflection of its terminal within the
bound DESIGN.md section 27 derives, and the guide records carry a reflected image's history where the G-buffer's cannot."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mirror_ref
import mirror_scenes
import query_ref
import temporal_ref
from tilecoderaytracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_mirror.h")
FUNCTIONS = ["rt_get_mirror_info", "rt_mirror_records", "rt_mirror_records_device", "rt_mirror_version"]
F = np.float32
EPS = 2.0 ** -24


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t|const char \*)\s*(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    assert '#include "rt_capi_query.h"' in text and len(re.findall(r"#include", text)) == 1
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    assert int(re.search(r"#define RT_MIRROR_VERSION (\d+)", text).group(1)) == lib.rt_mirror_version() == 1
    assert int(re.search(r"#define RT_MIRROR_MAX_BOUNCES (\d+)", text).group(1)) == capi.RT_MIRROR_MAX_BOUNCES == 64


def test_struct_sizes_match_the_header(tmp_path):
    P, I = capi.RtMirrorParams, capi.RtMirrorInfo
    assert C.sizeof(P) == 12 and (P.chunk_rays.offset, P.min_reflective.offset) == (4, 8)
    assert C.sizeof(I) == 32 and (I.chunks.offset, I.queries.offset, I.query_ms.offset, I.step_ms.offset) == (8, 12, 16, 24)
    if not shutil.which("gcc"):
        return
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_mirror.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d\\n", (int)sizeof(rt_mirror_params), (int)sizeof(rt_mirror_info),\n'
                   "  (int)offsetof(rt_mirror_info, chunks), (int)offsetof(rt_mirror_info, queries),\n"
                   "  (int)offsetof(rt_mirror_info, query_ms), (int)offsetof(rt_mirror_info, step_ms)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [12, 32, 8, 12, 16, 24]


def test_the_library_gained_the_step_kernel_and_the_unit_shares_the_host_plumbing():
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    names = [line.split()[-1] for line in r.stdout.splitlines() if line.split()]
    assert any("rt_mirror_step_kernel" in n and "__device_stub__" not in n for n in names)
    text = open(os.path.join(ROOT, "tilecoderaytracer_amd", "csrc", "rt_mirror.hip")).read()
    assert '#include "rt_host.h"' in text and "rt_internal_launch_hits" in text and "#pragma clang fp contract(off)" in text
    assert "mirror" not in open(os.path.join(ROOT, "tilecoderaytracer_amd", "csrc", "rt_tables.h")).read()


# ---- 2. the argument checks, in the header's order, without a device ---------------------------------------------------------

NAN = float("nan")
RAYS = np.zeros((4, 6), dtype=F)
ALIGNED, MISALIGNED_16, MISALIGNED_4 = 0x10000, 0x10008, 0x10002         # (device pointers that are only ever looked at)
_FAKE = C.create_string_buffer(1 << 20)                                   # a handle that is not NULL; no check reads it
FAKE_SCENE = C.addressof(_FAKE)
GOOD = dict(max_bounces=3, chunk_rays=0, min_reflective=1.0)
# (the word its message carries, the arguments that fail it), the header's checks (2) .. (10)
ORDER = [("params is NULL", dict(params=None)), ("max_bounces", dict(max_bounces=65)), ("chunk_rays", dict(chunk_rays=-1)),
         ("min_reflective", dict(min_reflective=NAN)), ("n < 0", dict(n=-1)), ("rows", dict(rows=0)),
         ("rays pointer", dict(rays=None)), ("out_hits pointer", dict(hits=None)), ("too large", dict(n=2 ** 31 - 1, rows=1)),
         ("d_rays", dict(rays=MISALIGNED_4)), ("d_out_hits", dict(hits=MISALIGNED_16)), ("d_out_guide", dict(guide=MISALIGNED_16)),
         ("d_out_weight", dict(weight=MISALIGNED_4)), ("d_out_path", dict(path=MISALIGNED_4))]
HOST_CHECKS = 9


def call(a, device):
    lib = capi.load_library()
    p = capi.RtMirrorParams(a["max_bounces"], a["chunk_rays"], a["min_reflective"])
    args = (a.get("scene", FAKE_SCENE), C.byref(p) if a["params"] else None, a["n"], a["rows"], a["rays"], a["hits"], a["guide"],
            a["weight"], a["path"])
    rc = lib.rt_mirror_records_device(*args, None) if device else lib.rt_mirror_records(*args)
    return rc, lib.rt_last_error().decode()


def bad_from(first, last, device):
    """valid arguments with the checks ORDER[first:last] failing together, where they can (an earlier check's bad value wins
    over a later one's for the same argument)"""
    a = dict(GOOD, params=True, n=4, rows=4, rays=ALIGNED if device else RAYS.ctypes.data, hits=ALIGNED, guide=ALIGNED,
             weight=ALIGNED, path=ALIGNED)
    for _, bad in reversed(ORDER[first:last]):
        a.update(bad)
    return a


@pytest.mark.parametrize("device", [False, True])
def test_every_argument_check_comes_before_the_device_in_the_headers_order(device):
    last = len(ORDER) if device else HOST_CHECKS
    for bad, word in ((dict(max_bounces=-1), "max_bounces"), (dict(chunk_rays=-7), "chunk_rays"), (dict(rows=-1), "rows")):
        rc, msg = call(dict(bad_from(last, last, device), **bad), device)
        assert rc == capi.RT_ERR_INVALID and word in msg, (bad, msg)
    for first in range(last):
        word = ORDER[first][0]
        rc, msg = call(bad_from(first, first + 1, device), device)                # alone
        assert rc == capi.RT_ERR_INVALID and word in msg, (first, word, msg)
        rc, msg = call(bad_from(first, last, device), device)                     # with every later one
        assert rc == capi.RT_ERR_INVALID and word in msg, (first, word, msg)
    for first in (0, 5, last - 1):                                                # (1) the scene comes first
        rc, msg = call(dict(bad_from(first, last, device), scene=None), device)
        assert rc == capi.RT_ERR_INVALID and msg == "scene is NULL", (first, msg)
    assert capi.load_library().rt_get_mirror_info(None, C.byref(capi.RtMirrorInfo())) == capi.RT_ERR_INVALID
    # n == 0 is RT_OK and launches nothing, whatever the pointers; the ranges' ends are valid up to the device
    assert call(dict(bad_from(last, last, device), n=0, rays=None, hits=None, guide=None, weight=None, path=None), device)[0] == 0
    for ends in (dict(max_bounces=0, min_reflective=float("-inf")), dict(max_bounces=64, min_reflective=float("inf"))):
        assert call(dict(bad_from(last, last, device), n=0, **ends), device)[0] == capi.RT_OK


# ---- 3. mirror_ref against what the header says follows from the definition ---------------------------------------------------

def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("key", ["builtin", "room"])
def test_without_a_followed_mirror_the_records_are_the_querys(key):
    rays = mirror_scenes.pixel_rays(key, 61, 37)
    plain = query_ref.intersect(mirror_scenes.ref_scene(key), rays)
    for bounces, floor in ((0, 1.0), (3, 1.5)):                                   # no bounce allowed; no object qualifies
        hits, guide, weight, path = mirror_ref.records(mirror_scenes.ref_scene(key), rays, bounces, floor)
        assert same(hits, plain) and same(guide, plain) and (weight == 1).all()
        if bounces == 0:                                                          # only the cut bit, where the first hit is a mirror
            rf = mirror_ref.reflective(mirror_scenes.ref_scene(key))
            first = (plain["object"] >= 0) & ((plain["flags"] & 2) == 0) & (rf[np.clip(plain["object"], 0, None)] >= 1)
            assert first.sum() >= 100 and (path == np.where(first, 0x100, 0)).all()
        else:
            assert (path == 0).all()


@pytest.mark.parametrize("key,floor", [("builtin", 0.5), ("room", 1.0), ("room", 0.5)])
def test_guides_and_tags(key, floor):
    hits, guide, weight, path, d = mirror_scenes.reference(key, 61, 37, 3, floor)
    k, cut, tag = mirror_ref.unpack(path)
    n_objects = len(mirror_scenes.ref_scene(key).objects)
    assert (k == d["k"]).all() and (cut == d["cut"]).all() and k.max() == 3 and (k >= 1).sum() > 100
    assert same(guide[k == 0], hits[k == 0]) and (tag[k == 0] == 0).all()          # no mirror followed: the terminal's bits
    followed = (k >= 1) & (hits["object"] >= 0)
    ids = guide["object"][followed]
    assert (ids >= 0).all() and (ids >= 4096).all() and n_objects < 4096           # tagged: >= 0 and no true index
    assert ((ids & 0xfff) == hits["object"][followed]).all() and ((ids >> 12) == tag[followed]).all()
    assert ((tag[k >= 1] >= 1) & (tag[k >= 1] <= 0x7fffe)).all()
    # chains that followed other mirrors, or the same in another order, carry other tags (no collision in these frames)
    chains = {}
    for t, c in zip(tag[k >= 1].tolist(), d["chain"][k >= 1].tolist()):
        assert chains.setdefault(t, c) == c
    assert len(set(map(tuple, chains.values()))) == len(chains) >= 2
    assert same(guide["color"], hits["color"]) and same(guide["flags"], hits["flags"])
    assert cut[k < 3].sum() == 0 and (weight[k == 0] == 1).all()


def test_the_room_has_chains_of_every_length():
    _, _, _, path, _ = mirror_scenes.reference("room", 61, 37, 3, 1.0)
    k, cut, _ = mirror_ref.unpack(path)
    assert (k == 1).sum() >= 200 and (k >= 2).sum() >= 50 and cut.sum() >= 10 and (k == 0).sum() >= 200
    assert len(mirror_scenes.ref_scene("room").objects) <= 40


def reflect64(scene, chain, point, normal):
    """the float64 reflection of terminal points and normals back through their chains' mirror planes, last mirror first"""
    p, n = point.astype(np.float64), normal.astype(np.float64)
    for s in range(chain.shape[1] - 1, -1, -1):
        for o in np.unique(chain[:, s]):
            if o < 0:
                continue
            ob = scene.objects[o]
            m = np.array([ob.normal.x, ob.normal.y, ob.normal.z], dtype=np.float64)
            sel = chain[:, s] == o
            p[sel] -= (2.0 * ((p[sel] @ m) + float(ob.distance_to_origin)) / (m @ m))[:, None] * m
            n[sel] -= (2.0 * (n[sel] @ m) / (m @ m))[:, None] * m
    return p, n


@pytest.mark.parametrize("W,H", mirror_scenes.SIZES)
@pytest.mark.parametrize("floor", [1.0, 0.5])
def test_a_planar_chains_guide_is_its_terminal_reflected_through_the_mirrors(W, H, floor):
    """unfolded through its mirrors a chain is the straight line E + t d0, but for one step of 1e-3 along
    a normal at each of its k mirrors and at a planar terminal (the records' point offsets), and fp32 rounding: a direction
    remade from {P, P + r} is off by 2 eps (1 + |P|) and carried over at most L, the rest is a few eps of the coordinates.
        |guide.point - reflected| <= (k + 1) (1.01e-3 + 8 eps (1 + EXTENT) (1 + L)),  eps = 2^-24
        |guide.normal - reflected| <= (k + 1) 32 eps"""
    scene = mirror_scenes.ref_scene("room")
    hits, guide, _, path, d = mirror_scenes.reference("room", W, H, 3, floor)
    k = d["k"]
    kinds = np.array([o.kind for o in scene.objects])
    planar = (k >= 1) & (hits["object"] >= 0) & (np.where(d["chain"] >= 0, kinds[np.clip(d["chain"], 0, None)], 1) != 0).all(-1)
    assert planar.sum() >= 200 and (k[planar] >= 2).sum() >= 50
    p, n = reflect64(scene, d["chain"][planar], hits["point"][planar], hits["normal"][planar])
    steps = (k[planar] + 1).astype(np.float64)
    L = guide["distance"][planar].astype(np.float64)
    dp = np.abs(guide["point"][planar] - p).max(-1)
    dn = np.abs(guide["normal"][planar] - n).max(-1)
    bound_p = steps * (1.01e-3 + 8 * EPS * (1 + mirror_scenes.EXTENT) * (1 + L))
    print(f"point: worst {dp.max():.3e} of its bound {bound_p[dp.argmax()]:.3e}; normal: worst {dn.max():.3e} of {32 * EPS * steps.max():.3e}")
    assert (dp <= bound_p).all() and (dn <= steps * 32 * EPS).all()
    assert np.abs(hits["point"][planar]).max() <= mirror_scenes.EXTENT


def signal(points, cells):
    """a view-independent value on a surface point: the parity of floor(cells * point) summed over the axes"""
    return (np.floor(points * F(cells)).sum(-1) % 2).astype(F)


def history_error(records, values, k2):
    """two frames under the room's two cameras through temporal_ref -> the mean |accumulated - frame 2's own value| over the
    pixels of frame 2 that followed a mirror"""
    cams = mirror_scenes.room_cameras()
    v1, m1, l1, _, _ = temporal_ref.accumulate(values[0], records[0], cams[0])
    v2 = temporal_ref.accumulate(values[1], records[1], cams[1], prev=(cams[0], records[0], v1, m1, l1))[0]
    return float(np.abs(v2 - values[1])[k2 >= 1].mean())


def test_guide_records_carry_the_history_of_a_reflected_image():
    """The payoff.  The signal lives on the terminal's real point, so a correct history of a static
    scene agrees with the frame's own value.  Its cells are 1 unit: a reflected image lies 12 to 40 units along its path, where
    a 61-pixel-wide frame resolves a 1-unit cell with 1.5 to 5 pixels; at 4 cells a unit they are below a pixel and both kinds of
    record only measure aliasing (0.236 and 0.231).  Guide records: 0.081; plain G-buffer records: 0.259."""
    W, H = mirror_scenes.SIZES[0]
    frames = [mirror_scenes.reference("room", W, H, 3, 1.0, camera) for camera in (0, 1)]
    plain = [mirror_scenes.reference("room", W, H, 0, 1.0, camera)[0] for camera in (0, 1)]
    values = [signal(f[0]["point"], 1) for f in frames]
    k2 = frames[1][4]["k"]
    assert (k2 >= 1).sum() >= 400
    with_guide = history_error([f[1] for f in frames], values, k2)
    with_plain = history_error(plain, values, k2)
    print(f"guide records {with_guide:.4f}, G-buffer records {with_plain:.4f}")
    assert with_plain > 0.1 and with_guide <= 0.5 * with_plain
