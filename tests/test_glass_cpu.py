"""Glass records (include/rt_glass.h) without a GPU: the header, the exported symbols, the struct sizes, every argument check in
the header's order (none touches a device or the handle), and glass_ref -- the tests' restatement of the definition -- held to
what the header says follows from it, so that the GPU tests, which compare against it, cannot pass vacuously: it is mirror_ref
where nothing is looked through, the room of glass_scenes.py has chains of every kind, the first child is refract_ref's, the
guide through panes and planar mirrors is the float64 unfolding of its terminal within the bound DESIGN.md section 29 derives,
and the guide records carry the history of what stands behind a window where the G-buffer's cannot.  Section 4 holds the
reference to the scenes "edges" and "open" -- every category of ray that the GPU tests on them are there for is present, by
count -- and pins the chains of the batch test_glass_large_gpu.py tiles."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import glass_ref
import glass_scenes
import mirror_large
import mirror_ref
import query_ref
import refract_ref
import temporal_ref
from tilecoderaytracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_glass.h")
FUNCTIONS = ["rt_get_glass_info", "rt_glass_records", "rt_glass_records_device", "rt_glass_version"]
F = np.float32
EPS = 2.0 ** -24
INF = float("inf")
W61, H37 = glass_scenes.SIZES[0]
BOUNCES = 4


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t|const char \*)\s*(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    assert '#include "rt_mirror.h"' in text and len(re.findall(r"#include", text)) == 1
    for name in FUNCTIONS + re.findall(r"\b(rt_glass\w*)\b", text):
        assert "glass" in name and not re.fullmatch(r"rt_\w*mirror\w*", name), name
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    assert int(re.search(r"#define RT_GLASS_VERSION (\d+)", text).group(1)) == lib.rt_glass_version() == 1


def test_struct_sizes_match_the_header(tmp_path):
    P, I = capi.RtGlassParams, capi.RtGlassInfo
    assert C.sizeof(P) == 16 and (P.chunk_rays.offset, P.min_reflective.offset, P.min_transmissive.offset) == (4, 8, 12)
    assert C.sizeof(I) == 32 and (I.chunks.offset, I.queries.offset, I.query_ms.offset, I.step_ms.offset) == (8, 12, 16, 24)
    assert [(n, t) for n, t in I._fields_] == [(n, t) for n, t in capi.RtMirrorInfo._fields_]
    if not shutil.which("gcc"):
        return
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_glass.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d %d %d %d\\n", (int)sizeof(rt_glass_params), (int)sizeof(rt_glass_info),\n'
                   "  (int)offsetof(rt_glass_params, chunk_rays), (int)offsetof(rt_glass_params, min_reflective),\n"
                   "  (int)offsetof(rt_glass_params, min_transmissive),\n"
                   "  (int)offsetof(rt_glass_info, chunks), (int)offsetof(rt_glass_info, queries),\n"
                   "  (int)offsetof(rt_glass_info, query_ms), (int)offsetof(rt_glass_info, step_ms)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [16, 32, 4, 8, 12, 8, 12, 16, 24]


def test_the_library_gained_the_glass_step_and_the_unit_shares_the_host_plumbing():
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    names = [line.split()[-1] for line in r.stdout.splitlines() if line.split()]
    steps = [n for n in names if "rt_glass_step_kernel" in n and "__device_stub__" not in n]
    assert len(steps) == 4, steps                                              # FIRST x GUIDE, in place
    csrc = os.path.join(ROOT, "tilecoderaytracer_amd", "csrc")
    text = open(os.path.join(csrc, "rt_glass.hip")).read()
    assert '#include "rt_host.h"' in text and "rt_internal_launch_hits" in text and "#pragma clang fp contract(off)" in text
    assert "rt_mirror_check_args" in text and "RT_INTERNAL_UNIT_GLASS" in text and "hipStreamSynchronize" not in text
    body = open(os.path.join(csrc, "rt_mirror_body.h")).read()
    assert len(re.findall(r"\bint rt_mirror_check_args\(", body)) == 1         # one copy of the checks


# ---- 2. the argument checks, in the header's order, without a device ---------------------------------------------------------

NAN = float("nan")
RAYS = np.zeros((4, 6), dtype=F)
ALIGNED, MISALIGNED_16, MISALIGNED_4 = 0x10000, 0x10008, 0x10002         # (device pointers that are only ever looked at)
_FAKE = C.create_string_buffer(1 << 20)                                   # a handle that is not NULL; no check reads it
FAKE_SCENE = C.addressof(_FAKE)
GOOD = dict(max_bounces=3, chunk_rays=0, min_reflective=1.0, min_transmissive=0.5)
# (the word its message carries, the arguments that fail it), the header's checks (2) .. (10)
ORDER = [("params is NULL", dict(params=None)), ("max_bounces", dict(max_bounces=65)), ("chunk_rays", dict(chunk_rays=-1)),
         ("min_reflective", dict(min_reflective=NAN)), ("min_transmissive", dict(min_transmissive=NAN)), ("n < 0", dict(n=-1)),
         ("rows", dict(rows=0)), ("rays pointer", dict(rays=None)), ("out_hits pointer", dict(hits=None)),
         ("too large", dict(n=2 ** 31 - 1, rows=1)), ("d_rays", dict(rays=MISALIGNED_4)), ("d_out_hits", dict(hits=MISALIGNED_16)),
         ("d_out_guide", dict(guide=MISALIGNED_16)), ("d_out_weight", dict(weight=MISALIGNED_4)),
         ("d_out_path", dict(path=MISALIGNED_4))]
HOST_CHECKS = 10


def call(a, device):
    lib = capi.load_library()
    p = capi.RtGlassParams(a["max_bounces"], a["chunk_rays"], a["min_reflective"], a["min_transmissive"])
    args = (a.get("scene", FAKE_SCENE), C.byref(p) if a["params"] else None, a["n"], a["rows"], a["rays"], a["hits"], a["guide"],
            a["weight"], a["path"])
    rc = lib.rt_glass_records_device(*args, None) if device else lib.rt_glass_records(*args)
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
    assert capi.load_library().rt_get_glass_info(None, C.byref(capi.RtGlassInfo())) == capi.RT_ERR_INVALID
    # n == 0 is RT_OK and launches nothing, whatever the pointers; the ranges' ends are valid up to the device
    assert call(dict(bad_from(last, last, device), n=0, rays=None, hits=None, guide=None, weight=None, path=None), device)[0] == 0
    for ends in (dict(max_bounces=0, min_reflective=-INF, min_transmissive=-INF),
                 dict(max_bounces=64, min_reflective=INF, min_transmissive=INF)):
        assert call(dict(bad_from(last, last, device), n=0, **ends), device)[0] == capi.RT_OK


# ---- 3. glass_ref against what the header says follows from the definition ----------------------------------------------------

def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize("key,floor,look", [("glass", 1.0, INF), ("glass", 0.5, INF), ("room", 1.0, 0.5), ("room", 0.5, 0.0)])
def test_where_nothing_is_looked_through_the_records_are_the_mirror_calls(key, floor, look):
    """min_transmissive = +inf on the glass room, and any value on the non-refractive room: mirror_ref word for word"""
    scene, rays = glass_scenes.ref_scene(key), glass_scenes.pixel_rays(key, W61, H37)
    for bounces in (0, 1, BOUNCES):
        got = glass_ref.records(scene, rays, bounces, floor, look)
        want = mirror_ref.records(scene, rays, bounces, floor)
        assert all(same(g, w) for g, w in zip(got, want)), (key, floor, look, bounces)
        assert (mirror_ref.unpack(want[3])[0] >= 1).sum() >= (100 if bounces else 0)


def kinds_of(d):
    """masks of the chain kinds of a reference's details: pane only, through a sphere, pane then mirror, mirror then pane"""
    ch, gl = d["chain"], d["glass"]
    first, second = ch[..., 0], ch[..., 1]
    pane_only = (d["k"] == 1) & (first == glass_scenes.PANE) & gl[..., 0]
    sphere = (((ch == glass_scenes.GLASS_SPHERE) | (ch == glass_scenes.BUBBLE)) & gl).any(-1)
    pane_mirror = (first == glass_scenes.PANE) & gl[..., 0] & (second >= 0) & ~gl[..., 1]
    mirror_pane = (first >= 0) & ~gl[..., 0] & (second == glass_scenes.PANE) & gl[..., 1]
    return pane_only, sphere, pane_mirror, mirror_pane


def test_the_glass_room_has_chains_of_every_kind():
    hits, guide, weight, path, d = glass_scenes.reference("glass", W61, H37, BOUNCES, 1.0, 0.5)
    k, cut, g, tag = glass_ref.unpack(path)
    assert (k == d["k"]).all() and (cut == d["cut"]).all() and (g == d["g"]).all() and (path & 0x200 == 0).all()
    counts = [int(m.sum()) for m in kinds_of(d)]
    print("pane only, sphere, pane then mirror, mirror then pane:", counts)
    assert min(counts) >= 20, counts
    childless = d["childless"] > 0                                             # the bubble's rim: total reflection, no child
    assert childless.sum() >= 5 and (hits["object"][childless & (k == 0)] == glass_scenes.BUBBLE).sum() >= 5
    assert (cut & g).sum() >= 1 and (k[cut] == BOUNCES).all()
    assert (g == d["glass"].any(-1)).all() and (g <= (k >= 1)).all()
    # a tagged guide where anything was followed, and tags that tell a pane looked through from nothing followed
    followed = (k >= 1) & (hits["object"] >= 0)
    assert ((guide["object"][followed] & 0xfff) == hits["object"][followed]).all() and (guide["object"][followed] >= 4096).all()
    assert same(guide[k == 0], hits[k == 0]) and (weight[k == 0] == 1).all() and (tag[k == 0] == 0).all()
    assert same(guide["color"], hits["color"]) and same(guide["flags"], hits["flags"])
    assert len(glass_scenes.ref_scene("glass").objects) <= 40


def test_glass_wins_over_mirror_and_a_childless_candidate_falls_to_the_mirror_rule():
    """min_reflective 0.05: the pane (rf 0.1) qualifies as a mirror too and is still looked through; with the bubble made a
    mirror, its rim -- candidates without a child -- reflects"""
    scene, rays = glass_scenes.ref_scene("glass"), glass_scenes.pixel_rays("glass", W61, H37)
    *_, d = glass_ref.records(scene, rays, 2, 0.05, 0.5, details=True)
    first_pane = d["chain"][..., 0] == glass_scenes.PANE
    assert first_pane.sum() >= 100 and d["glass"][..., 0][first_pane].all()
    orc, refr = glass_scenes.oracle_scene("glass")
    orc.set_reflective(glass_scenes.BUBBLE, 1.0)
    shiny = refract_ref.Scene(orc, {o: (tf, ior) for o, tf, ior in refr})
    *_, d = glass_ref.records(shiny, rays, 2, 1.0, 0.5, details=True)
    rim = (d["childless"] > 0) & (d["chain"][..., 0] == glass_scenes.BUBBLE)
    assert rim.sum() >= 5 and not d["glass"][..., 0][rim].any()


def test_the_first_child_is_the_render_paths():
    """The child of every pixel ray whose first hit is a candidate, against refract_ref.transmitted fed as refract_ref's render
    path feeds it -- _nearest's raw normal, not the header's normalize(P - centre): the origins agree bit for bit, and the
    rays without a child are the same."""
    scene = glass_scenes.ref_scene("glass")
    rays = np.ascontiguousarray(glass_scenes.pixel_rays("glass", W61, H37)).reshape(-1, 6)
    d = glass_scenes.reference("glass", W61, H37, BOUNCES, 1.0, 0.5)[4]
    E, dirs = rays[:, :3].copy(), query_ref.directions(rays)
    idx, t, P, N, _ = refract_ref._nearest(scene, E, dirs)
    first = d["first"].reshape(-1, 3)
    checked = 0
    for o, (tf, ior) in scene.refractive.items():
        sel = np.nonzero(idx == o)[0]
        ok, origin, _ = refract_ref.transmitted(scene.objects[o], E[sel], dirs[sel], t[sel], P[sel], N[sel], ior)
        assert same(first[sel][ok], origin[ok]) and np.isnan(first[sel][~ok]).all(), o
        assert (d["childless"].reshape(-1)[sel][~ok] >= 1).all()
        checked += int(ok.sum())
    assert checked >= 500


def unfold64(scene, chain, glass, point, normal):
    """the float64 unfolding of terminal points and normals back through their chains, last step first: reflected through a
    mirror's plane, unchanged through a pane"""
    p, n = point.astype(np.float64), normal.astype(np.float64)
    for s in range(chain.shape[1] - 1, -1, -1):
        for o in np.unique(chain[:, s]):
            if o < 0:
                continue
            ob = scene.objects[o]
            m = np.array([ob.normal.x, ob.normal.y, ob.normal.z], dtype=np.float64)
            sel = (chain[:, s] == o) & ~glass[:, s]
            p[sel] -= (2.0 * ((p[sel] @ m) + float(ob.distance_to_origin)) / (m @ m))[:, None] * m
            n[sel] -= (2.0 * (n[sel] @ m) / (m @ m))[:, None] * m
    return p, n


@pytest.mark.parametrize("W,H", glass_scenes.SIZES)
@pytest.mark.parametrize("floor", [1.0, 0.5])
def test_through_panes_and_planar_mirrors_the_guide_is_the_terminal_unfolded(W, H, floor):
    """a pane restarts the ray at ip + N' 1e-3 with d unchanged, so what the straight line E + L d0 misses
    per pane is the vector N' 1e-3 -- the same 1e-3 a mirror's or a planar terminal's point offset costs in section 27 -- and
    the remade direction's rounding is carried as there.  The mirror test's bound holds unchanged:
        |guide.point - unfolded| <= (k + 1) (1.01e-3 + 8 eps (1 + EXTENT) (1 + L)),  eps = 2^-24
        |guide.normal - unfolded| <= (k + 1) 32 eps"""
    scene = glass_scenes.ref_scene("glass")
    hits, guide, _, path, d = glass_scenes.reference("glass", W, H, BOUNCES, floor, 0.5)
    k = d["k"]
    kinds = np.array([o.kind for o in scene.objects])
    planar = (k >= 1) & (hits["object"] >= 0) & (np.where(d["chain"] >= 0, kinds[np.clip(d["chain"], 0, None)], 1) != 0).all(-1)
    through = planar & d["g"]
    assert through.sum() >= 400 and (k[through] >= 2).sum() >= 100
    p, n = unfold64(scene, d["chain"][planar], d["glass"][planar], hits["point"][planar], hits["normal"][planar])
    steps = (k[planar] + 1).astype(np.float64)
    L = guide["distance"][planar].astype(np.float64)
    dp = np.abs(guide["point"][planar] - p).max(-1)
    dn = np.abs(guide["normal"][planar] - n).max(-1)
    bound_p = steps * (1.01e-3 + 8 * EPS * (1 + glass_scenes.EXTENT) * (1 + L))
    print(f"point: worst {dp.max():.3e} of its bound {bound_p[dp.argmax()]:.3e}; normal: worst {dn.max():.3e} of {32 * EPS * steps.max():.3e}")
    assert (dp <= bound_p).all() and (dn <= steps * 32 * EPS).all()
    assert np.abs(hits["point"][planar]).max() <= glass_scenes.EXTENT
    # through panes alone: the guide's point is the terminal's own, and its normal the terminal's bits
    panes = planar & (d["glass"] | (d["chain"] < 0)).all(-1)
    assert panes.sum() >= 200 and same(guide["normal"][panes], hits["normal"][panes])


def signal(points, cells):
    """a view-independent value on a surface point: the parity of floor(cells * point) summed over the axes"""
    return (np.floor(points * F(cells)).sum(-1) % 2).astype(F)


def test_guide_records_carry_the_history_of_what_stands_behind_the_window():
    """The payoff, as test_mirror_cpu.py holds it for mirrors.  The signal lives on the terminal's real
    point, so a correct history of a static scene agrees with the frame's own value; under the trucked camera the G-buffer's
    records reproject the pane's plane, which is pure parallax error.  Over the pixels of frame 2 seen through the pane alone:
    guide records 0.032, plain G-buffer records 0.303."""
    W, H = glass_scenes.SIZES[0]
    frames = [glass_scenes.reference("glass", W, H, BOUNCES, 1.0, 0.5, camera) for camera in (0, 1)]
    plain = [glass_scenes.reference("glass", W, H, 0, 1.0, 0.5, camera)[0] for camera in (0, 1)]
    values = [signal(f[0]["point"], 1) for f in frames]
    d2 = frames[1][4]
    seen = (d2["k"] >= 1) & ((d2["chain"] == glass_scenes.PANE) | (d2["chain"] < 0)).all(-1) & (d2["glass"] | (d2["chain"] < 0)).all(-1)
    assert seen.sum() >= 200
    cams = glass_scenes.room_cameras()

    def history_error(records):
        v1, m1, l1, _, _ = temporal_ref.accumulate(values[0], records[0], cams[0])
        v2 = temporal_ref.accumulate(values[1], records[1], cams[1], prev=(cams[0], records[0], v1, m1, l1))[0]
        return float(np.abs(v2 - values[1])[seen].mean())

    with_guide, with_plain = history_error([f[1] for f in frames]), history_error(plain)
    print(f"guide records {with_guide:.4f}, G-buffer records {with_plain:.4f}")
    assert with_plain > 0.1 and with_guide <= 0.5 * with_plain


# ---- 4. the scenes that hold the step to the rule's edges: what test_glass_gpu.py's cases on them rely on ---------------------

def words_of(out):
    """every 32-bit word of a reference's four outputs, in one array"""
    return np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint32) for a in out[:4]])


def no_nan(out):
    """no float of a reference's outputs is a NaN, whose bits a kernel need not give"""
    floats = [out[0][f] for f in ("distance", "point", "normal", "color")] + [out[1][f] for f in ("distance", "point", "normal", "color")]
    return not any(np.isnan(a).any() for a in floats + [out[2]])


def edges(floor, look, bounces=BOUNCES):
    return glass_scenes.reference("edges", W61, H37, bounces, floor, look)


@pytest.mark.parametrize("floor", glass_scenes.EDGES_FLOORS)
def test_edges_every_threshold_moves_words_one_ulp_above_it_and_none_at_equality(floor):
    """tf >= min_transmissive: with min_transmissive ON a tf the words are those of the look below it, and one ulp above they
    are not; tf > 0: nothing changes among -inf, -1, 0 and the smallest tf, although the red sphere is listed with tf 0"""
    below = words_of(edges(floor, -INF))
    for look in (-1.0, 0.0):
        assert (words_of(edges(floor, look)) == below).all(), (floor, look)
    assert glass_scenes.EDGES_LOOKS[:3] == (-INF, -1.0, 0.0) and len(glass_scenes.EDGES_LOOKS) == 14
    for tf in glass_scenes.EDGES_TF:
        assert glass_scenes.up(tf) in glass_scenes.EDGES_LOOKS and F(glass_scenes.up(tf)) > F(tf) == F(tf)
        assert (words_of(edges(floor, tf)) == below).all(), (floor, tf)
        above = edges(floor, glass_scenes.up(tf))
        changed, paths = int((words_of(above) != below).sum()), int((above[3] != edges(floor, tf)[3]).sum())
        print(f"floor {floor}: across tf {tf}, {changed} words change, {paths} of them path words")
        assert changed >= 30 and paths >= 30, (floor, tf, changed, paths)
        assert no_nan(above)
        below = words_of(above)
    assert (words_of(edges(floor, INF)) == below).all()
    scene, rays = glass_scenes.ref_scene("edges"), glass_scenes.pixel_rays("edges", W61, H37)
    assert (words_of(mirror_ref.records(scene, rays, BOUNCES, floor)) == below).all()


def edge_kinds(scene, out, floor, look):
    """masks over the rays of a reference on "edges": an object that qualifies as glass and as a mirror followed as glass; a
    candidate without a child followed as a mirror (a candidate not followed as glass had no child); the chain ended, not cut,
    on the sphere listed with tf 0; the infinite floor looked through; the ior-1 sphere looked through"""
    hits, d = out[0], out[4]
    rf, (tf, _) = mirror_ref.reflective(scene), glass_ref.transmissive(scene)
    ch, gl = d["chain"], d["glass"]
    o = np.clip(ch, 0, None)
    candidate = (ch >= 0) & (tf[o] > 0) & (tf[o] >= F(look))
    qualifies = (ch >= 0) & (rf[o] >= F(floor))
    return dict(both=(candidate & qualifies & gl).any(-1), fell=(candidate & ~gl).any(-1),
                tf0=(hits["object"] == glass_scenes.RED_SPHERE) & ~d["cut"],
                floor=((ch == glass_scenes.FLOOR) & gl).any(-1), clear=((ch == glass_scenes.CLEAR_SPHERE) & gl).any(-1))


@pytest.mark.parametrize("floor", glass_scenes.EDGES_FLOORS)
def test_edges_has_rays_of_every_category(floor):
    scene = glass_scenes.ref_scene("edges")
    assert scene.objects[glass_scenes.FLOOR].kind == query_ref.INFINITE_PLANE
    assert scene.refractive[glass_scenes.RED_SPHERE][0] == 0 and scene.refractive[glass_scenes.CLEAR_SPHERE][1] == 1.0
    for look in (-INF, 0.2, 0.3):
        out = edges(floor, look)
        kinds = edge_kinds(scene, out, floor, look)
        counts = {name: int(m.sum()) for name, m in kinds.items()}
        print(f"floor {floor} look {look}:", counts)
        assert counts["both"] >= 100 and counts["fell"] >= 20 and counts["clear"] >= 20, counts
        assert counts["floor"] >= 50 or look > 0.2, counts                    # (the floor's tf is 0.2)
        assert (out[4]["childless"][kinds["fell"]] >= 1).all() and glass_ref.unpack(out[3])[2][kinds["both"]].all()
        if look == -INF:
            assert counts["tf0"] >= 50, counts


def test_through_the_ior_1_sphere_the_child_keeps_the_rays_direction():
    """eta = 1: k1 = 1 - (1 - c1 c1) is c1 c1 up to roundings, T1 is d up to roundings, and so is T2.  The pixel rays whose first
    hit is the ior-1 sphere, and the header's step 5 of them: D against d, in units of the float32 spacing at 1 (2^-23; the
    components of a unit vector are no larger)"""
    scene = glass_scenes.ref_scene("edges")
    d = edges(0.5, 0.2)[4]
    first = ((d["chain"][..., 0] == glass_scenes.CLEAR_SPHERE) & d["glass"][..., 0]).reshape(-1)
    assert first.sum() >= 20
    rays = np.ascontiguousarray(glass_scenes.pixel_rays("edges", W61, H37)).reshape(-1, 6)[first]
    dirs = query_ref.directions(rays)
    h = query_ref.intersect(scene, rays)
    assert (h["object"] == glass_scenes.CLEAR_SPHERE).all()
    exists, O, D, s = glass_ref.child(scene, h, rays[:, :3].copy(), dirs, glass_ref.transmissive(scene)[1])
    assert exists.all() and same(O, d["first"].reshape(-1, 3)[first]) and (s > 0).all()
    worst = float(np.abs(D.astype(np.float64) - dirs.astype(np.float64)).max() / 2.0 ** -23)
    print(f"ior 1: {int(first.sum())} rays, D differs from d by at most {worst:.2f} ulp")
    assert worst <= 4.0


@pytest.mark.parametrize("bounces,missed,behind_glass,twice", [(1, 400, 300, None), (3, 700, 500, 200)])
def test_open_has_followed_chains_that_end_in_a_miss(bounces, missed, behind_glass, twice):
    """object < 0 with k >= 1: the guide is the record itself, and the weight and the tag are carried"""
    hits, guide, weight, path, d = glass_scenes.reference("open", W61, H37, bounces, 1.0, 0.5)
    k, cut, g, tag = glass_ref.unpack(path)
    follow = k >= 1
    miss = follow & (hits["object"] < 0)
    counts = (int(follow.sum()), int(miss.sum()), int((miss & g).sum()), int((miss & (k >= 2)).sum()))
    print(f"open, max_bounces {bounces}: follow something, end in a miss, after glass, with k >= 2:", counts)
    assert counts[0] >= counts[1] >= missed and counts[2] >= behind_glass and (twice is None or counts[3] >= twice)
    assert same(guide[miss], hits[miss]) and ((path[miss] & 0xff) >= 1).all() and (tag[miss] >= 1).all() and not cut[miss].any()
    assert (weight[miss & g] != 1).any(-1).all()
    assert no_nan((hits, guide, weight))


def test_the_large_batchs_reference_is_what_the_large_test_relies_on():
    """test_glass_large_gpu.py's preconditions, which it asserts again before its first launch"""
    rays, words, details = glass_scenes.large_tile()
    assert mirror_large.TILE_RAYS == len(rays) == 7679
    assert [w.shape for w in words.values()] == [(7679, 12), (7679, 12), (7679, 3), (7679, 1)]
    assert glass_scenes.large_tile_figures(words, details) == glass_scenes.LARGE_FIGURES
    assert glass_scenes.LARGE_FIGURES == dict(alive=[7679, 5319, 2632, 1039, 577, 288, 148, 111, 64], cut=47, g=3495,
                                              glass_steps=[3007, 288, 367, 177, 76, 55, 24, 23], glass_sphere=627, bubble=123,
                                              childless=85)


def test_the_stated_deviation_is_reported():
    """follow_d traces a child along D itself, as the render does; the header traces normalize((O + D) - O).  The share of
    pixels whose terminal object differs carries no bar (DESIGN.md section 29 reports it: 0 of 2257 and 0 of 7680)."""
    scene = glass_scenes.ref_scene("glass")
    for W, H in glass_scenes.SIZES:
        rays = glass_scenes.pixel_rays("glass", W, H)
        ours = glass_scenes.reference("glass", W, H, BOUNCES, 1.0, 0.5)
        theirs = glass_ref.records(scene, rays, BOUNCES, 1.0, 0.5, follow_d=True)
        differ = int((ours[0]["object"] != theirs[0]["object"]).sum())
        print(f"{W} x {H}: terminal object differs under follow_d in {differ} of {W * H} pixels")
        first = glass_ref.unpack(ours[3])[0] == 0                              # (no child traced: the switch changes nothing)
        assert same(ours[0][first], theirs[0][first]) and same(ours[3][first], theirs[3][first])
