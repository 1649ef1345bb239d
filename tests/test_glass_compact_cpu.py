"""Compact glass records (include/rt_glass_compact.h) without a GPU: the header, the exported symbols, the info struct's layout,
every argument check held to rt_glass_records*' code and message for the same bad arguments (none touches a device or the
handle), rt_glass.h and the two older step kernels left as they were, the new unit's shape in its source -- one decision function
that the count kernel and the step kernel both call, the mirror unit's scan and no second one -- and the preconditions of
test_glass_compact_gpu.py held on the reference, so that those tests cannot pass vacuously: the numbers of live rays per query
fall from several workgroups to less than a wavefront, "open" is empty at query 4, and the batches hold the rays on which the
count and the step must agree about a child's existence: candidates without a child that go on as mirrors, and ones that end."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import glass_ref
import glass_scenes
import mirror_ref
from tilecoderaytracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "tilecoderaytracer_amd", "csrc")
HEADER = os.path.join(INCLUDE, "rt_glass_compact.h")
FUNCTIONS = ["rt_get_glass_compact_info", "rt_glass_compact_version", "rt_glass_records_compact", "rt_glass_records_compact_device"]
OLD_FUNCTIONS = ["rt_get_glass_info", "rt_glass_records", "rt_glass_records_device", "rt_glass_version"]
F = np.float32
INF = float("inf")
# rt_glass_compact_info: (field, offset), 568 bytes -- rt_mirror_compact_info's
LAYOUT = [("rays", 0), ("rays_queried", 8), ("chunks", 16), ("queries", 20), ("syncs", 24), ("reserved", 28), ("query_ms", 32),
          ("step_ms", 40), ("alive", 48)]


def declared(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return text, sorted(set(re.findall(r"^\s*(?:int|uint64_t|const char \*)\s*(rt_\w+)\s*\(", text, flags=re.M)))


def exported():
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    return [line.split()[-1] for line in r.stdout.splitlines() if line.split()]


# ---- 1, 2. the header and the library -----------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_includes_only_rt_glass_h():
    text, names = declared(HEADER)
    assert names == FUNCTIONS
    assert re.findall(r"#include\s*(\S+)", text) == ['"rt_glass.h"']
    assert int(re.search(r"#define RT_GLASS_COMPACT_VERSION (\d+)", text).group(1)) == 1
    said = open(HEADER).read()
    assert "waits" in said.lower() and "capturing" in said and "at most max_bounces waits a chunk" in said     # the syncs
    assert "EARLY END" in said and "217" in said and "1 237 029" in said                          # the early end, the scratch
    assert "NOT tested" in said and "2^32" in said


def test_the_library_exports_the_four_functions_and_the_version_is_1():
    lib = capi.load_library()
    names = exported()
    assert sorted(n for n in names if re.fullmatch(r"rt_\w*glass\w*compact\w*", n)) == FUNCTIONS      # and nothing else of its own
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    assert lib.rt_glass_compact_version() == 1
    kernels = [n for n in names if "__device_stub__" not in n]
    assert len([n for n in kernels if "rt_glass_compact_step_kernel" in n]) == 4           # FIRST x GUIDE
    assert len([n for n in kernels if "rt_glass_compact_count_kernel" in n]) == 1


# ---- 3. the info struct -------------------------------------------------------------------------------------------------------

def test_the_info_struct_is_568_bytes_with_the_mirror_compact_layout(tmp_path):
    I = capi.RtGlassCompactInfo
    assert C.sizeof(I) == 568 and [(n, getattr(I, n).offset) for n, _ in LAYOUT] == LAYOUT
    assert I.alive.size == 8 * (capi.RT_MIRROR_MAX_BOUNCES + 1) == 520
    assert [(n, t) for n, t in I._fields_] == [(n, t) for n, t in capi.RtMirrorCompactInfo._fields_]
    said = open(HEADER).read()
    for name, offset in LAYOUT:
        assert re.search(r"\b%s at %d\b" % (name, offset), said), (name, offset)
    if not shutil.which("gcc"):
        return
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_glass_compact.h"\n'
                   'int main(void) { rt_glass_compact_info i; printf("%d %d", (int)sizeof i, (int)sizeof i.alive);\n' +
                   "".join(f'  printf(" %d", (int)offsetof(rt_glass_compact_info, {n}));\n' for n, _ in LAYOUT) +
                   '  printf(" %d %d\\n", RT_GLASS_COMPACT_VERSION, (int)sizeof(rt_glass_params)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [568, 520] + [o for _, o in LAYOUT] + [1, 16]


# ---- 4. the argument checks are rt_glass_records*' ------------------------------------------------------------------------------

NAN = float("nan")
RAYS = np.zeros((4, 6), dtype=F)
ALIGNED, MISALIGNED_16, MISALIGNED_4 = 0x10000, 0x10008, 0x10002         # (device pointers that are only ever looked at)
_FAKE = C.create_string_buffer(1 << 20)                                   # a handle that is not NULL; no check reads it
FAKE_SCENE = C.addressof(_FAKE)
GOOD = dict(max_bounces=3, chunk_rays=0, min_reflective=1.0, min_transmissive=0.5)
# (the word its message carries, the arguments that fail it), rt_glass.h's checks (2) .. (10)
ORDER = [("params is NULL", dict(params=None)), ("max_bounces", dict(max_bounces=65)), ("chunk_rays", dict(chunk_rays=-1)),
         ("min_reflective", dict(min_reflective=NAN)), ("min_transmissive", dict(min_transmissive=NAN)), ("n < 0", dict(n=-1)),
         ("rows", dict(rows=0)), ("rays pointer", dict(rays=None)), ("out_hits pointer", dict(hits=None)),
         ("too large", dict(n=2 ** 31 - 1, rows=1)), ("d_rays", dict(rays=MISALIGNED_4)), ("d_out_hits", dict(hits=MISALIGNED_16)),
         ("d_out_guide", dict(guide=MISALIGNED_16)), ("d_out_weight", dict(weight=MISALIGNED_4)),
         ("d_out_path", dict(path=MISALIGNED_4))]
HOST_CHECKS = 10


def call(a, device, compact):
    lib = capi.load_library()
    p = capi.RtGlassParams(a["max_bounces"], a["chunk_rays"], a["min_reflective"], a["min_transmissive"])
    args = (a.get("scene", FAKE_SCENE), C.byref(p) if a["params"] else None, a["n"], a["rows"], a["rays"], a["hits"], a["guide"],
            a["weight"], a["path"])
    if compact:
        rc = lib.rt_glass_records_compact_device(*args, None) if device else lib.rt_glass_records_compact(*args)
    else:
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
def test_every_argument_check_gives_rt_glass_records_code_and_message(device):
    last = len(ORDER) if device else HOST_CHECKS
    cases = [dict(bad_from(last, last, device), **bad) for bad in (dict(max_bounces=-1), dict(chunk_rays=-7), dict(rows=-1))]
    for first in range(last):
        cases += [bad_from(first, first + 1, device), bad_from(first, last, device)]       # alone; with every later one
    cases += [dict(bad_from(first, last, device), scene=None) for first in (0, 5, last - 1)]  # (1) the scene comes first
    words = ["max_bounces", "chunk_rays", "rows"] + [w for w, _ in ORDER[:last] for _ in range(2)] + ["scene is NULL"] * 3
    assert len(cases) == len(words)
    for a, word in zip(cases, words):
        old, new = call(a, device, False), call(a, device, True)
        assert new == old and new[0] == capi.RT_ERR_INVALID and word in new[1], (a, old, new)
    assert capi.load_library().rt_get_glass_compact_info(None, C.byref(capi.RtGlassCompactInfo())) == capi.RT_ERR_INVALID
    # n == 0 is RT_OK and launches nothing, whatever the pointers; the ranges' ends are valid up to the device
    nothing = dict(bad_from(last, last, device), n=0, rays=None, hits=None, guide=None, weight=None, path=None)
    assert call(nothing, device, True)[0] == capi.RT_OK
    for ends in (dict(max_bounces=0, min_reflective=-INF, min_transmissive=-INF),
                 dict(max_bounces=64, min_reflective=INF, min_transmissive=INF)):
        assert call(dict(bad_from(last, last, device), n=0, **ends), device, True)[0] == capi.RT_OK


# ---- 5. what was there is what it was -------------------------------------------------------------------------------------------

def test_rt_glass_h_keeps_its_functions_and_the_older_step_kernels_their_instantiations():
    text, names = declared(os.path.join(INCLUDE, "rt_glass.h"))
    assert names == OLD_FUNCTIONS and re.findall(r"#include\s*(\S+)", text) == ['"rt_mirror.h"']
    assert int(re.search(r"#define RT_GLASS_VERSION (\d+)", text).group(1)) == capi.load_library().rt_glass_version() == 1
    assert C.sizeof(capi.RtGlassParams) == 16 and C.sizeof(capi.RtGlassInfo) == 32
    for header in ("rt_glass.h", "rt_mirror_compact.h"):                       # their "Not provided" point here
        assert "rt_glass_compact.h" in open(os.path.join(INCLUDE, header)).read(), header
    kernels = [n for n in exported() if "__device_stub__" not in n]
    assert len([n for n in kernels if "rt_glass_step_kernel" in n]) == 4
    assert len([n for n in kernels if "rt_mirror_step_kernel" in n]) == 8
    assert "hipStreamSynchronize" not in open(os.path.join(CSRC, "rt_glass.hip")).read()


def function_body(text, opening):
    """the text between the braces of the definition that `opening` (a regular expression) begins"""
    start = text.index("{", re.search(opening, text).end())
    depth = 0
    for at in range(start, len(text)):
        depth += {"{": 1, "}": -1}.get(text[at], 0)
        if depth == 0:
            return text[start:at + 1]
    raise AssertionError(opening)


def test_the_unit_shares_the_plumbing_and_one_decision_function_serves_both_kernels():
    unit = open(os.path.join(CSRC, "rt_glass_compact.hip")).read()
    assert '#include "rt_host.h"' in unit and "rt_internal_launch_hits" in unit and "#pragma clang fp contract(off)" in unit
    assert "rt_mirror_check_args" in unit and "RT_INTERNAL_UNIT_GLASS_COMPACT" in unit and "rt_internal_order_stream" in unit
    assert "rt_internal_mirror_compact_scan(" in unit                         # the mirror unit's scan ...
    assert "rt_scan_groups_kernel" not in unit and "rt_scan_total_kernel" not in unit      # ... and no second pair of kernels
    assert "more chains go on than the bounce had" in unit and "hipStreamIsCapturing" in unit
    assert re.search(r"RT_INTERNAL_UNIT_GLASS_COMPACT,\s*RT_INTERNAL_UNITS\s*}", open(os.path.join(CSRC, "rt_internal.h")).read())
    assert re.search(r"^SINGLE_UNITS\s*:=.*\brt_glass_compact\b", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    sources = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))}
    definitions = [f for f, text in sources.items() for _ in re.findall(r"\bRtGlassDecision rt_glass_decide\(", text)]
    assert definitions == ["rt_glass_compact_body.h"]
    body = re.sub(r"/\*.*?\*/", "", sources["rt_glass_compact_body.h"], flags=re.S)
    for kernel in (r"void rt_glass_compact_count_kernel\(", r"void rt_glass_compact_step_kernel\("):
        assert len(re.findall(kernel, body)) == 1
        inside = function_body(body, kernel)
        assert len(re.findall(r"\brt_glass_decide\(", inside)) == 1 and "rt_scan_rank(" in inside, kernel
        assert "rt_glass_child(" not in inside and "sqrtf" not in inside      # no second copy of the refraction beside it
    assert "rt_glass_child(" in function_body(body, r"RtGlassDecision rt_glass_decide\(")
    assert len(re.findall(r"\bbool rt_glass_child\(", "".join(sources.values()))) == 1


# ---- 6. the GPU tests' preconditions, on the reference ------------------------------------------------------------------------

W61, H37 = glass_scenes.SIZES[0]
W96, H80 = glass_scenes.SIZES[1]


def alive_of(path, max_bounces):
    """alive[b] = |{i : (path[i] & 0xff) >= b}| for b = 0 .. max_bounces"""
    k = glass_ref.unpack(np.asarray(path))[0].reshape(-1)
    return [int((k >= b).sum()) for b in range(max_bounces + 1)]


ALIVE = [("glass", W61, H37, 1.0, [2257, 1223, 454, 124, 81, 31, 22, 20, 12]),
         ("glass", W61, H37, 0.5, [2257, 1587, 782, 321, 169, 88, 37, 32, 18]),
         ("glass", W96, H80, 0.5, [7680, 5319, 2632, 1039, 577, 288, 148, 111, 64]),
         ("edges", W61, H37, 0.5, [2257, 1641, 828, 355, 182, 97, 43, 34, 19]),
         ("open", W61, H37, 1.0, [2257, 1178, 332, 67, 0, 0, 0, 0, 0]),
         ("open", W61, H37, 0.5, [2257, 1178, 332, 67, 0, 0, 0, 0, 0])]


@pytest.mark.parametrize("key,W,H,floor,want", ALIVE)
def test_the_live_rays_of_the_reference_per_query(key, W, H, floor, want):
    alive = alive_of(glass_scenes.reference(key, W, H, 8, floor, 0.5)[3], 8)
    assert alive == want
    assert all(a >= b for a, b in zip(alive, alive[1:]))                                   # non-increasing
    assert any(a > 256 for a in alive[1:])                                                 # more than one workgroup, past query 0
    if key == "open":
        assert alive[3] > 0 and alive[4] == 0                                              # empty at query 4: the early end
    elif W == W61:
        assert any(0 < a < 64 for a in alive)                                              # and less than one wavefront
    else:
        assert alive[8] == 64                                                              # (96 x 80: exactly one, at the limit)


def test_the_tiled_batch_has_more_live_entries_than_one_step_of_the_scan_covers():
    """64 tiles of the 96 x 80 frame: the list of query 1 takes more than kScanBlock = 1024 workgroups' counts (csrc/rt_scan.h)"""
    alive = alive_of(glass_scenes.reference("glass", W96, H80, 8, 0.5, 0.5)[3], 8)
    assert 64 * W96 * H80 == 491520 and 64 * alive[1] == 340416 and -(-340416 // 256) > 1024


def candidates_without_a_child(scene, out, look):
    """of a reference with details: the rays that somewhere met a candidate without a child and went on from it as a mirror,
    and the rays whose terminal hit is a candidate at which the chain ended without being cut -- a candidate without a child
    that is no mirror either"""
    hits, d = out[0], out[4]
    tf = glass_ref.transmissive(scene)[0]
    ch, gl = d["chain"], d["glass"]
    candidate = (ch >= 0) & (tf[np.clip(ch, 0, None)] > 0) & (tf[np.clip(ch, 0, None)] >= F(look))
    o = hits["object"]
    at_end = (o >= 0) & (hits["flags"] & 2 == 0) & (tf[np.clip(o, 0, None)] > 0) & (tf[np.clip(o, 0, None)] >= F(look))
    return (candidate & ~gl).any(-1), at_end & ~d["cut"]


def test_the_batches_hold_the_rays_on_which_count_and_step_must_agree_about_the_child():
    """"edges" under the pixel rays: candidates without a child -- the bubble's rim, which is a full mirror there -- go on as
    mirrors.  No pixel ray of "edges" ENDS on such a candidate (every sphere that lacks a child somewhere is a mirror there), so
    the other kind is held where the GPU tests take it from: the handmade batch on "edges" at a floor of 1.0 -- starts inside the
    glass sphere (t < 0, rf 0.7) -- and the glass room's pixel rays, whose bubble is no mirror."""
    scene = glass_scenes.ref_scene("edges")
    for floor in (1.0, 0.5):
        out = glass_scenes.reference("edges", W61, H37, 8, floor, 0.2)
        fell, ended = candidates_without_a_child(scene, out, 0.2)
        assert fell.sum() >= 20 and (out[4]["childless"][fell] >= 1).all() and ended.sum() == 0, (floor, fell.sum(), ended.sum())
    import glass_compact_batches
    rays = glass_compact_batches.handmade_rays()
    out = glass_ref.records(scene, rays, 3, 1.0, 0.2, details=True)
    fell, ended = candidates_without_a_child(scene, out, 0.2)
    assert fell.sum() >= 20 and ended.sum() >= 8, (fell.sum(), ended.sum())
    assert (out[0]["object"][ended] == glass_scenes.GLASS_SPHERE).all() and (out[0]["distance"][ended] < 0).all()
    room = glass_scenes.ref_scene("glass")
    fell, ended = candidates_without_a_child(room, glass_scenes.reference("glass", W61, H37, 8, 1.0, 0.5), 0.5)
    assert ended.sum() >= 5 and fell.sum() == 0


def test_the_list_size_batches_are_cut_as_the_gpu_test_needs_them():
    import glass_compact_batches as B
    ch = B.chains()
    k, glass = ch["k"], ch["glass"]
    assert B.LIST_SIZES == (0, 1, 63, 64, 65, 255, 256, 257) and B.ENDING == 300
    for bounce in (1, 2):
        for kind in B.KINDS:
            for c in B.LIST_SIZES:
                pick = B.list_size_batch(bounce, c, kind)
                alive = [int((k[pick] >= b).sum()) for b in range(bounce + 1)]
                assert alive[bounce] == c and alive[bounce - 1] == 300 + c, (bounce, kind, c, alive)
                going = pick[k[pick] >= bounce]
                assert (glass[going, bounce - 1] == (kind == "glass")).all()              # the survivors: all glass, or all mirror
                if c > 1:
                    at = np.flatnonzero(k[pick] >= bounce)
                    assert (np.diff(at) > 1).all()                                        # each among chains that end
    pick = B.all_alive_batch()
    assert len(pick) == 5319 and (k[pick] >= 1).all() and len(pick) % 256 != 0 and (np.diff(pick) > 0).all()
    steps = glass[pick, 0]
    assert steps.sum() >= 1000 and (~steps).sum() >= 1000                                 # both kinds of step in one list


def test_the_all_alive_tile_is_what_the_large_run_d_relies_on():
    """test_glass_compact_large_gpu.py's tile of run (d), which it asserts again before its first launch: the format is
    mirror_large.room_tile's, the figures are pinned, no word is the sentinel and no float field holds a NaN
    (mirror_large.tile_preconditions, inside all_alive_tile_figures)"""
    import glass_compact_batches as B
    import large_extents
    import mirror_large
    rays, words, details = B.all_alive_tile()
    M = 5319
    assert rays.shape == (M, 6) and rays.dtype == F and rays.flags["C_CONTIGUOUS"] and M % 2 == 1
    assert [(name, w.shape, w.dtype) for name, w in words.items()] == [(name, (M, n), np.int32) for name, n in mirror_large.WORDS.items()]
    ch, pick = B.chains(), B.all_alive_batch()
    assert (rays == ch["rays"][pick]).all()
    for w, a in zip(words.values(), ch["want"]):                             # the frame's reference at the batch's indices
        assert (w.reshape(-1) == np.ascontiguousarray(a[pick]).view(np.int32).reshape(-1)).all()
    for w in words.values():
        assert not (w.view(np.uint32) == np.uint32(large_extents.SENTINEL)).any()
    figures = B.all_alive_tile_figures(words, details)
    assert figures == B.ALL_ALIVE_FIGURES
    assert figures == dict(alive=[5319, 5319, 2632, 1039, 577, 288, 148, 111, 64], cut=47, g=3495,
                           glass_steps=[3007, 288, 367, 177, 76, 55, 24, 23], mirror_steps=[2312, 2344, 672, 400, 212, 93, 87, 41],
                           ended=[0, 2687, 1593, 462, 289, 140, 37, 47, 64], childless=15, ended_childless=15)
    # every step is one or the other, and what does not go on ended: the three rows account for the tile
    for b in range(8):
        assert figures["glass_steps"][b] + figures["mirror_steps"][b] == figures["alive"][b + 1]
        assert figures["alive"][b] - figures["alive"][b + 1] == figures["ended"][b]
    # the standard tile's rows past query 0 are this tile's: it is that tile without the 2360 chains that end at once (and with
    # ray 7679, which ends at once too)
    assert figures["alive"][1:] == glass_scenes.LARGE_FIGURES["alive"][1:] and figures["glass_steps"] == glass_scenes.LARGE_FIGURES["glass_steps"]
    assert glass_scenes.LARGE_FIGURES["childless"] - figures["childless"] == 70


def test_the_large_runs_list_sizes_from_the_tiles():
    """what test_glass_compact_large_gpu.py's runs (b) and (d) assert of their lists, from the closed form over the tile's path
    words (mirror_large.tiled_expected_info, which test_mirror_compact_cpu.py proves equal to the count over tiled words)"""
    import glass_compact_batches as B
    import mirror_large
    n, chunk, B31, B32 = 100000007, 90000001, 1 << 31, 1 << 32
    path = B.all_alive_tile()[1]["path"].view(np.uint32).reshape(-1)
    rays_, queried, chunks, queries, syncs, alive = mirror_large.tiled_expected_info(path, n, 8, chunk)
    assert alive[0] == alive[1] == n and (rays_, chunks, queries, syncs) == (n, 2, 18, 16) and min(alive[:9]) > 0 and alive[9:] == [0] * 56
    first = mirror_large.tiled_expected_info(path, chunk, 8)[5]
    assert first[:3] == [chunk, chunk, 44534472] and 48 * first[1] > B32 and 24 * first[1] > B31 and min(first[:9]) > 0
    assert first[1] > 89478485 == B32 // 48                                   # the fewest entries whose records pass 2^32 bytes
    path = glass_scenes.large_tile()[1]["path"].view(np.uint32).reshape(-1)
    first = mirror_large.tiled_expected_info(path, chunk, 8)[5]
    assert first[0] == chunk and first[1] == 62340474 and 62.3e6 < first[1] < 62.4e6
    assert 48 * first[1] < B32                                                # (why run (d) has a tile of its own)
    assert 237 * 1024 < -(-first[1] // 256) <= 238 * 1024                     # 238 groups of the scan's first level
    assert mirror_large.tiled_expected_info(path, n, 8, 0)[2] == 1 and mirror_large.tiled_expected_info(path, n, 8, 1237029)[2] == 81


@pytest.mark.parametrize("floor", [1.0, 0.5])
@pytest.mark.parametrize("bounces", [8, 3])
def test_in_open_chunks_end_at_different_bounces_and_a_later_chunk_goes_further(bounces, floor):
    """test_glass_compact_gpu.py's chunk test on "open": under each of its chunk sizes some chunk ends early and -- except in
    chunks of 1000, which run 4, 4 and 3 queries -- a later chunk runs more queries than it"""
    import glass_compact_batches as B
    assert B.OPEN_CHUNKS == (7, 64, 300, 600, 1000) and B.OPEN_CHUNKS_NO_LATER_CHUNK_GOES_FURTHER == (1000,)
    path = np.asarray(glass_scenes.reference("open", W61, H37, bounces, floor, 0.5)[3]).reshape(-1)
    for chunk in B.OPEN_CHUNKS:
        q = B.assert_chunks_end_at_different_bounces(path, bounces, chunk)
        assert len(q) == -(-len(path) // chunk) and max(q) == 4 and sum(q) == mirror_large_info(path, bounces, chunk)[3]
        assert (max(q) == bounces + 1) == (bounces == 3)                      # at 8 no chunk runs every query, at 3 some do
    assert B.queries_per_chunk(path, bounces, 300) == [2, 3, 4, 4, 3, 3, 4, 1]
    assert B.queries_per_chunk(path, bounces, 600) == [3, 4, 3, 4]


def mirror_large_info(path, bounces, chunk):
    import mirror_large
    return mirror_large.expected_info(path, bounces, chunk)


def test_the_default_chunk_is_the_mirror_compact_calls():
    unit = open(os.path.join(CSRC, "rt_glass_compact.hip")).read()
    assert "static_assert(kRayBytes == 217" in unit and "== 1237029" in unit and (256 << 20) // 217 == 1237029
