"""rt_indirect_paths over the live paths alone (include/rt_paths_compact.h) without a GPU: the header, the exported symbols, the
info's layout, the argument checks (rt_paths.h's, one copy), and -- on the reference alone, paths_ref over the CPU oracle -- the
conditions the comparisons of tests/test_paths_compact_gpu.py rest on: every frame's alive counts fall strictly and stay above
zero, so that a wrong list shows; the list-size construction yields the sizes it names; the two-chunk batch has a chunk that ends
at once and one that does not; and paths_compact_expect, the one helper the expected traces, queries and syncs come from, is the
header's rule."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ao_ref
import indirect_ref
import paths_compact_ref as ref
import paths_ref
import query_ref
from tilecoderaytracer_amd import capi
from tilecoderaytracer_amd.capi import RtPathsCompactInfo          # (a library without the unit has no such struct)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_paths_compact.h")
CSRC = os.path.join(ROOT, "tilecoderaytracer_amd", "csrc")
EXE = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
FUNCTIONS = ["rt_get_paths_compact_info", "rt_indirect_paths_compact", "rt_indirect_paths_compact_device", "rt_paths_compact_version"]
FRAME = {f[0]: f for f in indirect_ref.FRAMES}
# every (frame, B) tests/test_paths_compact_gpu.py compares with the oracle
USED = ([(f, B) for f in indirect_ref.FRAMES for B in (2, 3)] + [(FRAME[k], B) for k in ("builtin", "random3") for B in (4, 8)] +
        [(indirect_ref.EMITTER_FRAME, 3)])


def header_prose():
    """the header's comment as running text: the line breaks and the comment's leading stars taken out"""
    return " ".join(re.sub(r"\n \*", " ", open(HEADER).read()).split())


# ---- 1. the header, the symbols, the layout ------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t|const char \*)\s*(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    assert re.findall(r"#include\s*(\S+)", text) == ['"rt_paths.h"']
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    assert int(re.search(r"#define RT_PATHS_COMPACT_VERSION (\d+)", text).group(1)) == lib.rt_paths_compact_version() == 1
    assert lib.rt_paths_version() == 1                                  # the header it builds on is the one it was


def test_the_header_states_its_contract():
    said = header_prose()
    for words in ("THE DEFINITION: this header adds none", "bit for bit", "rt_paths.h's (1) .. (12)", "WAITS FOR ITS STREAM",
                  "capturing", "rt_indirect_paths_device can", "With bounces == 1 there is no count, no list and no wait",
                  "minus 1 if the chunk ran all B bounces", "never records * S * B", "141 bytes a path", "256 MiB",
                  "rt_get_paths_info is not touched", "in no stage", "Not provided", "Russian roulette", "2^32"):
        assert words in said, words
    for forked in ("0x7feb352d", "0x846ca68b"):                        # no arithmetic is repeated here
        assert forked not in said, forked


def test_the_info_is_136_bytes_laid_out_as_the_header_says(tmp_path):
    I = RtPathsCompactInfo
    assert C.sizeof(I) == 136
    assert [(n, getattr(I, n).offset) for n, _ in I._fields_] == [
        ("records", 0), ("rays", 8), ("chunks", 16), ("traces", 20), ("queries", 24), ("syncs", 28), ("raygen_ms", 32),
        ("trace_ms", 40), ("query_ms", 48), ("step_ms", 56), ("resolve_ms", 64), ("alive", 72)]
    said = header_prose()
    for words in ("rt_paths_compact_info is 136 bytes", "traces at 20", "syncs at 28", "raygen_ms at 32", "alive at 72"):
        assert words in said, words
    assert "sizeof(rt_paths_compact_info) == 136" in open(os.path.join(CSRC, "rt_paths_compact.hip")).read()
    if not shutil.which("gcc"):
        return
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_paths_compact.h"\n'
                   'int main(void) { printf("%d %d %d %d %d\\n", (int)sizeof(rt_paths_compact_info),\n'
                   "  (int)offsetof(rt_paths_compact_info, traces), (int)offsetof(rt_paths_compact_info, syncs),\n"
                   "  (int)offsetof(rt_paths_compact_info, raygen_ms), (int)offsetof(rt_paths_compact_info, alive)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [136, 20, 28, 32, 72]


def test_the_library_gained_the_count_step_and_resolve_kernels_and_no_third_scan():
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    names = [line.split()[-1] for line in r.stdout.splitlines() if line.split()]
    kernels = [n for n in names if "_kernel" in n and "__device_stub__" not in n]
    assert len([n for n in kernels if "rt_paths_compact_count_kernel" in n]) == 2      # first or not
    assert len([n for n in kernels if "rt_paths_compact_step_kernel" in n]) == 4       # first / last
    assert len([n for n in kernels if "rt_paths_compact_resolve_kernel" in n]) == 1
    assert len([n for n in kernels if "rt_scan_groups_kernel" in n]) == 1              # rt_mirror_compact.hip's, shared
    assert len([n for n in kernels if "rt_scan_total_kernel" in n]) == 1


def test_the_two_units_share_one_body_and_one_check():
    body = open(os.path.join(CSRC, "rt_paths_body.h")).read()
    for name in ("rt_paths_decide", "rt_paths_accumulate", "rt_paths_next_ray", "rt_paths_resolve", "rt_paths_check_args"):
        assert re.search(r"\b%s\(" % name, body), name
    units = [open(os.path.join(CSRC, f)).read() for f in ("rt_paths.hip", "rt_paths_compact.hip")]
    for text in units:
        assert '#include "rt_paths_body.h"' in text and "rt_paths_check_args(" in text
        assert "rt_paths_resolve(lds" in text and "must be 1.." not in text          # (the messages are the body's alone)
    compact = units[1]
    assert compact.count("rt_paths_decide(") == 2                                     # the count pass and the step
    assert "0x7feb352d" not in compact                                                # the hash is the body's
    # a slot of its own before RT_INTERNAL_UNITS (the glass unit's slot stays the last: tests/test_glass_compact_cpu.py)
    assert re.search(r"RT_INTERNAL_UNIT_PATHS_COMPACT,\s*RT_INTERNAL_UNIT_GLASS_COMPACT,\s*RT_INTERNAL_UNITS",
                     open(os.path.join(CSRC, "rt_internal.h")).read())


# ---- 2. the argument checks: rt_paths.h's, in its order, with its messages, without a device -----------------------------------------

NAN = float("nan")
GOOD = dict(samples=2, gather_depth=1, chunk_records=0, emitters=0, seed=0, key0=0, gain=1.0, bounces=2)
HITS = np.zeros(4, dtype=query_ref.HIT_DTYPE)
ALIGNED, MISALIGNED_16, MISALIGNED_4 = 0x10000, 0x10008, 0x10002         # (device pointers that are only ever looked at)
ORDER = [("params is NULL", dict(params=None)), ("samples", dict(samples=9)), ("bounces", dict(bounces=9)),
         ("gather_depth", dict(gather_depth=-2)), ("chunk_records", dict(chunk_records=-2)), ("emitters", dict(emitters=3)),
         ("gain", dict(gain=NAN)), ("n < 0", dict(n=-1)), ("hits pointer", dict(hits=None)), ("output pointer", dict(out=None)),
         ("533333333 records", dict(n=533333334)), ("16-byte", dict(hits=MISALIGNED_16)), ("d_out", dict(out=MISALIGNED_4)),
         ("d_base_rgb", dict(base=MISALIGNED_4))]
# a handle that is not NULL for the checks that come before the handle is read: zeroed memory, never dereferenced by them
_FAKE = C.create_string_buffer(1 << 20)
FAKE_SCENE = C.addressof(_FAKE)


def bad_from(first, last, device):
    a = dict(GOOD, params=True, n=4, hits=ALIGNED if device else HITS.ctypes.data, out=ALIGNED if device else 0x20000, base=None,
             scene=FAKE_SCENE)
    for _, bad in reversed(ORDER[first:last]):
        a.update(bad)
    return a


def call(a, device, compact=True):
    lib = capi.load_library()
    p = capi.RtPathsParams(*(a[k] for k in ("samples", "gather_depth", "chunk_records", "emitters", "seed", "key0", "gain", "bounces")))
    p = C.byref(p) if a["params"] else None
    dev, host = ((lib.rt_indirect_paths_compact_device, lib.rt_indirect_paths_compact) if compact else
                 (lib.rt_indirect_paths_device, lib.rt_indirect_paths))
    rc = dev(a["scene"], p, a["n"], a["hits"], a["base"], a["out"], None) if device else host(a["scene"], p, a["n"], a["hits"],
                                                                                               a["base"], a["out"])
    return rc, lib.rt_last_error().decode()


@pytest.mark.parametrize("device", [False, True])
def test_every_argument_check_is_rt_indirect_paths_own_in_its_order_with_its_message(device):
    last = len(ORDER) if device else 11
    for first in range(last):
        word = ORDER[first][0]
        for upto in (first + 1, last):                                              # alone; with every later one
            rc, msg = call(bad_from(first, upto, device), device)
            assert rc == capi.RT_ERR_INVALID and word in msg, (first, word, msg)
            assert (rc, msg) == call(bad_from(first, upto, device), device, compact=False), (first, word)
    for first in (0, 6, last - 1):                                                  # (1) the scene comes first
        rc, msg = call(dict(bad_from(first, last, device), scene=None), device)
        assert rc == capi.RT_ERR_INVALID and msg == "scene is NULL", (first, msg)
    assert capi.load_library().rt_get_paths_compact_info(None, C.byref(RtPathsCompactInfo())) == capi.RT_ERR_INVALID


# ---- 3. the conditions the GPU comparisons rest on, on the reference alone -----------------------------------------------------------

@pytest.mark.parametrize("frame,B", USED, ids=[f"{f[0]}{f[1]}x{f[2]}-B{B}" for f, B in USED])
def test_every_frames_alive_counts_fall_strictly_and_stay_above_zero(frame, B):
    """so a list that kept a dead path, lost a live one or came out empty shows in alive[] and in the words"""
    counts = paths_ref.oracle_walk(frame).counts(B)
    assert len(counts) == B and all(counts[b] > counts[b + 1] for b in range(B - 1)) and counts[B - 1] > 0, counts
    if frame in indirect_ref.FRAMES and frame[0] in paths_ref.ALIVE:
        k = min(B, 4)
        assert counts[:k] == paths_ref.ALIVE[frame[0]][:k]


def oracle_list_walk(hits):
    return ref.oracle_walk_of(hits, **ref.LIST_KW)


@pytest.fixture(scope="module")
def on():
    return ref.going_on(oracle_list_walk)


@pytest.mark.parametrize("c", ref.LIST_SIZES)
def test_the_list_size_construction_yields_exactly_c_live_paths_at_bounce_one(c, on):
    hits, base = ref.list_of_size(c, on), ref.builtin_records()
    went_on = np.zeros(len(base), dtype=bool)
    went_on[on] = True
    assert (hits["object"] < 0).sum() == (base["object"] < 0).sum() + len(on) - c           # the others, and only they, died
    assert np.array_equal(hits[~went_on], base[~went_on])                                   # the paths that end at once: left
    walk = oracle_list_walk(hits)
    counts = walk.counts(3)
    assert counts[1] == c and counts[0] == int(ao_ref.live_records(hits).sum())
    assert np.array_equal(np.flatnonzero(walk.alive[1]), on[:c])                            # no other path's key changed
    assert counts[0] - c > 100                                                               # paths that end at bounce 0 remain


def test_the_two_chunk_batch_has_a_chunk_that_ends_at_once_and_one_that_runs_every_bounce():
    hits = ref.two_chunk_batch()
    assert hits.shape == (600,)
    walk = ref.oracle_walk_of(hits, **ref.SKY_KW)
    want = ref.paths_compact_expect(walk, 300, 4, False)
    assert want["runs"] == [1, 4] and want["chunks"] == 2
    assert int(walk.alive[1][:2700].sum()) == 0 and int(walk.alive[0][:2700].sum()) == 2700
    assert (want["traces"], want["queries"], want["syncs"]) == (5, 5, 1 + 3)
    assert want["rays"] == 5400 + sum(want["alive"][1:]) and want["alive"][3] > 0
    assert ref.paths_compact_expect(walk, 300, 4, True)["queries"] == 4                    # the last bounce of the chunk that ran it


# ---- 4. the helper is the header's rule ------------------------------------------------------------------------------------------------

class FakeWalk:
    """a Walk's alive masks, hand-made: 4 records of S = 2 paths, bounce by bounce"""
    S = 2
    hits = np.zeros(4, dtype=query_ref.HIT_DTYPE)
    alive = [np.array(m, dtype=bool) for m in ([1, 1, 1, 1, 0, 0, 1, 1], [1, 0, 0, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, 0, 1],
                                               [0, 0, 0, 0, 0, 0, 0, 1])]

    def extend(self, B):
        assert B <= len(self.alive)
        return self


@pytest.mark.parametrize("chunk,B,emitters,want", [
    # one chunk: every bounce runs
    (4, 4, False, dict(chunks=1, runs=[4], traces=4, queries=4, syncs=3, rays=8 + 3 + 1 + 1)),
    (4, 4, True, dict(chunks=1, runs=[4], traces=4, queries=3, syncs=3, rays=8 + 3 + 1 + 1)),
    (0, 3, True, dict(chunks=1, runs=[3], traces=3, queries=2, syncs=2, rays=8 + 3 + 1)),
    # a record a chunk: bounces run 2, 1, 1, 4 -- a chunk that stops early waits once more than it traces again
    (1, 4, False, dict(chunks=4, runs=[2, 1, 1, 4], traces=8, queries=8, syncs=2 + 1 + 1 + 3, rays=8 + 3 + 1 + 1)),
    (1, 4, True, dict(chunks=4, runs=[2, 1, 1, 4], traces=8, queries=7, syncs=7, rays=13)),
    (3, 2, True, dict(chunks=2, runs=[2, 2], traces=4, queries=2, syncs=2, rays=8 + 3)),
    # one bounce: no count, no list, no wait
    (2, 1, False, dict(chunks=2, runs=[1, 1], traces=2, queries=2, syncs=0, rays=8)),
    (2, 1, True, dict(chunks=2, runs=[1, 1], traces=2, queries=0, syncs=0, rays=8)),
])
def test_the_expected_counts_are_the_headers_rule(chunk, B, emitters, want):
    got = ref.paths_compact_expect(FakeWalk(), chunk, B, emitters)
    assert {k: got[k] for k in want} == want
    assert got["records"] == 4 and got["alive"] == [6, 3, 1, 1][:B]


def test_the_default_chunk_is_the_most_records_within_256_mib():
    assert ref.chunk_of(0, 10 ** 9, 4) == (256 << 20) // (141 * 4)
    assert ref.chunk_of(0, 10 ** 9, 64) == 29746 and ref.chunk_of(0, 1000, 4) == 1000 and ref.chunk_of(7, 1000, 4) == 7
    text = open(os.path.join(CSRC, "rt_paths_compact.hip")).read()
    assert "kPathBytes == 141" in text and "(size_t)256 << 20" in text


# ---- 5. the executable --------------------------------------------------------------------------------------------------------------

def test_the_usage_text_names_the_flag_and_the_flag_needs_indirect(tmp_path):
    r = subprocess.run([EXE, "--no-such-option"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage:" in r.stderr and "[--indirect-compact]" in r.stderr
    r = subprocess.run([EXE, "--width", "8", "--height", "8", "--no-txt", "--indirect-compact"], capture_output=True, text=True,
                       cwd=tmp_path)
    assert r.returncode == 1 and "usage:" in r.stderr and "Start Ray Tracing" not in r.stdout and not os.listdir(tmp_path)
