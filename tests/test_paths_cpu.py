"""Diffuse light paths of more than one bounce (include/rt_paths.h) without a GPU: the header, the exported symbols, the struct
layouts, every argument check in the header's order (none touches a device or the handle), and paths_ref -- the tests'
restatement of the definition -- on the CPU oracle: the conditions the GPU tests rest on, with the figures the definition was
prototyped with, and a mutation study: every wrong rule of paths_ref.RULES changes an output word or an alive count on a
named input."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_frames
import ao_ref
import indirect_ref
import paths_ref
import query_ref
from tilecoderaytracer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "rt_paths.h")
EXE = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
FUNCTIONS = ["rt_get_paths_info", "rt_indirect_paths", "rt_indirect_paths_device", "rt_paths_version"]
F = np.float32
FRAME = {f[0]: f for f in indirect_ref.FRAMES}
FRAME_IDS = [f[0] for f in indirect_ref.FRAMES]


# ---- 1. the header ----------------------------------------------------------------------------------------------------------

def test_header_declares_exactly_its_functions_and_the_library_exports_them():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(set(re.findall(r"^\s*(?:int|uint64_t|const char \*)\s*(rt_\w+)\s*\(", text, flags=re.M))) == FUNCTIONS
    assert '#include "rt_capi_indirect.h"' in text and len(re.findall(r"#include", text)) == 1
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert getattr(lib, name) is not None, name
    assert int(re.search(r"#define RT_PATHS_VERSION (\d+)", text).group(1)) == lib.rt_paths_version() == 1
    assert int(re.search(r"#define RT_PATHS_MAX_BOUNCES (\d+)", text).group(1)) == capi.RT_PATHS_MAX_BOUNCES == 8
    assert lib.rt_capi_indirect_version() == 1                         # the header it builds on is the one it was


def test_the_header_says_what_follows_from_the_definition():
    text = " ".join(open(HEADER).read().split())
    for said in ("With bounces == 1 every word is rt_indirect_diffuse's", "chunk_records never change a bit",
                 "never falls as B grows", "zero-throughput stop changes no output word", "rt_capi_ao.h"):
        assert said in text, said
    for forked in ("0x7feb352d", "0x846ca68b"):                        # the hash is rt_capi_ao.h's, not repeated
        assert forked not in text, forked


def test_struct_layouts_match_the_header(tmp_path):
    P, I, Q = capi.RtPathsParams, capi.RtPathsInfo, capi.RtIndirectParams
    assert C.sizeof(P) == 32 and P.bounces.offset == 28
    assert [(n, getattr(P, n).offset) for n, _ in Q._fields_] == [(n, getattr(Q, n).offset) for n, _ in Q._fields_]
    assert C.sizeof(I) == 128
    assert [getattr(I, n).offset for n, _ in I._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64]
    text = open(HEADER).read()
    for said in ("rt_paths_params is 32 bytes", "bounces at 28", "rt_paths_info is 128 bytes", "step_ms at 48", "alive at 64"):
        assert said in " ".join(text.split()), said
    if not shutil.which("gcc"):
        return
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rt_paths.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d %d\\n", (int)sizeof(rt_paths_params), (int)sizeof(rt_paths_info),\n'
                   "  (int)offsetof(rt_paths_params, bounces), (int)offsetof(rt_paths_info, chunks),\n"
                   "  (int)offsetof(rt_paths_info, step_ms), (int)offsetof(rt_paths_info, resolve_ms),\n"
                   "  (int)offsetof(rt_paths_info, alive)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [32, 128, 28, I.chunks.offset, I.step_ms.offset, I.resolve_ms.offset, I.alive.offset]


def test_header_is_plain_c99_with_every_other_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    headers = sorted(h for h in os.listdir(INCLUDE) if h.endswith(".h"))
    assert "rt_paths.h" in headers
    src = tmp_path / "paths.c"
    src.write_text('#include "rt_paths.h"\n' + "".join(f'#include "{h}"\n' for h in headers) +
                   "int main(void) { rt_paths_params p = {4, 1, 0, 0, 7u, 0u, 1.0f, 3}; rt_paths_info i; (void)i;\n"
                   "  return (RT_PATHS_VERSION == 1 && sizeof p == 32 && p.bounces == 3) ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-fsyntax-only", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_gained_the_step_and_resolve_kernels_and_no_render_kernel():
    r = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True)
    names = [line.split()[-1] for line in r.stdout.splitlines() if line.split()]
    kernels = [n for n in names if "rt_paths_" in n and "_kernel" in n and "__device_stub__" not in n]
    assert len([n for n in kernels if "rt_paths_step_kernel" in n]) == 4           # first / last: four instances
    assert len([n for n in kernels if "rt_paths_resolve_kernel" in n]) == 1
    render = [n for n in names if "rt_render_kernel" in n and "__device_stub__" not in n]
    assert len(render) == 117 and not [n for n in render if "paths" in n]
    assert "paths" not in open(os.path.join(ROOT, "tilecoderaytracer_amd", "csrc", "rt_tables.h")).read()


# ---- 2. the argument checks, in the header's order, without a device ---------------------------------------------------------

NAN, INF = float("nan"), float("inf")
GOOD = dict(samples=2, gather_depth=1, chunk_records=0, emitters=0, seed=0, key0=0, gain=1.0, bounces=2)
HITS = np.zeros(4, dtype=query_ref.HIT_DTYPE)
ALIGNED, MISALIGNED_16, MISALIGNED_4 = 0x10000, 0x10008, 0x10002         # (device pointers that are only ever looked at)
# the checks after (1) in the header's order: (the word its message carries, the arguments that fail it)
ORDER = [("params is NULL", dict(params=None)), ("samples", dict(samples=9)), ("bounces", dict(bounces=9)),
         ("gather_depth", dict(gather_depth=-2)), ("chunk_records", dict(chunk_records=-2)), ("emitters", dict(emitters=3)),
         ("gain", dict(gain=NAN)), ("n < 0", dict(n=-1)), ("hits pointer", dict(hits=None)), ("output pointer", dict(out=None)),
         ("533333333 records", dict(n=533333334)), ("16-byte", dict(hits=MISALIGNED_16)), ("d_out", dict(out=MISALIGNED_4)),
         ("d_base_rgb", dict(base=MISALIGNED_4))]
# A handle that is not NULL for the checks that come before the handle is read: all of them but the last (the scene has area
# lights).  Zeroed memory, so that a check that did read it would find nothing rather than fault.
_FAKE = C.create_string_buffer(1 << 20)
FAKE_SCENE = C.addressof(_FAKE)


def bad_from(first, last, device):
    a = dict(GOOD, params=True, n=4, hits=ALIGNED if device else HITS.ctypes.data, out=ALIGNED if device else 0x20000, base=None,
             scene=FAKE_SCENE)
    for _, bad in reversed(ORDER[first:last]):
        a.update(bad)
    return a


def call(a, device):
    lib = capi.load_library()
    p = capi.RtPathsParams(*(a[k] for k in ("samples", "gather_depth", "chunk_records", "emitters", "seed", "key0", "gain", "bounces")))
    p = C.byref(p) if a["params"] else None
    rc = (lib.rt_indirect_paths_device(a["scene"], p, a["n"], a["hits"], a["base"], a["out"], None) if device else
          lib.rt_indirect_paths(a["scene"], p, a["n"], a["hits"], a["base"], a["out"]))
    return rc, lib.rt_last_error().decode()


@pytest.mark.parametrize("device", [False, True])
def test_every_argument_check_comes_before_the_device_in_the_headers_order(device):
    """each bad argument alone is RT_ERR_INVALID with its message; a bad argument together with every later one is still
    reported as the earlier one.  (A call that passes every one of these reads the handle, and is made on the GPU only.)"""
    last = len(ORDER) if device else 11
    for first in range(last):
        word = ORDER[first][0]
        rc, msg = call(bad_from(first, first + 1, device), device)                 # alone
        assert rc == capi.RT_ERR_INVALID and word in msg, (first, word, msg)
        rc, msg = call(bad_from(first, last, device), device)                      # with every later one
        assert rc == capi.RT_ERR_INVALID and word in msg, (first, word, msg)
    for first in (0, 6, last - 1):                                                  # (1) the scene comes first
        rc, msg = call(dict(bad_from(first, last, device), scene=None), device)
        assert rc == capi.RT_ERR_INVALID and msg == "scene is NULL", (first, msg)
    assert capi.load_library().rt_get_paths_info(None, C.byref(capi.RtPathsInfo())) == capi.RT_ERR_INVALID


@pytest.mark.parametrize("device", [False, True])
def test_bounces_at_the_last_admitted_and_the_first_refused_value(device):
    """0 and 9 are refused as `bounces`, right after `samples` and before gather_depth; 1 and 8 pass on to the next check"""
    later = dict(gather_depth=-1)
    for bounces in (0, 9, -1, 2 ** 31 - 1):
        rc, msg = call(dict(bad_from(0, 0, device), bounces=bounces, **later), device)
        assert rc == capi.RT_ERR_INVALID and "bounces must be 1..8" in msg and f"got {bounces}" in msg, (bounces, msg)
        rc, msg = call(dict(bad_from(0, 0, device), bounces=bounces, samples=0), device)
        assert rc == capi.RT_ERR_INVALID and "samples" in msg, (bounces, msg)
    for bounces in (1, 8):
        rc, msg = call(dict(bad_from(0, 0, device), bounces=bounces, **later), device)
        assert rc == capi.RT_ERR_INVALID and "gather_depth" in msg, (bounces, msg)


# ---- 3. the reference on the oracle's frames: the conditions the GPU tests rest on ------------------------------------------------

def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("key", FRAME_IDS)
def test_one_bounce_is_the_indirect_term_bit_for_bit(key):
    frame = FRAME[key]
    for emitters in (False, True):
        for with_base in (False, True):
            assert indirect_ref.same_bits(paths_ref.oracle_term(frame, 1, emitters, with_base),
                                          indirect_ref.oracle_term(frame, emitters, with_base)), (key, emitters, with_base)


@pytest.mark.parametrize("key", FRAME_IDS)
def test_the_alive_counts_are_the_measured_ones(key):
    w = paths_ref.oracle_walk(FRAME[key])
    counts = w.counts(4)
    assert counts == paths_ref.ALIVE[key]
    hits = indirect_ref.oracle_gather(*FRAME[key])[1]
    assert counts[0] == w.S * int(ao_ref.live_records(hits).sum())


def fresh_walk(frame, rule=None, key0=0, hits=None, gain=1.0):
    key, W, H, depth, n, seed, gather_depth = frame
    orc = adaptive_frames.oracle_scene(key)
    hits = indirect_ref.oracle_gather(*frame)[1] if hits is None else hits
    w = paths_ref.Walk(paths_ref.oracle_tracer(orc, gather_depth), hits, n, indirect_ref.object_diffuse(orc), gain, seed, key0, rule)
    w.orc = orc
    return w


@pytest.mark.parametrize("key,without", [("twomirrors", [4388, 1703, 385, 162]), ("builtin", [20286, 20248, 20233, 20227])])
def test_the_zero_throughput_stop_shows_in_the_counts_and_in_no_output_word(key, without):
    """the header says so: the counts tell the rule apart, the output does not -- with gain -0.75 as well"""
    assert fresh_walk(FRAME[key], "dead_only").counts(4) == without != paths_ref.ALIVE[key]
    for gain in (1.0, -0.75):
        a, b = fresh_walk(FRAME[key], "dead_only", gain=gain), fresh_walk(FRAME[key], gain=gain)
        for B in (2, 3, 4):
            assert indirect_ref.same_bits(a.term(B), b.term(B)), (key, gain, B)


@pytest.mark.parametrize("key", sorted(paths_ref.CONDITIONS))
def test_every_compared_bounce_adds_something_to_half_of_the_live_records(key):
    """measured: builtin 0.834 0.834 0.832, random3 0.891 0.890 0.890, grid16 0.681 0.561 (0.453 at 3 -> 4: not held)"""
    paths_ref.check_conditions(FRAME[key])


def test_the_emitters_flag_is_exercised_at_later_bounces():
    """EMITTER_FRAME at B = 3: the two settings differ on at least 150 records (measured 185, against 115 at B = 1), at least 50
    of which are equal at B = 1 (measured 70)"""
    w = paths_ref.oracle_walk(indirect_ref.EMITTER_FRAME)
    d3 = (bits(w.term(3, False)) != bits(w.term(3, True))).any(axis=-1)
    d1 = (bits(w.term(1, False)) != bits(w.term(1, True))).any(axis=-1)
    assert d3.sum() >= 150 and (d3 & ~d1).sum() >= 50, (int(d3.sum()), int(d1.sum()), int((d3 & ~d1).sum()))


@pytest.mark.parametrize("key", FRAME_IDS)
def test_with_a_gain_that_is_not_negative_the_term_never_falls_as_bounces_grow(key):
    terms = [paths_ref.oracle_term(FRAME[key], B, False, False) for B in (1, 2, 3, 4)]
    for B in (1, 2, 3):
        assert np.isfinite(terms[B]).all() and (terms[B] >= terms[B - 1]).all(), (key, B)


def test_strips_and_two_uneven_chunks_of_the_reference_equal_the_whole():
    frame = FRAME["builtin"]
    hits = indirect_ref.oracle_gather(*frame)[1]
    W, H = hits.shape
    whole_w = paths_ref.oracle_walk(frame)
    whole, counts = whole_w.term(3), whole_w.counts(3)
    parts = [fresh_walk(frame, key0=x0 * H, hits=np.ascontiguousarray(hits[x0:x1])) for x0, x1 in ((0, 20), (20, 21), (21, 61))]
    assert indirect_ref.same_bits(np.concatenate([p.term(3) for p in parts]), whole)
    assert [sum(c) for c in zip(*(p.counts(3) for p in parts))] == counts
    flat = np.ascontiguousarray(hits).reshape(-1)                          # two uneven chunks of the flat batch: key0 = i0
    cut = 1013
    parts = [fresh_walk(frame, key0=i0, hits=np.ascontiguousarray(flat[i0:i1])) for i0, i1 in ((0, cut), (cut, len(flat)))]
    assert indirect_ref.same_bits(np.concatenate([p.term(3) for p in parts]), whole.reshape(-1, 3))


# ---- 4. the mutation study: every wrong rule shows on a named input ----------------------------------------------------------------

def inside_records():
    """made-up records inside the built-in scene's diffuse sphere 4 (centre (-2.5, 3, 1), radius 1): every gather ray meets the
    sphere from within, so that g_0 carries RT_HIT_INSIDE"""
    rng = np.random.RandomState(3)
    hits = np.zeros(24, dtype=query_ref.HIT_DTYPE)
    N = rng.normal(size=(24, 3))
    hits["object"] = 4
    hits["point"] = (np.array([-2.5, 3.0, 1.0]) + rng.uniform(-0.3, 0.3, (24, 3))).astype(F)
    hits["normal"] = (N / np.linalg.norm(N, axis=1)[:, None]).astype(F)
    hits["color"] = F(1.0)
    hits["distance"] = F(1.0)
    return hits


def mutation_inputs():
    """rule -> (frame, the records (None: the frame's), key0, B)"""
    builtin = FRAME["builtin"]
    strip = np.ascontiguousarray(indirect_ref.oracle_gather(*builtin)[1][20:41])
    return {"same_seed": (builtin, None, 0, 2), "flat_key": (builtin, strip, 20 * 37, 2), "no_late_mask": (builtin, None, 0, 2),
            "backward": (builtin, None, 0, 3), "late_T": (FRAME["twomirrors"], None, 0, 3), "no_flip": (builtin, inside_records(), 0, 2),
            "dead_only": (FRAME["twomirrors"], None, 0, 2)}


@pytest.mark.parametrize("rule", paths_ref.RULES)
def test_every_wrong_rule_changes_an_output_word_or_an_alive_count(rule):
    frame, hits, key0, B = mutation_inputs()[rule]
    right, wrong = fresh_walk(frame, None, key0, hits), fresh_walk(frame, rule, key0, hits)
    words = int((bits(right.term(B)) != bits(wrong.term(B))).sum())
    counts = right.counts(B) != wrong.counts(B)
    print(rule, "words", words, "counts", right.counts(B), wrong.counts(B))
    assert words > 0 or counts, rule
    if rule in ("late_T", "dead_only"):                                   # these two show in the counts alone
        assert counts and words == 0
    else:
        assert words > 0
    if rule == "no_flip":
        assert ((right.g["flags"] & ao_ref.HIT_INSIDE) != 0).sum() >= 24        # the input does reach inside records


def test_the_study_covers_every_rule_the_issue_names():
    assert set(mutation_inputs()) == set(paths_ref.RULES) and len(paths_ref.RULES) == 7


# ---- 5. the executable ------------------------------------------------------------------------------------------------------------

def test_the_usage_text_names_the_bounces():
    r = subprocess.run([EXE, "--no-such-option"], capture_output=True, text=True)
    assert r.returncode == 1 and "usage:" in r.stderr and "--indirect-bounces B" in r.stderr


@pytest.mark.parametrize("args", [["--indirect-bounces", "2"], ["--indirect", "2", "--indirect-bounces", "0"],
                                  ["--indirect", "2", "--indirect-bounces", "9"], ["--indirect", "2", "--indirect-bounces", "x"],
                                  ["--indirect", "2", "--indirect-bounces"], ["--indirect", "2", "--indirect-bounces", "2:1"]])
def test_the_executable_refuses_bad_bounces_with_a_usage_error(args, tmp_path):
    r = subprocess.run([EXE, "--width", "8", "--height", "8", "--no-txt"] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 1 and "usage:" in r.stderr and "--indirect-bounces" in r.stderr, (args, r.stderr)
    assert "Start Ray Tracing" not in r.stdout and not os.listdir(tmp_path)
