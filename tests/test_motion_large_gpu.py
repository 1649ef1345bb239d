"""The accumulation kernel (csrc/rt_accumulate_body.h) REPROJECTED on a frame of 16 400 x 16 400, through both calls that share
it -- rt_temporal_accumulate_device with three channels, rt_motion_accumulate_device with one channel and a table read from
global memory -- by test_temporal_large_gpu.py's ground rules.  That test has equal cameras, so a pixel's only tap is its own
cell; here the cameras differ, every live pixel takes the four taps around floorf(px), floorf(pz), and the 257 x 4100 = 1 053 700
tiles of 256 pixels are more than the 2^20 workgroups of a launch, so some workgroups make a second trip through the tile loop.
The records (12.9 GB) pass 2^32 bytes three times; the previous frame's moments cross 2^31 at the pixel of the records' 3 * 2^32,
and prev_value with three channels crosses 2^31 at the pixel of their 2 * 2^32 (it is 3.2 GB: there is no 2^32 of it in a frame
that fits a test's memory together with everything else; test_temporal_large_gpu.py's 18 944^2 frame has one channel).

To fit the memory the previous frame's records are the frame's own: the scene stands still and the previous camera is a small
truck of the current one, so a point reprojects a few columns beside its own pixel; plane_eps 0 and normal_cos -1 leave the key
-- object and side -- to decide each tap.  The table of run M moves three objects by a rotation of 3e-4 rad and a shift of a
millimetre or two, which keeps their taps as near."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import adaptive_frames
import cameras
import large_extents as le
import motion_ref
import motion_scenes
import query_ref
import temporal_ref
from large_extents import Guarded, hashed
from test_query_gpu import assert_hits_same
from tilecoderaytracer_amd import HostScene, Renderer, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE, temporal_params

pytestmark = pytest.mark.gpu
F = np.float32
B31, B32 = 1 << 31, 1 << 32
W = H = 16400
N = W * H
LDS_ENTRIES = 170                                               # test_motion_gpu.py's: one entry more and no build stages the table
MOVED = (2, 4, 5)                                               # the built-in scene's spheres (cameras.ANCHORS)
REACH = 64                                                      # the most columns a tap may lie beside its pixel's
KW = dict(max_history=4, normal_cos=-1.0, plane_eps=0.0, alpha_moments=0.25)
NAMES = ("value", "moments", "length", "variance", "flags")


def camera_pair():
    """-> (previous camera, current camera): the built-in scene's own, and before it the same camera 0.004 to the side and 0.0015
    up, a few columns and rows of parallax at the scene's depths"""
    eye, look = np.array(cameras.ANCHORS["builtin"]["eye"]), np.array(cameras.ANCHORS["builtin"]["look"])
    out = (look - eye) / np.linalg.norm(look - eye)
    h = np.cross(out, (0.0, 0.0, 1.0))
    h = h / np.linalg.norm(h)
    d = 0.004 * h + 0.0015 * np.cross(h, out)
    return cameras.camera(eye + d, look + d), cameras.camera(eye, look)


def motion_table():
    """LDS_ENTRIES + 1 entries, the identity's bits but for MOVED: each a rotation by 3e-4 rad about an axis of its own through
    the scene's focus and a shift below 2e-3"""
    table = np.tile(motion_ref.IDENTITY, (LDS_ENTRIES + 1, 1))
    rng = np.random.default_rng(16400)
    c = np.array(cameras.ANCHORS["builtin"]["focus"])
    for o in MOVED:
        R = motion_scenes.rotation(rng.normal(size=3), 3e-4)
        t = rng.uniform(-1.0, 1.0, 3) * 1.2e-3
        table[o] = np.concatenate([R, (c - R @ c + t)[:, None]], axis=1).reshape(12).astype(F)
    table.setflags(write=False)
    return table


def boundary_runs():
    """the runs of columns compared with the Python reference: the first, the last, and those around the records' 2^32, 2 * 2^32
    and 3 * 2^32 bytes and prev_value's 2^31 with three channels (the pixel of the records' 2 * 2^32)"""
    cols = set(le.boundary_columns([B32, 2 * B32, 3 * B32], 48 * H, W)) | set(le.boundary_columns([B31], 12 * H, W))
    assert 12 * N < B32 < 16 * N and 8 * N > B31
    return le.runs(sorted(cols))


@functools.lru_cache(maxsize=None)
def oracle_column(x):
    cam = camera_pair()[1]
    records = query_ref.intersect(oracle_column.scene(), le.column_rays(cam, W, H, x, x + 1))
    records.setflags(write=False)
    return records


oracle_column.scene = functools.lru_cache(maxsize=None)(lambda: query_ref.Scene(adaptive_frames.oracle_scene("builtin")))


def oracle_columns(x0, x1):
    return np.concatenate([oracle_column(x) for x in range(x0, x1)])


def reference(kind, cur, records, x0, prev_records, prev_words, prev_x0, **more):
    """temporal_ref (run T) or motion_ref with the table (run M) over columns [x0, x0 + n) with the previous frame's columns
    from prev_x0"""
    cam_prev, cam = camera_pair()
    prev = (cam_prev, prev_records) + tuple(prev_words)
    if kind == "T":
        return temporal_ref.accumulate(cur, records, cam, prev, x0=x0, W=W, prev_x0=prev_x0, **KW, **more)
    return motion_ref.accumulate(cur, records, cam, prev, motion_table(), x0=x0, W=W, prev_x0=prev_x0, **KW, **more)


def points_before(kind, records):
    """where the records' points were in the previous frame: their own, but a moving record's"""
    if kind == "T":
        return records["point"]
    return motion_ref.moved(records, motion_table(), motion_ref.moving_records(records, motion_table()))[0]


@functools.lru_cache(maxsize=None)
def input_conditions(kind):
    """The conditions on the inputs, counted without a GPU on the oracle's records of the boundary columns and of the previous
    frame's columns their taps reach -> dict of counts: pixels with and without history, pixels with history whose first tap
    (floorf(px), floorf(pz)) is not their own cell, moving records with history, and the widest reach in columns."""
    cam_prev, _ = camera_pair()
    channels = 3 if kind == "T" else 1
    got = dict(history=0, without=0, other_cell=0, moving_history=0, reach=0)
    for c0, c1 in boundary_runs():
        records = oracle_columns(c0, c1)
        before = points_before(kind, records)
        lo, hi = temporal_ref.tap_columns(cam_prev, records, W, H, before) or (c0, c1)   # (None: every point left the frame)
        got["reach"] = max(got["reach"], c0 - lo, hi - c1)
        n = hi - lo
        words = (np.zeros((n, H, 3) if channels == 3 else (n, H), dtype=F), np.zeros((n, H, 2), dtype=F), np.ones((n, H), dtype=F))
        cur = np.zeros((c1 - c0, H, 3) if channels == 3 else (c1 - c0, H), dtype=F)
        out = reference(kind, cur, records, c0, oracle_columns(lo, hi), words, lo, details=True)
        history = ~out[4]
        with np.errstate(all="ignore"):
            _, px, pz = temporal_ref.project(cam_prev, before, W, H)
        x, z = np.meshgrid(np.arange(c0, c1), np.arange(H), indexing="ij")
        got["history"] += int(history.sum())
        got["without"] += int((~history).sum())
        got["other_cell"] += int((history & ((np.floor(px) != x) | (np.floor(pz) != z))).sum())
        if kind == "M":
            got["moving_history"] += int((history & out[5]["moving"]).sum())
    return got


def assert_conditions(got, kind):
    assert got["history"] >= 1000 and got["without"] >= 1000 and got["other_cell"] >= 1000, got
    assert got["reach"] <= REACH, got
    if kind == "M":
        assert got["moving_history"] >= 300, got


def accumulate_large(kind):
    import torch
    channels = 3 if kind == "T" else 1
    per = (channels, 2, 1, 1, 1)
    need = Guarded.need(12 * N) + Guarded.need(3 * N) + (2 * channels + 3) * 4 * N + sum(Guarded.need(N * k) for k in per[:4]) \
        + Guarded.need(N, as_bytes=True) + sum(Guarded.need(le.STRIP_COLUMNS * H * k) for k in per) + (3 << 30)
    le.require_device_memory(need)
    t0 = time.time()
    conditions = input_conditions(kind)
    assert_conditions(conditions, kind)
    lib = capi.load_library()
    cam_prev, cam = camera_pair()
    params = temporal_params(channels, False, KW["max_history"], KW["normal_cos"], KW["plane_eps"], 0.0, KW["alpha_moments"])
    table = motion_table()
    name = "rt_temporal_accumulate_device" if kind == "T" else f"rt_motion_accumulate_device with {len(table)} motions"
    what = f"{name} {W}x{H} channels {channels}"
    host = HostScene.builtin()
    r = Renderer(host)
    own = r._cam
    bufs = []
    cur = p_value = p_len = p_moments = d_table = None
    try:
        hits, colours = Guarded(12 * N), Guarded(3 * N)
        bufs += [hits, colours]
        r._cam = C.pointer(cam)
        r.render_gbuffer_device(W, H, 0, 0, W, colours.ptr, hits.ptr)
        torch.cuda.synchronize()
        hits.assert_written("the frame's records")
        colours.free()
        torch.cuda.empty_cache()
        cur, p_value, p_len = hashed(channels * N, 1), hashed(channels * N, 2), hashed(N, 3, 5.0, 1.0)
        p_moments = hashed(2 * N, 4)
        d_table = torch.from_numpy(table.copy()).cuda()
        assert d_table.data_ptr() % 16 == 0
        ins = [t.view(torch.int32) for t in (cur, p_value, p_moments, p_len, d_table)] + [hits.body]
        before = [le.checksum(t) for t in ins]
        out = [Guarded(N * k) for k in per[:4]] + [Guarded(N, as_bytes=True)]
        bufs += out

        def call(x0, x1, ptrs):
            head = (0, C.byref(params), C.byref(cam_prev), C.byref(cam), W, H, x0, x1)
            rest = (cur.data_ptr() + x0 * H * 4 * channels, hits.ptr + x0 * H * 48, hits.ptr, p_value.data_ptr(), p_moments.data_ptr(),
                    p_len.data_ptr(), *ptrs, None)
            if kind == "T":
                capi.check(lib.rt_temporal_accumulate_device(*head, *rest))
            else:
                capi.check(lib.rt_motion_accumulate_device(*head, d_table.data_ptr(), len(table), *rest))

        call(0, W, [g.ptr for g in out])
        torch.cuda.synchronize()
        for g, output in zip(out, NAMES):
            g.assert_written(f"{what}, {output}")
        without = le.count_equal(out[4].body, 1)
        assert without + le.count_equal(out[4].body, 0) == N and 1000 <= without <= N - 1000
        assert le.count_equal(out[2].body.view(torch.float32), 4.0) > 1000           # max_history reached
        # (1) every word against the same kernel's strips: one trip through the tile loop each
        small = [Guarded(le.STRIP_COLUMNS * H * k, as_bytes=(n == 4)) for n, k in enumerate(per)]
        bufs += small
        for x0 in range(0, W, le.STRIP_COLUMNS):
            x1 = min(x0 + le.STRIP_COLUMNS, W)
            for s in small:
                s.refill()
            call(x0, x1, [s.ptr for s in small])
            torch.cuda.synchronize()
            for k, (big, s) in enumerate(zip(out, small)):
                words = (x1 - x0) * H * per[k]
                s.assert_written(f"{what}: {NAMES[k]} of strip {x0}:{x1}", words)
                assert s.sentinels_left() == s.n - words, f"{what}: {NAMES[k]} of strip {x0}:{x1} was written past its end"
                if k == 4:
                    assert torch.equal(big.body[x0 * H:x1 * H], s.body[:words]), f"{what}: flags of columns {x0}:{x1}"
                else:
                    text = le.device_difference(big.body[x0 * H * per[k]:x1 * H * per[k]], s.body[:words], H * per[k],
                                                f"{what}: {NAMES[k]}, columns {x0}:{x1} against their own strip", x0)
                    assert text is None, text
        # (2) the boundary columns against the Python reference, which sees those columns and their taps' alone
        sl = lambda t, k, a, b: t[a * H * k:b * H * k].cpu().numpy()
        shaped = lambda a, n, k: a.view(F).reshape((n, H, k) if k > 1 else (n, H))
        for c0, c1 in boundary_runs():
            records = sl(hits.body, 12, c0, c1).view(HIT_DTYPE).reshape(c1 - c0, H)
            assert_hits_same(records, oracle_columns(c0, c1), f"{what}: the records of columns {c0}:{c1}, which the conditions were counted on")
            lo, hi = temporal_ref.tap_columns(cam_prev, records, W, H, points_before(kind, records)) or (c0, c1)
            assert c0 - lo <= REACH and hi - c1 <= REACH, (c0, c1, lo, hi)
            prev_words = (shaped(sl(p_value, channels, lo, hi), hi - lo, channels), shaped(sl(p_moments, 2, lo, hi), hi - lo, 2),
                          shaped(sl(p_len, 1, lo, hi), hi - lo, 1))
            want = reference(kind, shaped(sl(cur, channels, c0, c1), c1 - c0, channels), records, c0,
                             sl(hits.body, 12, lo, hi).view(HIT_DTYPE).reshape(hi - lo, H), prev_words, lo)
            for k, (g, w) in enumerate(zip(out, want)):
                got = sl(g.body, per[k], c0, c1)
                w = np.ascontiguousarray(w).reshape(-1)
                as_words = np.uint8 if k == 4 else np.int32
                d = le.first_difference(got.view(as_words), w.view(as_words))
                assert d is None, (f"{what}: {NAMES[k]}, columns {c0}:{c1} against the reference: {d[3]} words differ, first in "
                                   f"column {c0 + d[0] // (H * per[k])}, word {d[0] % (H * per[k])} of it")
        assert [le.checksum(t) for t in ins] == before, f"{what}: an input changed"
        assert all(g.guards_untouched() for g in out) and hits.guards_untouched()
        print(f"[large motion] {what}: {without} of {N} pixels without history; on the boundary columns {conditions}; "
              f"{time.time() - t0:.1f} s")
    finally:
        r._cam = own
        for g in bufs:
            g.free()
        cur = p_value = p_len = p_moments = d_table = ins = None
        torch.cuda.empty_cache()
        r.close()


def test_temporal_three_channels_reprojected_where_the_records_pass_2_32_bytes():
    """Run T: rt_temporal_accumulate_device, three channels, cameras that differ, max_history 4 over previous lengths 1..6, every
    output asked for.
    (1) every word of the five outputs equals the same kernel's on strips of 1024 columns (65 792 tiles: one trip through the
        tile loop) written at offset 0 of small guarded buffers: the addressing of the current records and values and of the
        outputs, and the loop `tile += gridDim.x` whose second trip only the full launch makes;
    (2) the first and last column and those around the records' 2^32, 2 * 2^32 and 3 * 2^32 bytes equal temporal_ref, which is
        given those columns and the previous frame's columns their taps reach, and raises if a tap falls beside them: a strip
        shares its tap addressing with the full launch, so only this catches an error there.
    The one-line narrowings this is there for (derived from the code; no narrowed kernel was built or run):
      `(int)(i * A.H + j)` for the tap's `cell` cannot wrap (a pixel number fits 31 bits at every accepted size), but
        `(uint32_t)(48 * cell) / 16` for `3 * index` in load_rec reads the taps of column 5456's upper part and of every later
        column from the frame's first columns: (2) differs wherever the keys differ, and (1) too, since a strip's current records
        are read at small offsets and its taps at large ones;
      `prev_value[(uint32_t)(12 * cell) / 4 ...]`, a byte offset in 32 bits, is right below 2^32 bytes and is not reached here;
        `(int32_t)` of it wraps at prev_value's 2^31, column 10 911, and (2) differs there;
      a 32-bit `tile` is enough for 1 053 700 tiles; `tile < (uint32_t)kMaxGroups` for `tile < A.tiles`, or a `return` for the
        `continue` after the barriers, ends the loop after one trip: the pixels of tiles 2^20.. -- columns 16 320 to 16 399 --
        keep the sentinel, which assert_written and (1) both report."""
    accumulate_large("T")


def test_motion_one_channel_with_a_table_in_global_memory_reprojected_where_the_records_pass_2_32_bytes():
    """Run M: rt_motion_accumulate_device, one channel, a table of LDS_ENTRIES + 1 entries -- the kTableGlobal kernel, which no
    other large test runs -- that moves the built-in scene's three spheres; otherwise run T, with motion_ref as (2)'s reference.
    The one-line narrowings this is there for (derived from the code; no narrowed kernel was built or run):
      those of run T, in the kernel's other instantiation;
      `motions + 3 * h.a.x` is small at every table the call accepts (4096 entries);
      the staging of the current records, `cur_hits + 3 * (xl * A.H + z0)` with `xl * A.H` in 32 bits, is right for a strip and
        for the full frame alike (below 2^31 pixels) -- but `(uint32_t)(48 * ...)` there reads the wrong records from column
        5456 on, and (1) differs since a strip's own offsets are small."""
    accumulate_large("M")
