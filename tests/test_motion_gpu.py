"""Temporal accumulation that follows moving objects (include/rt_motion.h) on the GPU against its definition:
rt_motion_accumulate and rt_motion_accumulate_device against motion_ref word for word -- value, moments, length, variance and
flags -- over the pose pairs whose conditions test_motion_cpu.py counts on the oracle's records, static tables against the
existing call, made-up records under a made-up table of 4096 entries on either side of every table path's threshold, NaN and
infinity in the previous frame, strips, TemporalHistory.push(motions=) against the host calls and render_animated against the
composition of the public calls.  The device entry point writes into sentinel-filled guarded outputs.  Bar: BIT-EXACT."""
import ctypes as C

import numpy as np
import pytest

import motion_ref
import motion_scenes
import poisoned
import temporal_ref
from large_extents import SENTINEL_BYTE, Guarded
from test_motion_cpu import made_up_case, made_up_table
from test_temporal_cpu import PAIRS, made_up_history, pair_records
from test_temporal_gpu import NAMES, OPTIONS, assert_all_same
from test_upsample_gpu import random_frame
from tilecoderaytracer_amd import (Renderer, TemporalHistory, capi, motion_accumulate, render_animated,
                                   temporal_accumulate)
from tilecoderaytracer_amd.renderer import temporal_params

pytestmark = pytest.mark.gpu

F = np.float32
LDS_ENTRIES = 170                                               # the largest table the LDS path takes (csrc/rt_accumulate_body.h)


def device_accumulate(cur, hits, cam, prev, motions, want, x0=0, W=None, optional=True, **kw):
    """rt_motion_accumulate_device into sentinel-filled outputs -> the five outputs (variance and flags None without
    `optional`); every word of the outputs written, none beside, and no input -- the table among them -- changed"""
    import torch
    channels = 3 if cur.ndim == 3 else 1
    Wn, H = hits.shape
    W = (prev[1].shape[0] if prev is not None else x0 + Wn) if W is None else W
    params = temporal_params(channels, **kw)
    n_motions = 0 if motions is None else len(motions)
    what = f"rt_motion_accumulate_device {W}x{H} columns {x0}:{x0 + Wn} channels {channels} n_motions {n_motions} {kw}"
    poisoned.assert_reference_has_no_sentinel(list(want[:4]), what)
    inputs = [cur, hits] + (list(prev[1:]) if prev is not None else [])
    if n_motions:
        inputs.append(np.ascontiguousarray(motions, dtype=F))
    d_in = [poisoned._on_device(np.ascontiguousarray(a).reshape(-1).view(np.int32)) for a in inputs]
    before = [t.clone() for t in d_in]
    n = Wn * H
    specs = [(n * channels, channels, False), (n * 2, 2, False), (n, 1, False), (n, 1, False), (n, 1, True)]
    bufs = [Guarded(words + poisoned.SLACK_CELLS * per, as_bytes=b) for words, per, b in specs]
    out_ptrs = [g.ptr for g in bufs] if optional else [g.ptr for g in bufs[:3]] + [None, None]
    prev_ptrs = [t.data_ptr() for t in d_in[2:6]] if prev is not None else [None] * 4
    table_ptr = d_in[-1].data_ptr() if n_motions else None
    assert table_ptr is None or table_ptr % 16 == 0
    capi.check(capi.load_library().rt_motion_accumulate_device(
        0, C.byref(params), C.byref(prev[0]) if prev is not None else None, C.byref(cam), W, H, x0, x0 + Wn, table_ptr, n_motions,
        d_in[0].data_ptr(), d_in[1].data_ptr(), *prev_ptrs, *out_ptrs, poisoned._stream()))
    torch.cuda.synchronize()
    for t, b in zip(d_in, before):
        assert torch.equal(t, b), f"{what}: an input was written"
    out = []
    for k, (g, (words, per, as_bytes)) in enumerate(zip(bufs, specs)):
        host = g.all.cpu().numpy()
        if k >= 3 and not optional:
            assert g.sentinels_left() == g.n and g.guards_untouched()
            out.append(None)
            continue
        body = poisoned.check_output(host[:g.guard], host[g.guard:g.guard + g.n], host[g.guard + g.n:], words,
                                     poisoned.layout(per, H, x0), f"{what}, {NAMES[k]}", SENTINEL_BYTE if as_bytes else poisoned.SENTINEL)
        out.append(body.copy())
    shape = (Wn, H)
    flags = out[4]
    if flags is not None:
        assert ((flags == 0) | (flags == 1)).all()
        flags = flags.reshape(shape).view(np.bool_)
    return (out[0].view(F).reshape(shape + ((3,) if channels == 3 else ())), out[1].view(F).reshape(shape + (2,)),
            out[2].view(F).reshape(shape), out[3].view(F).reshape(shape) if out[3] is not None else None, flags)


def both_ways(cur, hits, cam, prev, motions, what, x0=0, W=None, want=None, **kw):
    """the host call and the device entry point against the reference (or `want`) -> the reference's outputs"""
    if want is None:
        want = motion_ref.accumulate(cur, hits, cam, prev, motions, x0=x0, W=W, **kw)
    assert_all_same(motion_accumulate(cur, hits, cam, prev, motions, x0=x0, W=W, **kw), want, f"{what} {kw}")
    assert_all_same(device_accumulate(cur, hits, cam, prev, motions, want, x0=x0, W=W, **kw), want, f"{what} {kw}, device")
    return want


# ---- 1. the pose pairs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(61, 37), (96, 80)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(motion_scenes.PAIRS))
def test_a_pose_pairs_frame_is_the_reference_word_for_word(name, size):
    W, H = size
    cam_prev, cam, prev_hits, hits = motion_scenes.records(name, W, H)
    table = motion_scenes.table(name)
    rng = np.random.default_rng(W + len(name))
    moving = motion_ref.moving_records(hits, table)
    for channels, kw in OPTIONS:
        cur = rng.random((W, H, 3) if channels == 3 else (W, H), dtype=F)
        prev = (cam_prev, prev_hits) + made_up_history(H + channels, W, H, channels)
        want = both_ways(cur, hits, cam, prev, table, f"{name} {W}x{H}", **kw)
        if kw.get("normal_cos", 0.9) == 0.9 and kw.get("plane_eps", 0.05) == 0.05:
            # the conditions test_motion_cpu.py counts: a kernel that ignored the table would fail by the third
            with_table = int((~want[4])[moving].sum())
            without = int((~temporal_ref.accumulate(cur, hits, cam, prev, **kw)[4])[moving].sum())
            assert moving.sum() >= 80 and 4 * with_table >= 3 * moving.sum() and 3 * without <= 2 * with_table, (name, kw)
    want = motion_ref.accumulate(cur, hits, cam, prev, table)                    # without the optional outputs
    got = device_accumulate(cur, hits, cam, prev, table, want, optional=False)
    assert_all_same(got[:3], want[:3], f"{name} without variance and flags")
    both_ways(cur, hits, cam, None, table, f"{name}, first frame")               # the table is never read: any address would do


# ---- 2. static tables against the existing call ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PAIRS)
def test_static_tables_give_the_existing_calls_words(name):
    W, H = 61, 37
    cam_prev, cam, prev_hits, hits = pair_records(name, W, H)
    live = ~temporal_ref.dead_records(hits)
    lowest = int(hits["object"][live].min())
    rng = np.random.default_rng(len(name) + 1)
    cur = rng.random((W, H, 3), dtype=F)
    prev = (cam_prev, prev_hits) + made_up_history(9, W, H, 3)
    want = temporal_accumulate(cur, hits, cam, prev)                              # the existing GPU call
    identity = np.tile(motion_ref.IDENTITY, (LDS_ENTRIES + 1, 1))
    for what, motions in (("NULL", None), ("n_motions 0", np.zeros((0, 12), dtype=F)), ("identity", identity),
                          ("identity, short", identity[:14]), ("too short", rng.random((lowest, 12), dtype=F))):
        both_ways(cur, hits, cam, prev, motions, f"{name} {what}", want=want)
    assert (~want[4]).sum() >= 20


# ---- 3. made-up records under a made-up table ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(67, 70), (5, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_made_up_records_under_a_made_up_table(size):
    Wn, H = size
    cam_prev, cam, prev_hits, hits = made_up_case(Wn, H, 11 if Wn == 67 else 21)
    table = made_up_table(3)
    assert np.isnan(table).any() and np.isinf(table).any() and (table.view(np.uint32) == 0x80000000).any()
    rng = np.random.default_rng(14)
    live = ~temporal_ref.dead_records(hits)
    for channels, kw in ((3, dict(normal_cos=0.3, plane_eps=0.5)), (1, dict(normal_cos=-1.0, plane_eps=0.2, max_history=3, alpha=0.5))):
        cur = rng.random((Wn, H, 3) if channels == 3 else (Wn, H), dtype=F)
        prev = (cam_prev, prev_hits) + made_up_history(15, Wn, H, channels)
        for n in (0, 1, 7, LDS_ENTRIES, LDS_ENTRIES + 1, 4096):
            motions = table[:n]
            want = both_ways(cur, hits, cam, prev, motions, f"made-up records, n_motions {n}", **kw)
            moving = motion_ref.moving_records(hits, motions)
            if n:
                assert moving.sum() >= 3 and (live & ~moving).sum() >= 60, (n, int(moving.sum()))
            if n == 4096 and Wn == 67:
                assert (~want[4]).sum() >= 300 and want[4][live].sum() >= 300, (kw, int((~want[4]).sum()), int(want[4][live].sum()))
                assert moving.sum() >= 1000 and (~want[4])[moving].sum() >= 100 and want[4][moving].sum() >= 100
    # equal cameras: a moving record is reprojected, a static one takes its own cell
    want = both_ways(cur, hits, cam, (cam, prev_hits) + prev[2:], table, "made-up records, equal cameras", **kw)
    info = motion_ref.accumulate(cur, hits, cam, (cam, prev_hits) + prev[2:], table, details=True, **kw)[5]
    assert info["identity"].sum() >= 60 and info["moving"].sum() >= 60


# ---- 4. NaN and infinity in the previous frame --------------------------------------------------------------------------------------

def test_nan_and_infinity_in_the_previous_frame_under_a_moving_table():
    W, H = 61, 37
    cam_prev, cam, prev_hits, hits = pair_records("truck", W, H)
    prev_hits = prev_hits.copy()
    rng = np.random.default_rng(5)
    value, moments, length = made_up_history(6, W, H, 3)
    pick = lambda share: rng.random((W, H)) < share
    value[pick(0.03), 1] = np.nan
    value[pick(0.03), 2] = np.inf
    moments[pick(0.03), 0] = -np.inf
    moments[pick(0.03), 1] = np.nan
    length[pick(0.03)] = np.inf
    length[pick(0.03)] = np.nan
    prev_hits["normal"][pick(0.05), 1] = np.nan
    prev_hits["normal"][pick(0.02), 0] = np.inf
    prev_hits["point"][pick(0.03), 2] = np.nan
    cur = rng.random((W, H, 3), dtype=F)
    # every object of the built-in scene a little moved, some by a motion that holds a NaN or an infinity itself
    table = made_up_table(8, 64)
    for kw in (dict(), dict(plane_eps=0.0, max_history=4, alpha=0.2)):
        want = both_ways(cur, hits, cam, (cam_prev, prev_hits, value, moments, length), table, "NaN and infinity", **kw)
        assert np.isnan(want[0]).sum() > 20 and np.isnan(want[1]).sum() > 20 and np.isfinite(want[2]).all()
        assert motion_ref.moving_records(hits, table).sum() > 300 and (~want[4]).sum() > 300


# ---- 5. strips -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["spheres_equal", "box_dolly"])
def test_a_strip_equals_the_frames_columns(name):
    W, H, x0, x1 = 61, 37, 16, 48
    cam_prev, cam, prev_hits, hits = motion_scenes.records(name, W, H)
    table = motion_scenes.table(name)
    cur = np.random.default_rng(3).random((W, H, 3), dtype=F)
    prev = (cam_prev, prev_hits) + made_up_history(4, W, H, 3)
    frame = motion_accumulate(cur, hits, cam, prev, table)
    part_cur, part_hits = np.ascontiguousarray(cur[x0:x1]), np.ascontiguousarray(hits[x0:x1])
    want = both_ways(part_cur, part_hits, cam, prev, table, f"{name} strip", x0=x0)
    assert_all_same(want, [a[x0:x1] for a in frame], f"{name}: the strip against the frame's columns")
    moving = motion_ref.moving_records(part_hits, table)
    assert moving.sum() >= 50 and (~want[4])[moving].sum() >= 30 and want[4].sum() >= 5


# ---- 6. the history object and the animated render -------------------------------------------------------------------------------------

SEQUENCE = [motion_scenes.REST, motion_scenes.SHIFTED, dict(motion_scenes.SHIFTED, angle=0.3, axis=(0.3, -0.2, 1.0)),
            dict(motion_scenes.TURNED, shifts={1: (0.2, 0.2, 0.1)})]
CAMERAS = ["equal", "equal", "truck", "truck"]                   # the current camera of camera_pair(): frames 0 1 and 2 3 are equal


def sequence_tables():
    from tilecoderaytracer_amd import object_motions
    hosts = [motion_scenes.host(p) for p in SEQUENCE]
    return hosts, [None] + [object_motions(a.desc, b.desc) for a, b in zip(hosts, hosts[1:])]


def test_temporal_history_push_with_motions_over_four_frames_equals_four_host_calls():
    import query_ref
    from rays_ref import camera_rays
    W, H = 61, 37
    kw = dict(max_history=3, alpha=0.1)
    rng = np.random.default_rng(7)
    history = TemporalHistory(W, H, 3, **kw)
    _, tables = sequence_tables()
    state = None
    for k, (pose, cam_name, table) in enumerate(zip(SEQUENCE, CAMERAS, tables)):
        cam = motion_scenes.camera_pair(cam_name)[1]
        hits = query_ref.intersect(query_ref.Scene(motion_scenes.oracle(pose)), camera_rays(cam, W, H))
        cur = rng.random((W, H, 3), dtype=F)
        value, moments, length, variance, flags = motion_accumulate(cur, hits, cam, state, table, **kw)
        if k == 2:                                               # a frame pushed as two strips
            parts = [history.push(cur[:23], hits[:23], cam, 0, 23, motions=table), history.push(cur[23:], hits[23:], cam, 23, motions=table)]
            got = [np.concatenate([a, b]) for a, b in zip(*parts)]
        elif k == 3:                                             # a table that is on the device already
            import torch
            got = history.push(cur, hits, cam, motions=torch.tensor(table.reshape(-1), device="cuda"))
        else:
            got = history.push(cur, hits, cam, motions=table)
        assert_all_same(got, (value, variance, flags), f"push {k}")
        moving = motion_ref.moving_records(hits, table)
        assert flags.all() == (k == 0) and (k == 0 or ((~flags).sum() > 1000 and (~flags)[moving].sum() >= 100))
        state = (cam, hits, value, moments, length)
        kept = history.state()
        assert_all_same(kept[2:], state[2:], f"state after push {k}")
        assert kept[1].tobytes() == hits.tobytes() and history.frames == k + 1
    assert length.max() == 3
    # without a table the pushes are what they were
    plain = TemporalHistory(W, H, 3, **kw)
    assert_all_same(plain.push(cur, hits, cam), [a for k, a in enumerate(temporal_accumulate(cur, hits, cam, **kw)) if k in (0, 3, 4)], "plain")


@pytest.mark.parametrize("term", ["indirect", "ao", "direct"])
def test_render_animated_is_the_composition_of_the_public_calls(term):
    W, H, depth = 45, 38, 3
    hosts, tables = sequence_tables()
    renderers = [Renderer(h) for h in hosts]
    cams = [motion_scenes.camera_pair(n)[1] for n in CAMERAS]
    kw = dict(max_history=3, alpha=0.05, plane_eps=0.02)
    term_kw = dict(indirect=dict(gather_depth=1, gain=1.25), ao=dict(radius=2.0), direct=dict())[term]
    state = None
    for k, (r, cam, table) in enumerate(zip(renderers, cams, tables)):
        own = r._cam
        r._cam = C.pointer(cam)
        if term == "direct":
            r.set_shadow_seed(k)
        rgb, hits = r.render_gbuffer(W, H, depth)
        cur = rgb if term == "direct" else r.indirect_diffuse(hits, 1, seed=k, base=rgb, **term_kw) if term == "indirect" \
            else r.ambient_occlusion(hits, 1, seed=k, **term_kw)
        r._cam = own
        value, moments, length, variance, flags = motion_accumulate(cur, hits, cam, state, table, **kw)
        state = (cam, hits, value, moments, length)
    owned = [r._cam for r in renderers]
    got = render_animated(list(zip(renderers, cams, tables)), W, H, depth, term=term, samples=1, **kw, **term_kw)
    assert all(r._cam is c for r, c in zip(renderers, owned))
    assert_all_same(got, (value, variance, flags), f"render_animated {term}")
    moving = motion_ref.moving_records(hits, tables[-1])
    assert (~flags).sum() > 1000 and moving.sum() >= 80 and (~flags)[moving].sum() >= 60 and length.max() == 3
    # the same frames without their tables: the movers' history is shorter
    plain = render_animated([(r, c, None) for r, c in zip(renderers, cams)], W, H, depth, term=term, samples=1, **kw, **term_kw)
    assert plain[2][moving].sum() > flags[moving].sum()
    with pytest.raises(ValueError):
        render_animated(list(zip(renderers, cams, tables)), W, H, depth, term="glossy")
    with pytest.raises(ValueError):
        render_animated([], W, H, depth)
    for r in renderers:
        r.close()


# ---- 7. the device entry point's refusals -------------------------------------------------------------------------------------------

def test_device_entry_refuses_and_the_next_call_is_unharmed():
    import torch
    W, H = 20, 70
    hits = random_frame(8, W, H)
    cur = np.random.default_rng(9).random((W, H, 3), dtype=F)
    cam_prev, cam = motion_scenes.camera_pair("truck")
    prev = (cam_prev, hits) + made_up_history(10, W, H, 3)
    table = made_up_table(3, 8)
    d_hits = poisoned._on_device(hits.reshape(-1).view(np.int32))
    d = [poisoned._on_device(a.view(np.int32)) for a in (cur,) + prev[2:]]
    d_table = poisoned._on_device(np.concatenate([np.zeros(4, np.int32), table.reshape(-1).view(np.int32)]))
    g = [Guarded(W * H * k) for k in (3, 2, 1)]
    lib = capi.load_library()
    params = temporal_params(3)
    call = lambda table_ptr, n, out_value: lib.rt_motion_accumulate_device(
        0, C.byref(params), C.byref(cam_prev), C.byref(cam), W, H, 0, W, table_ptr, n, d[0].data_ptr(), d_hits.data_ptr(),
        d_hits.data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), out_value, g[1].ptr, g[2].ptr, None, None, poisoned._stream())
    good = d_table.data_ptr() + 16
    for table_ptr, n, out_value, word in ((good - 8, 8, g[0].ptr, "16-byte"), (good + 4, 0, g[0].ptr, "16-byte"), (good, 4097, g[0].ptr, "n_motions must"),
                                          (good, -1, g[0].ptr, "n_motions must"), (None, 1, g[0].ptr, "motions is NULL"),
                                          (good, 8, good, "overlaps the motion table"), (good, 8, good + 8 * 48 - 4, "overlaps the motion table"),
                                          (good, 8, d[1].data_ptr(), "overlaps a prev_")):
        rc = call(table_ptr, n, out_value)
        assert rc == capi.RT_ERR_INVALID and word in lib.rt_last_error().decode(), (word, lib.rt_last_error().decode())
    torch.cuda.synchronize()
    for buf in g:
        assert buf.sentinels_left() == buf.n and buf.guards_untouched()          # nothing was launched
    both_ways(cur, hits, cam, prev, table, "after the refusals", normal_cos=0.0)
