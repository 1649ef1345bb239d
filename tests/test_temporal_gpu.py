"""Temporal accumulation (include/rt_temporal.h) on the GPU against its definition: rt_temporal_accumulate and
rt_temporal_accumulate_device against temporal_ref word for word -- value, moments, length, variance and flags -- over the camera
pairs whose conditions test_temporal_cpu.py counts on the oracle's records, over made-up records, strips, the first frame and the
identity path, NaN and infinity in the history, TemporalHistory against the host calls and render_accumulated against the
composition of the public calls.  The device entry point writes into sentinel-filled guarded outputs.  Bar: BIT-EXACT."""
import ctypes as C

import numpy as np
import pytest

import cameras
import poisoned
import temporal_ref
from large_extents import SENTINEL_BYTE, Guarded
from test_temporal_cpu import EYE, LOOK, PAIRS, made_up_history, pair_records
from test_upsample_gpu import assert_same, random_frame
from tilecoderaytracer_amd import HostScene, Renderer, TemporalHistory, capi, temporal_accumulate
from tilecoderaytracer_amd.renderer import HIT_DTYPE, temporal_params

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("value", "moments", "length", "variance", "flags")


def assert_all_same(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert_same(g, w, f"{what}: {name}")


def device_accumulate(cur, hits, cam, prev, want, x0=0, W=None, optional=True, **kw):
    """rt_temporal_accumulate_device into sentinel-filled outputs -> the five outputs (variance and flags None without
    `optional`); every word of the outputs written, none beside, and no input changed"""
    import torch
    channels = 3 if cur.ndim == 3 else 1
    Wn, H = hits.shape
    W = (prev[1].shape[0] if prev is not None else x0 + Wn) if W is None else W
    params = temporal_params(channels, **kw)
    what = f"rt_temporal_accumulate_device {W}x{H} columns {x0}:{x0 + Wn} channels {channels} {kw}"
    poisoned.assert_reference_has_no_sentinel(list(want[:4]), what)
    inputs = [cur, hits] + (list(prev[1:]) if prev is not None else [])
    d_in = [poisoned._on_device(np.ascontiguousarray(a).reshape(-1).view(np.int32)) for a in inputs]
    before = [t.clone() for t in d_in]
    n = Wn * H
    specs = [(n * channels, channels, False), (n * 2, 2, False), (n, 1, False), (n, 1, False), (n, 1, True)]
    bufs = [Guarded(words + poisoned.SLACK_CELLS * per, as_bytes=b) for words, per, b in specs]
    out_ptrs = [g.ptr for g in bufs] if optional else [g.ptr for g in bufs[:3]] + [None, None]
    prev_ptrs = [t.data_ptr() for t in d_in[2:]] if prev is not None else [None] * 4
    capi.check(capi.load_library().rt_temporal_accumulate_device(
        0, C.byref(params), C.byref(prev[0]) if prev is not None else None, C.byref(cam), W, H, x0, x0 + Wn, d_in[0].data_ptr(),
        d_in[1].data_ptr(), *prev_ptrs, *out_ptrs, poisoned._stream()))
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


def both_ways(cur, hits, cam, prev, what, x0=0, W=None, **kw):
    """the host call and the device entry point against the reference -> the reference's outputs"""
    want = temporal_ref.accumulate(cur, hits, cam, prev, x0=x0, W=W, **kw)
    assert_all_same(temporal_accumulate(cur, hits, cam, prev, x0=x0, W=W, **kw), want, f"{what} {kw}")
    assert_all_same(device_accumulate(cur, hits, cam, prev, want, x0=x0, W=W, **kw), want, f"{what} {kw}, device")
    return want


# ---- 1. the camera pairs of the built-in scene ------------------------------------------------------------------------------------

OPTIONS = [(3, dict()), (3, dict(match_color=True, alpha=0.2, alpha_moments=0.1)), (3, dict(plane_eps=0.0, max_history=4)),
           (1, dict(max_history=1)), (1, dict(match_color=True, plane_eps=0.0, alpha=0.2, max_history=4, normal_cos=0.5))]


@pytest.mark.parametrize("size", [(61, 37), (96, 80)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", PAIRS)
def test_a_moved_cameras_frame_is_the_reference_word_for_word(name, size):
    W, H = size
    cam_prev, cam, prev_hits, hits = pair_records(name, W, H)
    rng = np.random.default_rng(W + len(name))
    live = ~temporal_ref.dead_records(hits)
    for channels, kw in OPTIONS:
        cur = rng.random((W, H, 3) if channels == 3 else (W, H), dtype=F)
        prev = (cam_prev, prev_hits) + made_up_history(H + channels, W, H, channels)
        want = both_ways(cur, hits, cam, prev, f"{name} {W}x{H}", **kw)
        flags, length = want[4], want[2]
        assert flags[~live].all() and 20 <= (~flags).sum(), (name, kw)
        if name == "equal":
            assert not flags[live].any()
        else:
            assert flags[live].sum() >= 5, (name, kw)
        cap = kw.get("max_history", 32)
        assert length.max() <= cap and (cap > 4 or (length == cap).sum() >= 20), (name, kw)      # max_history 1 and 4 reached
    # without the optional outputs
    want = temporal_ref.accumulate(cur, hits, cam, prev)
    got = device_accumulate(cur, hits, cam, prev, want, optional=False)
    assert_all_same(got[:3], want[:3], f"{name} without variance and flags")


def test_the_first_frame_is_the_sample():
    W, H = 61, 37
    _, cam, _, hits = pair_records("truck", W, H)
    rng = np.random.default_rng(1)
    for channels in (1, 3):
        cur = rng.random((W, H, 3) if channels == 3 else (W, H), dtype=F)
        cur.reshape(-1).view(np.uint32)[7] = 0x7FC12345           # a NaN's payload survives: word for word
        cur.reshape(-1)[11:14] = [np.inf, -0.0, 1e-42]
        want = both_ways(cur, hits, cam, None, "first frame", max_history=1 if channels == 1 else 32)
        assert want[4].all() and (want[2] == 1).all() and (want[3].view(np.uint32) == 0).all()
        assert np.array_equal(want[0].view(np.uint32), cur.view(np.uint32))


def test_equal_cameras_take_the_identity_path_whatever_the_records_points_say():
    """the previous records differ from the current ones at made-up pixels -- another object, another side, another colour, a
    turned normal, a point off the plane -- and every other pixel's only tap is its own cell, even where its point is changed
    so that it would reproject elsewhere"""
    W, H = 61, 37
    cam_prev, cam, _, hits = pair_records("equal", W, H)
    prev_hits = hits.copy()
    rng = np.random.default_rng(2)
    pick = lambda share: rng.random((W, H)) < share
    prev_hits["object"][pick(0.05)] += 1
    prev_hits["flags"][pick(0.05)] ^= 1
    prev_hits["color"][pick(0.05)] *= F(0.5)
    turned = pick(0.05)
    prev_hits["normal"][turned] = prev_hits["normal"][turned][:, ::-1] * F(-1.0)
    prev_hits["point"][pick(0.05)] += F(0.06)                    # more than plane_eps along some normals
    shifted = hits.copy()
    shifted["point"][:, ::2] += np.array([0.5, 0.25, 0.0], dtype=F) * hits["normal"][:, ::2, ::-1]      # (mostly along the surface)
    cur = rng.random((W, H, 3), dtype=F)
    prev = (cam_prev, prev_hits) + made_up_history(3, W, H, 3)
    live = ~temporal_ref.dead_records(hits)
    counts = []
    for kw in (dict(), dict(match_color=True), dict(plane_eps=0.0), dict(normal_cos=-1.0, plane_eps=0.0)):
        want = both_ways(cur, hits, cam, prev, "identity", **kw)
        counts.append(int(want[4][live].sum()))
        assert 50 <= counts[-1] <= live.sum() - 500
    assert counts[1] > counts[0] > counts[2] > counts[3] > 0      # each test rejects pixels of its own
    want = both_ways(cur, shifted, cam, (cam_prev, shifted) + prev[2:], "identity, shifted points", plane_eps=0.0)
    assert not want[4][live].any()
    other = cameras.camera(EYE, LOOK + np.array([1e-4, 0.0, 0.0]))                                       # not the identity any more
    assert temporal_ref.accumulate(cur, shifted, other, (cam_prev, shifted) + prev[2:], plane_eps=0.0)[4][live].sum() > 100


def test_a_strip_equals_the_frames_columns():
    W, H, x0, x1 = 61, 37, 16, 48
    for name in ("truck", "equal"):
        cam_prev, cam, prev_hits, hits = pair_records(name, W, H)
        cur = np.random.default_rng(3).random((W, H, 3), dtype=F)
        prev = (cam_prev, prev_hits) + made_up_history(4, W, H, 3)
        frame = temporal_accumulate(cur, hits, cam, prev)
        part_cur, part_hits = np.ascontiguousarray(cur[x0:x1]), np.ascontiguousarray(hits[x0:x1])
        want = both_ways(part_cur, part_hits, cam, prev, f"{name} strip", x0=x0)
        assert_all_same(want, [a[x0:x1] for a in frame], f"{name}: the strip against the frame's columns")
        assert not want[4].all() and (name == "equal" or want[4].sum() >= 5)
    first = both_ways(part_cur, part_hits, cam, None, "first frame, strip", x0=x0, W=W)
    assert first[4].all()


def test_nan_and_infinity_in_the_previous_frame():
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
    plain = temporal_ref.accumulate(cur, hits, cam, (cam_prev, pair_records("truck", W, H)[2], value, moments, length))
    for kw in (dict(), dict(plane_eps=0.0, max_history=4, alpha=0.2)):
        want = both_ways(cur, hits, cam, (cam_prev, prev_hits, value, moments, length), "NaN and infinity", **kw)
        assert np.isnan(want[0]).sum() > 20 and np.isnan(want[1]).sum() > 20 and np.isfinite(want[2]).all()
        assert (want[3] >= 0).all() or np.isnan(want[3]).any()
    assert want[4].sum() > plain[4].sum()                        # a NaN normal or point skips the tap


def test_made_up_records_under_a_moved_camera():
    """random records on a rough plane y ~ 0 seen from y = -12, the previous camera a little aside: taps pass or fail by every
    clause at once, and neighbouring pixels reproject far apart"""
    W, H = 67, 70                                               # two tile rows and a part of a third, 17 tile columns
    hits, prev_hits = random_frame(11, W, H), random_frame(11, W, H)
    changed = np.random.default_rng(12).random((W, H)) < 0.3
    prev_hits[changed] = random_frame(13, W, H)[changed]
    centre = np.array([W * 0.125, 0.0, H * 0.125])
    cam = cameras.camera(centre + [0.0, -12.0, 0.0], centre, up=(0.0, 0.0, 1.0), screen=(1.5, 1.5))
    cam_prev = cameras.camera(centre + [0.4, -12.0, -0.3], centre + [0.2, 0.0, 0.1], up=(0.0, 0.0, 1.0), screen=(1.5, 1.5), roll=0.05)
    rng = np.random.default_rng(14)
    for channels, kw in ((3, dict(normal_cos=0.3, plane_eps=0.5)), (3, dict(normal_cos=0.0, plane_eps=0.0, match_color=True)),
                         (1, dict(normal_cos=-1.0, plane_eps=0.2, max_history=3, alpha=0.5, alpha_moments=1.0))):
        cur = rng.random((W, H, 3) if channels == 3 else (W, H), dtype=F)
        prev = (cam_prev, prev_hits) + made_up_history(15, W, H, channels)
        want = both_ways(cur, hits, cam, prev, "made-up records", **kw)
        live = ~temporal_ref.dead_records(hits)
        assert (~want[4]).sum() >= 300 and want[4][live].sum() >= 300, (kw, int((~want[4]).sum()), int(want[4][live].sum()))


def test_the_host_call_without_variance_and_flags():
    """rt_temporal_accumulate with out_variance and out_flags NULL and kernel_ms given: the three outputs it has left are the
    reference's word for word.  5 x 67: one whole 64-lane tile and 3 lanes of the next along z, and columns that fill neither a
    workgroup's four wavefronts nor a column group."""
    Wn, H = 5, 67
    hits, prev_hits = random_frame(21, Wn, H), random_frame(21, Wn, H)
    changed = np.random.default_rng(22).random((Wn, H)) < 0.3
    prev_hits[changed] = random_frame(23, Wn, H)[changed]
    centre = np.array([Wn * 0.125, 0.0, H * 0.125])
    cam = cameras.camera(centre + [0.0, -12.0, 0.0], centre, up=(0.0, 0.0, 1.0), screen=(1.5, 1.5))
    cam_prev = cameras.camera(centre + [0.4, -12.0, -0.3], centre + [0.2, 0.0, 0.1], up=(0.0, 0.0, 1.0), screen=(1.5, 1.5), roll=0.05)
    cur = np.random.default_rng(24).random((Wn, H, 3), dtype=F)
    value, moments, length = made_up_history(25, Wn, H, 3)
    kw = dict(normal_cos=0.3, plane_eps=0.5)
    want = temporal_ref.accumulate(cur, hits, cam, (cam_prev, prev_hits, value, moments, length), **kw)
    assert (~want[4]).sum() >= 20 and want[4].sum() >= 20           # pixels with a history and pixels without
    params = temporal_params(3, **kw)
    got = [np.empty((Wn, H, 3), dtype=F), np.empty((Wn, H, 2), dtype=F), np.empty((Wn, H), dtype=F)]
    ms = C.c_double(-1.0)
    capi.check(capi.load_library().rt_temporal_accumulate(
        0, C.byref(params), C.byref(cam_prev), C.byref(cam), Wn, H, 0, Wn, cur.ctypes.data, hits.ctypes.data, prev_hits.ctypes.data,
        value.ctypes.data, moments.ctypes.data, length.ctypes.data, *[a.ctypes.data for a in got], None, None, C.byref(ms)))
    assert_all_same(got, want[:3], "host call without variance and flags")
    assert ms.value > 0.0


# ---- 2. the history object and the accumulated render ------------------------------------------------------------------------------

def test_temporal_history_push_over_four_frames_equals_four_host_calls():
    W, H = 61, 37
    kw = dict(max_history=3, alpha=0.1)
    names = ("equal", "truck", "pan", "equal")
    rng = np.random.default_rng(7)
    history = TemporalHistory(W, H, 3, **kw)
    state = None
    cam_prev, _, hits, _ = pair_records("equal", W, H)
    cams = [cam_prev] + [pair_records(n, W, H)[1] for n in names[1:]]
    records = [hits] + [pair_records(n, W, H)[3] for n in names[1:]]
    for k, (cam, hits) in enumerate(zip(cams, records)):
        cur = rng.random((W, H, 3), dtype=F)
        value, moments, length, variance, flags = temporal_accumulate(cur, hits, cam, state, **kw)
        if k == 2:                                               # a frame pushed as two strips
            parts = [history.push(cur[:23], hits[:23], cam, 0, 23), history.push(cur[23:], hits[23:], cam, 23)]
            got = [np.concatenate([a, b]) for a, b in zip(*parts)]
            with pytest.raises(ValueError):
                history.push(cur[23:], hits[23:], cam, 23)
        else:
            got = history.push(cur, hits, cam)
        assert_all_same(got, (value, variance, flags), f"push {k}")
        assert flags.all() == (k == 0) and (k == 0 or (~flags).sum() > 1000)
        state = (cam, hits, value, moments, length)
        kept = history.state()
        assert_all_same(kept[2:], state[2:], f"state after push {k}")
        assert kept[1].tobytes() == hits.tobytes() and history.frames == k + 1
    assert length.max() == 3
    history.reset()
    assert history.state() is None
    value, variance, flags = history.push(cur, hits, cam)
    assert flags.all() and np.array_equal(value.view(np.uint32), cur.view(np.uint32))
    one = TemporalHistory(W, H, 1)
    plane = np.ascontiguousarray(cur[..., 0])
    assert_all_same(one.push(plane, hits, cam), [a for k, a in enumerate(temporal_accumulate(plane, hits, cam)) if k in (0, 3, 4)], "one channel")


@pytest.mark.parametrize("term", ["indirect", "ao", "direct"])
def test_render_accumulated_is_the_composition_of_the_public_calls(term):
    W, H, depth = 45, 38, 3
    r = Renderer(HostScene.builtin())
    plain = cameras.camera(EYE, LOOK)
    d = np.array([0.1, -0.1, 0.0])
    cams = [plain, cameras.camera(EYE, LOOK), cameras.camera(EYE + d, LOOK + d), cameras.camera(EYE + 2 * d, LOOK + 2 * d)]
    kw = dict(max_history=3, alpha=0.05, plane_eps=0.02)
    term_kw = dict(indirect=dict(gather_depth=1, gain=1.25), ao=dict(radius=2.0), direct=dict())[term]
    state = None
    own = r._cam
    for k, cam in enumerate(cams):
        r._cam = C.pointer(cam)
        if term == "direct":
            r.set_shadow_seed(k)
        rgb, hits = r.render_gbuffer(W, H, depth)
        cur = rgb if term == "direct" else r.indirect_diffuse(hits, 1, seed=k, base=rgb, **term_kw) if term == "indirect" \
            else r.ambient_occlusion(hits, 1, seed=k, **term_kw)
        value, moments, length, variance, flags = temporal_accumulate(cur, hits, cam, state, **kw)
        state = (cam, hits, value, moments, length)
    r._cam = own
    got = r.render_accumulated(cams, W, H, depth, term=term, samples=1, **kw, **term_kw)
    assert r._cam is own
    assert_all_same(got, (value, variance, flags), f"render_accumulated {term}")
    live = ~temporal_ref.dead_records(hits)
    assert (~flags).sum() > 1000 and flags[live].any() and length.max() == 3
    if term != "direct":                                        # (the built-in scene's lights are points: its direct frames are equal)
        assert (variance > 0).sum() > 500
    with pytest.raises(ValueError):
        r.render_accumulated(cams, W, H, depth, term="glossy")
    r.close()


# ---- 3. the device entry point's refusals -------------------------------------------------------------------------------------------

def test_device_entry_refuses_and_the_next_call_is_unharmed():
    import torch
    W, H = 20, 70
    hits = random_frame(8, W, H)
    cur = np.random.default_rng(9).random((W, H, 3), dtype=F)
    cam = cameras.camera(EYE, LOOK)
    prev = (cameras.camera(EYE, LOOK), hits) + made_up_history(10, W, H, 3)
    d_hits = poisoned._on_device(np.concatenate([np.zeros(4, np.int32), hits.reshape(-1).view(np.int32)]))
    d = [poisoned._on_device(a.view(np.int32)) for a in (cur,) + prev[2:]]
    g = [Guarded(W * H * k) for k in (3, 2, 1)]
    lib = capi.load_library()
    params = temporal_params(3)
    call = lambda device, hits_ptr, prev_hits_ptr, out_value: lib.rt_temporal_accumulate_device(
        device, C.byref(params), C.byref(prev[0]), C.byref(cam), W, H, 0, W, d[0].data_ptr(), hits_ptr, prev_hits_ptr, d[1].data_ptr(),
        d[2].data_ptr(), d[3].data_ptr(), out_value, g[1].ptr, g[2].ptr, None, None, poisoned._stream())
    good = d_hits.data_ptr() + 16
    for hits_ptr, prev_ptr, out_value, device, word in ((good - 8, good, g[0].ptr, 0, "16-byte"), (good, good + 4, g[0].ptr, 0, "16-byte"),
                                                        (good, good, g[0].ptr + 2, 0, "4-byte"), (good, good, d[1].data_ptr(), 0, "overlap"),
                                                        (good, good, good + 48, 0, "overlap"), (good, good, g[0].ptr, 99, "device index")):
        rc = call(device, hits_ptr, prev_ptr, out_value)
        assert rc == capi.RT_ERR_INVALID and word in lib.rt_last_error().decode(), word
    torch.cuda.synchronize()
    for buf in g:
        assert buf.sentinels_left() == buf.n and buf.guards_untouched()          # nothing was launched
    both_ways(cur, hits, cam, prev, "after the refusals", normal_cos=0.0)
