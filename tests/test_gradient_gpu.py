"""Temporal-gradient weights for an accumulated history (include/rt_gradient.h) on the GPU against its definition:
rt_gradient_reweight and rt_gradient_reweight_device against gradient_ref bit for bit -- value, moments, length, variance, lambda
and flags -- on gradient_edges.py's inputs at the edges of the rule and on random made-up frames of one lane, one tile, one past
it in both directions and several tiles with ragged cells, at every scale and radius, with one and three channels, with then_hits
given and NULL, in place against out of place, with every combination of the optional outputs, a strip against the frame's
columns, the device entry point captured in a graph (one kernel node) and replayed once, and the composed calls.  The device
entry point writes into sentinel-filled guarded outputs.  Bar: BIT-EXACT."""
import ctypes as C
import itertools

import numpy as np
import pytest

import gradient_edges
import gradient_ref
import motion_scenes
import poisoned
from gradient_edges import made_up_inputs
from large_extents import SENTINEL_BYTE, Guarded
from test_upsample_gpu import assert_same
from tilecoderaytracer_amd import (Renderer, TemporalHistory, capi, gradient_reweight, history_clamp, motion_accumulate,
                                   object_motions, render_animated)
from tilecoderaytracer_amd.renderer import gradient_params

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = gradient_ref.NAMES
SHAPES = [(1, 1), (4, 64), (5, 65), (13, 130), (61, 37)]
# every scale x every radius, with both settings of match_color and every value of the other parameters
COMBOS = [dict(scale=s, radius=r, match_color=bool((s + r) % 2), normal_cos=(0.9, -1.0, 0.3)[r], gain=(2.0, 1.0, 8.0)[r],
               lambda_min=(0.0, 0.1, 0.0)[r], den_floor=(1e-6, 0.0, 0.5)[r]) for s in (2, 3, 5, 8) for r in (0, 1, 2)]


def assert_all_same(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        if g is not None:
            assert_same(g, w, f"{what}: {name}")


def device_reweight(inputs, want, in_place=False, optional=(True, True, True), **kw):
    """rt_gradient_reweight_device into sentinel-filled outputs -- in place: value, moments and length into (copies of) the
    inputs themselves -> the six outputs (None for an optional one that is not asked for); every word of the outputs written,
    none beside, and no input changed but those written in place"""
    import torch
    cur, hits = inputs[0], inputs[1]
    channels = 3 if cur.ndim == 3 else 1
    Wn, H = hits.shape
    params = gradient_params(channels, **kw)
    what = f"rt_gradient_reweight_device {Wn}x{H} channels {channels} in place {in_place} optional {optional} {kw}"
    poisoned.assert_reference_has_no_sentinel(list(want[:5]), what)
    poisoned.assert_reference_has_no_sentinel(want[5], what)
    d_in = [None if a is None else poisoned._on_device(np.ascontiguousarray(a).reshape(-1).view(np.int32)) for a in inputs]
    before = [None if t is None else t.clone() for t in d_in]
    n = Wn * H
    specs = [(n * channels, channels, False), (n * 2, 2, False), (n, 1, False), (n, 1, False), (n, 1, False), (n, 1, True)]
    bufs = [Guarded(words + poisoned.SLACK_CELLS * per, as_bytes=b) for words, per, b in specs]
    asked = [not in_place] * 3 + list(optional)
    out_ptrs = [t.data_ptr() for t in d_in[2:5]] if in_place else [g.ptr for g in bufs[:3]]
    out_ptrs += [g.ptr if a else None for g, a in zip(bufs[3:], optional)]
    capi.check(capi.load_library().rt_gradient_reweight_device(0, C.byref(params), Wn, H, *[None if t is None else t.data_ptr() for t in d_in],
                                                               *out_ptrs, poisoned._stream()))
    torch.cuda.synchronize()
    for k, (t, b) in enumerate(zip(d_in, before)):
        assert t is None or (in_place and 2 <= k < 5) or torch.equal(t, b), f"{what}: input {k} was written"
    out = []
    for k, (g, (words, per, as_bytes)) in enumerate(zip(bufs, specs)):
        if not asked[k]:
            assert g.sentinels_left() == g.n and g.guards_untouched(), f"{what}: {NAMES[k]} was written"
            out.append(d_in[k + 2].cpu().numpy() if k < 3 else None)
            continue
        host = g.all.cpu().numpy()
        body = poisoned.check_output(host[:g.guard], host[g.guard:g.guard + g.n], host[g.guard + g.n:], words,
                                     poisoned.layout(per, H), f"{what}, {NAMES[k]}", SENTINEL_BYTE if as_bytes else poisoned.SENTINEL)
        out.append(body.copy())
    for g in bufs:
        g.free()
    shape = (Wn, H)
    view = lambda a, s: None if a is None else a.view(F).reshape(s)
    return (view(out[0], shape + ((3,) if channels == 3 else ())), view(out[1], shape + (2,)), view(out[2], shape),
            view(out[3], shape), view(out[4], shape), None if out[5] is None else out[5].reshape(shape))


def both_ways(inputs, what, device=True, in_place=False, **kw):
    """the host call and (device) the device entry point against the reference -> the reference's outputs"""
    want = gradient_ref.reweight(*inputs, **kw)
    assert_all_same(gradient_reweight(*inputs, **kw), want, f"{what} {kw}")
    if device:
        assert_all_same(device_reweight(inputs, want, in_place=in_place, **kw), want, f"{what} {kw}, device")
    return want


# ---- 1. the edge inputs --------------------------------------------------------------------------------------------------------------

def edge_case_both_ways(name, what=""):
    """a case of gradient_edges.CASES with one and three channels, out of place and in place -> the references' outputs"""
    wants = []
    for channels in (1, 3):
        case = gradient_edges.CASES[name](channels)
        for in_place in (False, True):
            wants.append(both_ways(case[:9], f"{what}{name} channels {channels}", device=True, in_place=in_place, **case[9]))
    return wants


@pytest.mark.parametrize("name", list(gradient_edges.CASES))
def test_edge_inputs_are_the_reference_bit_for_bit(name):
    """gradient_edges.py's inputs at the edges of the header's rule (test_gradient_cpu.py holds that each tells a rule one line
    off the header's from the header's): the host call and the guarded device entry, in place and out of place, with one and
    three channels"""
    edge_case_both_ways(name)


# ---- 2. random made-up frames: every shape, scale, radius, channel count, then_hits given and NULL ------------------------------------

@pytest.mark.parametrize("Wn, H", SHAPES, ids=lambda v: str(v))
def test_shapes_scales_and_radii_are_the_reference_bit_for_bit(Wn, H):
    """one lane, exactly one tile, one past it in both directions, several tiles with ragged cells; every second combination
    goes through the guarded device entry point too, in place and out of place in turn"""
    seen = np.zeros(4, dtype=np.int64)
    for k, kw in enumerate(COMBOS):
        for channels, then in ((1, (k + Wn) % 2 == 0), (3, (k + Wn) % 2 == 1)):
            inputs = made_up_inputs(Wn * 1000 + H + k, Wn, H, channels, kw["scale"], special=k % 3 != 0)
            if not then:
                inputs[8] = None
            want = both_ways(inputs, f"{Wn}x{H} channels {channels} then {then}", device=(k + channels) % 4 < 2, in_place=k % 4 < 2, **kw)
            seen += np.bincount(want[5].reshape(-1), minlength=4)[:4]
    assert Wn * H < 300 or (seen >= 20).all(), seen              # untouched, re-blended, left for no cell and restarted


# ---- 3. in place, and the optional outputs -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels, then", [(3, True), (1, True), (3, False), (1, False)])
def test_in_place_is_out_of_place_and_the_optional_outputs_may_be_null(channels, then):
    """every kernel of the library's form (channels x then_hits given or NULL) with every combination of the three optional
    outputs, in place and out of place"""
    Wn, H = 13, 130
    kw = COMBOS[4]                                               # scale 3, radius 1
    inputs = made_up_inputs(50 + channels, Wn, H, channels, kw["scale"])
    if not then:
        inputs[8] = None
    want = gradient_ref.reweight(*inputs, **kw)
    assert (want[5] == 1).sum() >= 100
    for in_place in (False, True):
        for optional in itertools.product((False, True), repeat=3):
            got = device_reweight(inputs, want, in_place=in_place, optional=optional, **kw)
            assert_all_same(got, want, f"in place {in_place}, optional {optional}")
    # the host call in place, without its optional outputs, with the kernel's time
    value, moments, length = (np.array(a, copy=True) for a in inputs[2:5])
    ms = C.c_double(-1.0)
    params = gradient_params(channels, **kw)
    ptr = lambda a: None if a is None else a.ctypes.data
    capi.check(capi.load_library().rt_gradient_reweight(0, C.byref(params), Wn, H, ptr(inputs[0]), ptr(inputs[1]), ptr(value), ptr(moments),
                                                        ptr(length), *[ptr(a) for a in inputs[5:]], ptr(value), ptr(moments), ptr(length),
                                                        None, None, None, C.byref(ms)))
    assert_all_same((value, moments, length), want, "the host call in place")
    assert ms.value > 0.0


# ---- 4. a strip -----------------------------------------------------------------------------------------------------------------------------

def test_a_strip_equals_the_frames_columns_but_those_whose_window_reaches_beyond_it():
    Wn, H = 61, 37
    for channels, kw in ((3, COMBOS[1]), (1, COMBOS[3]), (3, COMBOS[8])):           # scale 2 r 1, scale 3 r 0, scale 5 r 2
        s, r = kw["scale"], kw["radius"]
        inputs = made_up_inputs(90 + channels + s, Wn, H, channels, s)
        full = gradient_reweight(*inputs, **kw)
        x0, x1 = 2 * s, Wn - 7
        i0, i1 = x0 // s, -(-x1 // s)
        part = [np.ascontiguousarray(a[x0:x1]) for a in inputs[:5]] + [np.ascontiguousarray(a[i0:i1]) for a in inputs[5:]]
        strip = both_ways(part, "strip", device=False, **kw)
        cols = [x for x in range(x0, x1) if x // s - r >= i0 and x // s + r + 1 < i1]
        assert len(cols) >= 10
        assert_all_same([o[[x - x0 for x in cols]] for o in strip], [f[cols] for f in full], f"strip {kw}")


# ---- 5. captured in a graph ---------------------------------------------------------------------------------------------------------------

def test_device_entry_captured_in_a_graph_is_one_kernel_node_and_replays_to_the_reference():
    """the device call only enqueues, so the capture allocates nothing; the replayed words are the eager ones and the
    definition's, and the captured graph is a single kernel node"""
    import torch
    Wn, H = 61, 37
    kw = COMBOS[1]
    inputs = made_up_inputs(5, Wn, H, 3, kw["scale"], special=False)
    want = gradient_ref.reweight(*inputs, **kw)
    assert (want[5] == 1).sum() >= 100
    d_in = [poisoned._on_device(np.ascontiguousarray(a).reshape(-1).view(np.int32)) for a in inputs]
    n = Wn * H
    new = lambda: [torch.zeros((n * w,), dtype=torch.int32, device="cuda") for w in (3, 2, 1, 1, 1)] + \
        [torch.zeros((n,), dtype=torch.uint8, device="cuda")]
    eager, replayed = new(), new()
    params, lib = gradient_params(3, **kw), capi.load_library()

    def enqueue(outs, stream_ptr):
        capi.check(lib.rt_gradient_reweight_device(0, C.byref(params), Wn, H, *[t.data_ptr() for t in d_in], *[t.data_ptr() for t in outs],
                                                   stream_ptr))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    enqueue(eager, side.cuda_stream)
    side.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)                # (the captured graph stays, for its nodes to be listed)
    with torch.cuda.graph(graph, stream=side):
        enqueue(replayed, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all(int(b.abs().max()) == 0 for b in replayed[:5])                    # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    shapes = ((Wn, H, 3), (Wn, H, 2), (Wn, H), (Wn, H), (Wn, H))
    for outs, what in ((eager, "eager"), (replayed, "replayed")):
        got = [t.cpu().numpy().view(F).reshape(s) for t, s in zip(outs[:5], shapes)] + [outs[5].cpu().numpy().reshape(Wn, H)]
        assert_all_same(got, want, f"one stream, {what}")
    # the graph's nodes: torch's own graph object, whose handle the runtime lists
    raw = graph.raw_cuda_graph()
    assert raw
    if raw:
        hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
        hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
        hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        count = C.c_size_t(0)
        assert hip.hipGraphGetNodes(C.c_void_p(raw), None, C.byref(count)) == 0 and count.value == 1, count.value
        node, kind = (C.c_void_p * 1)(), C.c_int(-1)
        assert hip.hipGraphGetNodes(C.c_void_p(raw), node, C.byref(count)) == 0
        assert hip.hipGraphNodeGetType(node[0], C.byref(kind)) == 0 and kind.value == 0         # hipGraphNodeTypeKernel
    del graph
    # refusals launch nothing
    g = Guarded(n * 3)
    ptrs = [t.data_ptr() for t in d_in]
    tail = [eager[1].data_ptr(), eager[2].data_ptr(), None, None, None, None]
    for bad, out_value, word in (((ptrs[0], ptrs[1] + 8) + tuple(ptrs[2:]), g.ptr, "16-byte"),
                                 ((ptrs[0] + 2,) + tuple(ptrs[1:]), g.ptr, "4-byte"),
                                 (tuple(ptrs), ptrs[0], "d_cur or d_hits"), (tuple(ptrs), ptrs[5], "cell buffer"),
                                 (tuple(ptrs), ptrs[2] + 4, "partially")):
        rc = lib.rt_gradient_reweight_device(0, C.byref(params), Wn, H, *bad, out_value, *tail)
        assert rc == capi.RT_ERR_INVALID and word in lib.rt_last_error().decode(), (word, lib.rt_last_error().decode())
    rc = lib.rt_gradient_reweight_device(99, C.byref(params), Wn, H, *ptrs, g.ptr, *tail)
    assert rc == capi.RT_ERR_INVALID and "device index" in lib.rt_last_error().decode()
    torch.cuda.synchronize()
    assert g.sentinels_left() == g.n and g.guards_untouched()


# ---- 6. the composed calls ---------------------------------------------------------------------------------------------------------------

SEQUENCE = [motion_scenes.REST, motion_scenes.REST, motion_scenes.SHIFTED, dict(motion_scenes.SHIFTED, angle=0.3, axis=(0.3, -0.2, 1.0))]
CAMERAS = ["equal", "equal", "equal", "truck"]                   # the current camera of camera_pair()
W48, H32, S = 48, 32, 2


def under(r, cam, call):
    """call() with the renderer's camera replaced by cam"""
    own, r._cam = r._cam, C.pointer(cam)
    try:
        return call()
    finally:
        r._cam = own


def composed(term, gkw, ckw=None, kw=dict(max_history=8, match_color=True), term_kw=None):
    """the sequence through the public host calls: per frame the G-buffer and the term, motion_accumulate(), from frame 1 on the
    two cell frames and gradient_reweight(), then (ckw) history_clamp() -> (renderers, cameras, tables, per frame: (cur, hits,
    the cells or None, accumulated, re-weighted or None, the frame's final (value, moments, length, variance)))"""
    hosts = [motion_scenes.host(p) for p in SEQUENCE]
    tables = [None] + [object_motions(a.desc, b.desc) for a, b in zip(hosts, hosts[1:])]
    renderers = [Renderer(h) for h in hosts]
    cams = [motion_scenes.camera_pair(n)[1] for n in CAMERAS]
    term_kw = term_kw or {}

    def shade(r, cam, k, W, H):
        if term == "direct":
            r.set_shadow_seed(k)
        rgb, hits = under(r, cam, lambda: r.render_gbuffer(W, H, 3))
        if term == "ao":
            return r.ambient_occlusion(hits, 1, seed=k, **term_kw), hits
        if term == "indirect":
            return r.indirect_diffuse(hits, 1, seed=k, base=rgb, **term_kw), hits
        return rgb, hits

    state, frames = None, []
    for k, (r, cam, table) in enumerate(zip(renderers, cams, tables)):
        cells = None
        if k >= 1:
            now_lo, lo_hits = shade(r, cam, k, W48 // S, H32 // S)
            then_lo, then_hits = shade(renderers[k - 1], cam, k, W48 // S, H32 // S)
            cells = (now_lo, then_lo, lo_hits, then_hits)
        cur, hits = shade(r, cam, k, W48, H32)
        acc = motion_accumulate(cur, hits, cam, state, table, **kw)
        final, weighed = acc[:4], None
        if cells is not None:
            weighed = gradient_reweight(cur, hits, acc[0], acc[1], acc[2], *cells, **gkw)
            final = weighed[:4]
        if ckw is not None:
            final = history_clamp(cur, hits, final[0], final[1], final[2], **ckw)[:4]
        state = (cam, hits) + tuple(final[:3])
        frames.append((cur, hits, cells, acc, weighed, final))
    return renderers, cams, tables, frames


def test_temporal_history_push_with_a_gradient_equals_the_public_calls():
    gkw = dict(scale=S, radius=1, gain=2.0)
    kw = dict(max_history=8, match_color=True)
    renderers, cams, tables, frames = composed("direct", gkw)
    history = TemporalHistory(W48, H32, 3, **kw)
    assert history.gradient_lambda is None and history.gradient_flags is None
    touched = 0
    for k, (cam, table, (cur, hits, cells, acc, weighed, final)) in enumerate(zip(cams, tables, frames)):
        gradient = None if cells is None else dict(gkw, now_lo=cells[0], then_lo=cells[1], lo_hits=cells[2], then_hits=cells[3])
        got = history.push(cur, hits, cam, motions=table, gradient=gradient)
        assert_same(got[0], final[0], f"push {k}: value")
        assert_same(got[1], final[3], f"push {k}: variance")
        assert_same(got[2], acc[4], f"push {k}: flags")
        kept = history.state()
        for a, b, name in zip(kept[2:], final[:3], NAMES):
            assert_same(a, b, f"state after push {k}: {name}")
        if weighed is not None:
            assert_same(history.gradient_lambda.cpu().numpy().reshape(W48, H32), weighed[4], f"push {k}: lambda")
            assert_same(history.gradient_flags.cpu().numpy().reshape(W48, H32), weighed[5], f"push {k}: gradient flags")
            touched += int((weighed[5] & 1).sum())
    assert touched >= 50
    with pytest.raises(capi.RtError):
        history.push(cur, hits, cam, gradient=dict(gradient, scale=9))
    with pytest.raises(ValueError):
        history.push(cur, hits, cam, gradient=dict(gradient, now_lo=cells[0][:5]))
    with pytest.raises(TypeError):
        history.push(cur, hits, cam, gradient=dict(gradient, channels=3))
    for r in renderers:
        r.close()


@pytest.mark.parametrize("term", ["direct", "ao", "indirect"])
def test_render_animated_with_a_gradient_is_the_composition_of_the_public_calls(term):
    gkw = dict(scale=S, radius=1, gain=2.0)
    ckw = dict(box=0, radius=1, min_taps=2, clip_history=2) if term == "direct" else None
    kw = dict(max_history=8, match_color=True)
    term_kw = dict(ao=dict(radius=2.0), direct=dict(), indirect=dict())[term]
    renderers, cams, tables, frames = composed(term, gkw, ckw, kw, term_kw)
    final, acc = frames[-1][5], frames[-1][3]
    sequence = list(zip(renderers, cams, tables))
    got = render_animated(sequence, W48, H32, 3, term=term, samples=1, clamp=ckw, gradient=gkw, **kw, **term_kw)
    assert_same(got[0], final[0], f"render_animated {term} with a gradient: value")
    assert_same(got[1], final[3], f"render_animated {term} with a gradient: variance")
    assert_same(got[2], acc[4], f"render_animated {term} with a gradient: flags")
    assert sum(int((f[4][5] & 1).sum()) for f in frames[1:]) >= 20
    # gradient=None is the call as it was, and differs
    plain = render_animated(sequence, W48, H32, 3, term=term, samples=1, clamp=ckw, **kw, **term_kw)
    assert not np.array_equal(plain[0], got[0])
    with pytest.raises(ValueError):
        render_animated(sequence, 45, H32, 3, term=term, samples=1, gradient=gkw, **kw, **term_kw)
    with pytest.raises(capi.RtError):
        render_animated(sequence, W48, H32, 3, term=term, samples=1, gradient=dict(gkw, radius=3), **kw, **term_kw)
    for r in renderers:
        r.close()


# ---- 7. the kernel form that was not kept ------------------------------------------------------------------------------------------------------

def test_both_kernel_forms_where_the_library_has_them():
    """A build with -DRT_GRADIENT_VARIANTS=1, named in TCRT_LIBRARY, has both forms of the window's reads and the switch between
    them: each is held to the reference, on made-up frames of every shape and on every edge case of gradient_edges.py.  The
    library proper has one form and no switch."""
    lib = capi.load_library()
    if not hasattr(lib, "rt_internal_gradient_variant"):
        return
    lib.rt_internal_gradient_variant.argtypes, lib.rt_internal_gradient_variant.restype = [C.c_int], C.c_int
    kept = lib.rt_internal_gradient_variant(0)
    try:
        for form in (0, 1):
            lib.rt_internal_gradient_variant(form)
            for Wn, H in SHAPES:
                for k, kw in enumerate(COMBOS):
                    inputs = made_up_inputs(Wn + H + k, Wn, H, 3 if k % 2 else 1, kw["scale"])
                    if k % 3 == 0:
                        inputs[8] = None
                    both_ways(inputs, f"form {form} {Wn}x{H}", in_place=k % 2 == 0, **kw)
            for name in gradient_edges.CASES:
                edge_case_both_ways(name, f"form {form} ")
    finally:
        lib.rt_internal_gradient_variant(kept)
