"""rt_indirect_paths over the live paths alone (include/rt_paths_compact.h) on the GPU.  The header adds no definition: every
output word is compared with rt_indirect_paths' of the same handle and, where the CPU oracle covers the scene, with paths_ref;
alive[] with the reference's counts; rays, traces, queries and syncs with paths_compact_ref.paths_compact_expect, the header's
rule over the reference's per-path alive masks.  The conditions these comparisons rest on -- alive counts that fall strictly and
stay above zero, lists of the sizes named, a chunk that ends at once -- are asserted on the reference by
tests/test_paths_compact_cpu.py.  Bar: BIT-EXACT."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_frames
import ao_ref
import indirect_ref
import paths_compact_ref as ref
import paths_ref
import poisoned
from test_paths_gpu import BUILTIN, FRAME, H37, STRIPS, W61, alive, assert_same, frame_id, own_walk, records
from tilecoderaytracer_amd import HostScene, Renderer, RtError, capi, indirect_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
COUNTS = ("records", "rays", "chunks", "traces", "queries", "syncs", "alive")


def builtin_kd():
    import oracle_lib
    return indirect_ref.object_diffuse(oracle_lib.OracleScene.builtin())


def check_info(r, want, B, emitters, what):
    """the compact info against paths_compact_expect's dict; the stage times"""
    info = r.paths_compact_info()
    got = ref.info_of(info, B)
    assert got == {k: want[k] for k in COUNTS}, (what, got, want)
    assert [int(v) for v in info.alive[B:]] == [0] * (8 - B), what
    assert info.raygen_ms > 0 and info.trace_ms > 0 and info.step_ms > 0 and info.resolve_ms > 0, what
    assert (info.query_ms == 0) == (B == 1 and bool(emitters)) and info.query_ms >= 0, (what, info.query_ms)
    return info


def check_oracle_frame(frame, B, emitters, with_base):
    key, W, H, depth, n, seed, gather_depth = frame
    what = f"{key} {W}x{H} n{n} B{B} emitters {emitters} base {with_base}"
    rgb = indirect_ref.oracle_gather(*frame)[0]
    want = paths_ref.oracle_term(frame, B, emitters, with_base)
    r = Renderer(adaptive_frames.host_scene(key))
    kw = dict(bounces=B, samples=n, gather_depth=gather_depth, seed=seed, emitters=emitters, base=rgb if with_base else None)
    got = r.indirect_paths(records(frame), compact=True, **kw)
    assert_same(got, want, what)
    walk = paths_ref.oracle_walk(frame)
    info = check_info(r, ref.paths_compact_expect(walk, 0, B, emitters), B, emitters, what)
    assert info.rays < W * H * n * n * B                                    # (some path ended: fewer rays than the in-place call)
    assert_same(got, r.indirect_paths(records(frame), **kw), what + ": rt_indirect_paths of the same handle")
    assert alive(r.paths_info(), B) == (walk.counts(B), [0] * (8 - B))


# ---- 1. every word against the CPU oracle and against rt_indirect_paths -------------------------------------------------------------

@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("emitters", [False, True])
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("frame", indirect_ref.FRAMES, ids=frame_id)
def test_against_the_oracle(frame, B, emitters, with_base):
    check_oracle_frame(frame, B, emitters, with_base)


@pytest.mark.parametrize("B", [4, 8])
@pytest.mark.parametrize("key", ["builtin", "random3"])
def test_long_paths_against_the_oracle(key, B):
    check_oracle_frame(FRAME[key], B, False, True)


@pytest.mark.parametrize("emitters", [False, True])
def test_the_emitter_frame_at_three_bounces(emitters):
    check_oracle_frame(indirect_ref.EMITTER_FRAME, 3, emitters, False)


# ---- 2. one bounce -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frame", indirect_ref.FRAMES, ids=frame_id)
def test_one_bounce_is_rt_indirect_diffuse_device_word_for_word(frame):
    import torch
    key, W, H, depth, n, seed, gather_depth = frame
    r = Renderer(adaptive_frames.host_scene(key))
    N = W * H
    d_hits = poisoned._on_device(records(frame).view(np.int32))
    d_base = poisoned._on_device(np.array(indirect_ref.oracle_gather(*frame)[0]).view(np.int32))
    for emitters in (False, True):
        for base in (0, d_base.data_ptr()):
            kw = dict(samples=n, gather_depth=gather_depth, seed=seed, emitters=emitters, gain=0.75)
            one = torch.full((N * 3,), poisoned.SENTINEL, dtype=torch.int32, device="cuda")
            two = torch.full((N * 3,), poisoned.SENTINEL, dtype=torch.int32, device="cuda")
            r.indirect_diffuse_device(N, d_hits.data_ptr(), base, one.data_ptr(), poisoned._stream(), **kw)
            r.indirect_paths_device(N, d_hits.data_ptr(), base, two.data_ptr(), poisoned._stream(), bounces=1, compact=True, **kw)
            torch.cuda.synchronize()
            assert torch.equal(one, two), (key, emitters, bool(base))
            info = r.paths_compact_info()
            assert (info.records, info.rays, info.chunks, info.traces, info.syncs) == (N, N * n * n, 1, 1, 0)
            assert info.traces == info.chunks and info.queries == (0 if emitters else 1) and (info.query_ms > 0) == (not emitters)
            assert alive(info, 1) == (paths_ref.oracle_walk(frame).counts(1), [0] * 7)
    assert_same(one.cpu().numpy().view(F).reshape(W, H, 3), indirect_ref.oracle_term(frame, True, True, 0.75), f"{key}: one bounce")


# ---- 3. lists whose sizes are at the edges of a wavefront and of a workgroup ----------------------------------------------------------

@pytest.fixture(scope="module")
def builtin_handle():
    r = Renderer(HostScene.builtin())
    kd = builtin_kd()
    walk_of = lambda hits: own_walk(r, hits, kd, ref.LIST_KW["n"], ref.LIST_KW["gather_depth"], ref.LIST_KW["seed"])   # noqa: E731
    return r, walk_of, ref.going_on(walk_of)


@pytest.mark.parametrize("c", ref.LIST_SIZES)
def test_a_list_of_exactly_c_entries_at_bounce_one(c, builtin_handle):
    r, walk_of, on = builtin_handle
    hits = ref.list_of_size(c, on)
    walk = walk_of(hits)
    base = np.random.RandomState(c).uniform(0, 1, (len(hits), 3)).astype(F)
    kw = dict(bounces=3, samples=1, gather_depth=ref.LIST_KW["gather_depth"], seed=ref.LIST_KW["seed"])
    for emitters in (False, True):
        got = r.indirect_paths(hits, emitters=emitters, base=base, compact=True, **kw)
        assert_same(got, walk.term(3, emitters, base), f"a list of {c}, emitters {emitters}")
        info = check_info(r, ref.paths_compact_expect(walk, 0, 3, emitters), 3, emitters, f"a list of {c}")
        assert info.alive[1] == c and info.alive[0] > c + 100
        assert_same(got, r.indirect_paths(hits, emitters=emitters, base=base, **kw), f"a list of {c}: rt_indirect_paths")


# ---- 4. every path ends at its first ray ------------------------------------------------------------------------------------------------

def test_paths_that_all_end_at_their_first_ray():
    hits = ref.sky_records(300)
    r = Renderer(HostScene.builtin())
    one = r.indirect_paths(hits, 1, 3, 1, seed=2)
    assert (r.intersect_rays(indirect_rays(hits, 3, seed=2).reshape(-1, 6))["object"] < 0).all()
    for emitters in (False, True):
        three = r.indirect_paths(hits, 3, 3, 1, seed=2, emitters=emitters, compact=True)
        assert_same(three, one, f"all paths end early, emitters {emitters}")
        info = r.paths_compact_info()
        assert alive(info, 3) == ([2700, 0, 0], [0] * 5)
        assert (info.traces, info.queries, info.syncs, info.rays, info.chunks) == (1, 1, 1, 2700, 1)
    assert (one > 0).all()                                                   # the sky's colour, weighted


# ---- 5. chunks that end at different bounces; scratch reused between calls ---------------------------------------------------------------

def test_chunks_that_end_at_different_bounces_and_scratch_reuse():
    hits = ref.two_chunk_batch()
    r = Renderer(HostScene.builtin())
    kw = dict(bounces=4, samples=ref.SKY_KW["n"], gather_depth=ref.SKY_KW["gather_depth"], seed=ref.SKY_KW["seed"])
    walk = own_walk(r, hits, builtin_kd(), kw["samples"], kw["gather_depth"], kw["seed"])
    want = r.indirect_paths(hits, **kw)
    assert alive(r.paths_info(), 4) == (walk.counts(4), [0] * 4)
    expect = ref.paths_compact_expect(walk, 300, 4, False)
    assert expect["runs"] == [1, 4]                                          # one chunk with one bounce run, one with four
    for chunk in (300, 1, 1013, 0):                                          # the same handle, in turn
        got = r.indirect_paths(hits, chunk_records=chunk, compact=True, **kw)
        assert_same(got, want, f"two chunks, chunk_records {chunk}")
        check_info(r, ref.paths_compact_expect(walk, chunk, 4, False), 4, False, f"chunk_records {chunk}")
    for emitters, n, count in ((True, 2, 1000), (False, 4, 77)):             # other batch sizes on the handle's scratch
        other = ref.builtin_records()[:count]
        kw2 = dict(bounces=3, samples=n, gather_depth=1, seed=9, emitters=emitters)
        assert_same(r.indirect_paths(other, compact=True, **kw2), r.indirect_paths(other, **kw2), f"then {count} records, n{n}")
        assert alive(r.paths_compact_info(), 3) == alive(r.paths_info(), 3)
    assert_same(r.indirect_paths(hits, chunk_records=300, compact=True, **kw), want, "and the first batch again")


# ---- 6. more live entries than one group of the scan -----------------------------------------------------------------------------------

def test_more_live_entries_than_one_scan_group():
    import torch
    W, H, n, B = 128, 80, 7, 3
    r = Renderer(HostScene.builtin())
    _, hits = r.render_gbuffer(W, H, 4)
    N = W * H
    assert N * n * n == 501760
    d_hits = poisoned._on_device(np.ascontiguousarray(hits).view(np.int32))
    one = torch.full((N * 3,), poisoned.SENTINEL, dtype=torch.int32, device="cuda")
    two = torch.full((N * 3,), poisoned.SENTINEL, dtype=torch.int32, device="cuda")
    kw = dict(bounces=B, samples=n, gather_depth=1, seed=3, emitters=False)
    r.indirect_paths_device(N, d_hits.data_ptr(), 0, one.data_ptr(), poisoned._stream(), **kw)
    r.indirect_paths_device(N, d_hits.data_ptr(), 0, two.data_ptr(), poisoned._stream(), compact=True, **kw)
    torch.cuda.synchronize()
    plain, info = r.paths_info(), r.paths_compact_info()
    assert plain.alive[1] > ref.SCAN_GROUP, f"alive[1] = {plain.alive[1]}: the list does not span two groups of the scan"
    assert plain.chunks == info.chunks == 1
    assert torch.equal(one, two)
    assert alive(info, B) == alive(plain, B)
    assert (info.traces, info.queries, info.syncs) == (3, 3, 2) and info.rays == N * n * n + info.alive[1] + info.alive[2]
    assert not (one == poisoned.SENTINEL).any()


# ---- 7. strips and chunks ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,emitters,B", [(2, False, 3), (3, True, 2)])
def test_chunks_and_strips_never_change_a_bit(n, emitters, B):
    r = Renderer(HostScene.builtin())
    hits = records()
    N = hits.size
    kw = dict(bounces=B, samples=n, gather_depth=2, seed=11, emitters=emitters)
    want = r.indirect_paths(hits, **kw)
    counts = alive(r.paths_info(), B)
    assert 0 < counts[0][B - 1] < counts[0][0]
    for chunk in (0, 1013, 7 * H37):
        got = r.indirect_paths(hits, chunk_records=chunk, compact=True, **kw)
        assert_same(got, want, f"n{n} B{B} chunk_records {chunk}")
        info = r.paths_compact_info()
        assert info.chunks == (-(-N // chunk) if chunk else 1) and alive(info, B) == counts
        assert info.rays == N * n * n + sum(counts[0][1:])
    parts, sums = [], [0] * B
    for x0, x1 in STRIPS:
        parts.append(r.indirect_paths(np.ascontiguousarray(hits[x0:x1]), key0=x0 * H37, chunk_records=13 * H37, compact=True, **kw))
        sums = [a + b for a, b in zip(sums, alive(r.paths_compact_info(), B)[0])]
    assert r.paths_compact_info().records == 40 * H37 and r.paths_compact_info().chunks == 4
    assert_same(np.concatenate(parts), want, f"n{n} B{B} strips")
    assert sums == counts[0]
    launches = r.timing().launches
    assert r.indirect_paths(hits[:0], compact=True, **kw).shape == (0, H37, 3)           # an empty batch launches nothing
    r.indirect_paths_device(0, 0, 0, 0, compact=True)
    assert r.timing().launches == launches and r.paths_compact_info().records == 40 * H37


# ---- 8. the base, poisoned outputs, the device entry on a side stream ---------------------------------------------------------------------

@pytest.mark.parametrize("n,emitters,chunk,B", [(3, False, 0, 2), (2, True, 7 * H37, 3), (2, False, 1013, 3)])
def test_the_base_in_place_and_out_of_place_into_poisoned_outputs(n, emitters, chunk, B):
    import torch
    r = Renderer(HostScene.builtin())
    rgb, hits = np.array(indirect_ref.oracle_gather(*BUILTIN)[0]), records()
    hits["object"][5, 7] = -1                                              # more dead records than the frame's three
    hits["flags"][40, 2] |= indirect_ref.HIT_LIGHT
    N = hits.size
    live = ao_ref.live_records(hits).reshape(hits.shape)
    kw = dict(bounces=B, samples=n, gather_depth=1, gain=0.75, seed=4, emitters=emitters, chunk_records=chunk)
    term = r.indirect_paths(hits, **kw)                                    # (the in-place call: its own tests pin it)
    want = r.indirect_paths(hits, base=rgb, **kw)
    assert_same(r.indirect_paths(hits, compact=True, **kw), term, "host, no base")
    assert not term[~live].view(np.uint32).any() and (term[live] != 0).any()
    assert_same(r.indirect_paths(hits, base=rgb, compact=True, **kw), want, "host, with a base")
    assert_same(want[~live], rgb[~live], "dead records return the base")
    d_hits = poisoned._on_device(hits.view(np.int32))
    d_base = poisoned._on_device(rgb.view(np.int32))
    side = torch.cuda.Stream()                                             # the device entry runs on a side stream
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert poisoned._stream() == side.cuda_stream != 0
        for with_base in (True, False):
            what = f"rt_indirect_paths_compact_device 61x37 n={n} B={B} base {with_base}"
            expect = want if with_base else term
            poisoned.assert_reference_has_no_sentinel(expect, what)
            o = poisoned._Outputs([(N * 3, 3, poisoned.RGB, False)])
            r.indirect_paths_device(N, d_hits.data_ptr(), d_base.data_ptr() if with_base else 0, o.ptrs()[0], poisoned._stream(),
                                    compact=True, **kw)
            out, = o.checked(r, H37, 0, 1, what)                            # every word written, none beside
            assert_same(out.view(F).reshape(expect.shape), expect, what)
        assert np.array_equal(d_base.cpu().numpy().view(F).reshape(rgb.shape).view(np.uint32), rgb.view(np.uint32))   # the base unchanged
        in_place = d_base.clone()
        r.indirect_paths_device(N, d_hits.data_ptr(), in_place.data_ptr(), in_place.data_ptr(), poisoned._stream(), compact=True, **kw)
        torch.cuda.synchronize()
        assert_same(in_place.cpu().numpy().view(F).reshape(rgb.shape), want, "in place")
    info = r.paths_compact_info()
    stages = (info.raygen_ms, info.trace_ms, info.query_ms, info.step_ms, info.resolve_ms)
    assert all(t > 0 for t in stages)
    assert r.timing().last_kernel_ms == pytest.approx(sum(stages), rel=1e-12)
    r.render(W61, H37, 2)                                                  # another launch: the timing is that launch's again
    assert r.timing().last_kernel_ms != pytest.approx(sum(stages), rel=1e-12)


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------------

def test_a_capturing_stream_is_refused_and_the_next_call_is_unharmed():
    """the call waits for its stream, so it cannot be recorded: RT_ERR_INVALID before anything is enqueued -- the capture ends
    with an empty graph -- and the handle's next call gives the definition's words.  The Renderer is this test's own."""
    import torch
    r = Renderer(HostScene.builtin())
    try:
        hits = records()
        N = hits.size
        kw = dict(bounces=3, samples=2, gather_depth=1, seed=6)
        want = r.indirect_paths(hits, **kw)
        assert_same(r.indirect_paths(hits, compact=True, **kw), want, "before the capture")
        before = bytes(memoryview(r.paths_compact_info()))
        d_hits = poisoned._on_device(hits.view(np.int32))
        out = torch.zeros((N * 3,), dtype=torch.int32, device="cuda")
        lib = capi.load_library()
        p = capi.RtPathsParams(2, 1, 0, 0, 6, 0, 1.0, 3)
        launches = r.timing().launches
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = lib.rt_indirect_paths_compact_device(r._scene, C.byref(p), N, d_hits.data_ptr(), None, out.data_ptr(),
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
            message = lib.rt_last_error().decode()
        torch.cuda.synchronize()
        assert rc == capi.RT_ERR_INVALID and "capturing" in message and "rt_indirect_paths_device" in message, (rc, message)
        assert int(out.abs().max()) == 0 and r.timing().launches == launches   # nothing was enqueued, nothing ran
        assert bytes(memoryview(r.paths_compact_info())) == before            # (a refused call is not the handle's last call)
        del graph
        assert_same(r.indirect_paths(hits, compact=True, **kw), want, "after the refusal")
        out2 = torch.zeros((N * 3,), dtype=torch.int32, device="cuda")
        r.indirect_paths_device(N, d_hits.data_ptr(), 0, out2.data_ptr(), poisoned._stream(), compact=True, **kw)
        torch.cuda.synchronize()
        assert_same(out2.cpu().numpy().view(F).reshape(want.shape), want, "after the refusal (device)")
    finally:
        r.close()


def test_argument_errors_carry_rt_indirect_paths_messages_and_launch_nothing():
    r = Renderer(HostScene.builtin())
    hits = records()
    kw0 = dict(bounces=2, samples=2)
    want = r.indirect_paths(hits, compact=True, **kw0)
    launches = r.timing().launches
    for kw, word in ((dict(bounces=0), "bounces"), (dict(bounces=9), "bounces"), (dict(bounces=9, samples=9), "samples"),
                     (dict(bounces=8, gather_depth=-1), "gather_depth")):
        messages = []
        for compact in (True, False):
            with pytest.raises(RtError) as e:
                r.indirect_paths(hits, compact=compact, **kw)
            assert e.value.code == capi.RT_ERR_INVALID and word in e.value.message, (kw, e.value.message)
            messages.append(e.value.message)
        assert messages[0] == messages[1]
    with pytest.raises(RtError) as e:                                     # a misaligned base
        r.indirect_paths_device(hits.size, 0x10000, 0x10002, 0x10000, compact=True)
    assert e.value.code == capi.RT_ERR_INVALID and "d_base_rgb must be 4-byte aligned" in e.value.message
    with pytest.raises(RtError) as e:
        r.indirect_diffuse(hits, bounces=0, compact=True)                  # compact: the new call, whatever bounces is
    assert "bounces" in e.value.message
    assert r.timing().launches == launches
    assert_same(r.indirect_paths(hits, compact=True, **kw0), want, "after the refusals")


def test_a_soft_shadow_scene_is_refused_and_the_handle_renders_on():
    import oracle_lib
    from test_soft_gpu import lights_of, make
    from test_texture_gpu import Desc
    area = [(i, 2, 0.6) for i in lights_of(oracle_lib.OracleScene.builtin())]
    r = make(Desc(HostScene.builtin()), area)
    W, H, depth = 40, 32, 2
    before, hits = r.render_gbuffer(W, H, depth)
    launches = r.timing().launches
    for kw in (dict(samples=2), dict(samples=1, emitters=True, bounces=8), dict(bounces=1)):
        with pytest.raises(RtError) as e:
            r.indirect_paths(hits, compact=True, **kw)
        assert e.value.code == capi.RT_ERR_INVALID and "area lights" in e.value.message and "chunk_records" in e.value.message
    with pytest.raises(RtError) as e:                                     # the last check: a misaligned base is reported before it
        r.indirect_paths_device(hits.size, 0x10000, 0x10002, 0x10000, compact=True)
    assert e.value.code == capi.RT_ERR_INVALID and "d_base_rgb" in e.value.message
    assert r.timing().launches == launches
    assert_same(r.render(W, H, depth), before, "the handle after the refusal")


# ---- 10. the two infos ----------------------------------------------------------------------------------------------------------------

def test_the_two_infos_do_not_touch_each_other():
    r = Renderer(HostScene.builtin())
    hits = records()
    zero = bytes(136)
    assert bytes(memoryview(r.paths_compact_info())) == zero               # all zero before the first call
    r.indirect_paths(hits, 2, 2)
    plain = bytes(memoryview(r.paths_info()))
    assert bytes(memoryview(r.paths_compact_info())) == zero
    r.indirect_paths(hits[:30], 3, 3, compact=True)
    compact = bytes(memoryview(r.paths_compact_info()))
    assert compact != zero and bytes(memoryview(r.paths_info())) == plain
    assert r.paths_compact_info().records == 30 * H37 and r.paths_info().records == hits.size
    r.indirect_paths(hits[:10], 2, 1)
    assert bytes(memoryview(r.paths_compact_info())) == compact and r.paths_info().records == 10 * H37


# ---- 11. the call on another stream than the handle's last, held, call ----------------------------------------------------------------

@pytest.mark.parametrize("first_compact", [False, True], ids=["in-place-then-compact", "compact-then-compact"])
def test_the_call_on_another_stream_than_a_held_paths_call_of_the_handle(first_compact):
    """test_stream_order_gpu.py's pattern and its run_held(): stream A is held busy, call 1 is issued on it, and with nothing
    synchronised call 2 -- this header's, other seed, other key0, so that it generates other rays into the handle's scratch --
    on stream B.  Call 1 is rt_indirect_paths_device, which never waits and so has not started when call 2 is issued (waits =
    False: run_held's assertion for waits = True is that call 1 DID wait for its held stream, which only this header's call
    does) or this header's call as well (waits = True)."""
    import held_stream
    import stream_order_refs as refs
    from test_stream_order_gpu import Outputs, run_held
    st = held_stream.streams()
    I = refs.INDIRECT
    recs = refs.records()
    N = recs.size
    orc = refs.oracle()
    d_hits = poisoned._on_device(np.ascontiguousarray(recs).view(np.int32))
    r = Renderer(HostScene.builtin())

    class Pair:
        case, handle, reset, waits = "paths-compact", None, None, first_compact
        want = tuple((paths_ref.paths(orc, recs, I["samples"], 3, I["gather_depth"], 1.0, c["seed"], c["key0"])[0],) for c in I["calls"])

        def __init__(self):
            self.out = (Outputs(self.want[0]), Outputs(self.want[1]))

        def issue(self, k, stream):
            r.indirect_paths_device(N, d_hits.data_ptr(), 0, self.out[k].ptrs()[0], stream, bounces=3, samples=I["samples"],
                                    gather_depth=I["gather_depth"], compact=(first_compact or k == 1), **I["calls"][k])

    assert refs.differing_share(Pair.want[0], Pair.want[1]) > 0.5
    run_held(Pair(), st["side"], st["other"], f"paths {'compact' if first_compact else 'in place'} side, then compact other")
    assert r.paths_compact_info().records == N


# ---- 12. composition and the executable -----------------------------------------------------------------------------------------------

def test_the_compositions_with_compact_equal_their_forms_without():
    r = Renderer(HostScene.builtin())
    W, H, depth = 40, 36, 3
    kw = dict(samples=2, gather_depth=1, gain=1.0, seed=0)
    rgb, hits = r.render_gbuffer(W, H, depth)
    want = r.render_indirect(W, H, depth, bounces=2, **kw)
    assert_same(want, r.indirect_paths(hits, 2, base=rgb, **kw), "render_indirect(bounces=2)")
    r.indirect_paths(hits[:1], 2, compact=True)
    assert_same(r.render_indirect(W, H, depth, bounces=2, compact=True, **kw), want, "render_indirect(bounces=2, compact=True)")
    assert r.paths_compact_info().records == W * H and r.paths_compact_info().syncs == 1
    assert_same(r.indirect_diffuse(hits, base=rgb, bounces=2, compact=True, **kw), want, "indirect_diffuse(bounces=2, compact=True)")
    one = r.indirect_diffuse(hits, base=rgb, **kw)
    assert_same(r.indirect_diffuse(hits, base=rgb, compact=True, **kw), one, "indirect_diffuse(compact=True): one bounce")
    assert r.paths_compact_info().syncs == 0 and r.paths_compact_info().records == W * H
    assert_same(r.render_indirect(W, H, depth, compact=True, **kw), one, "render_indirect(compact=True): one bounce")
    assert paths_ref.differing_share(one, want, hits) >= 0.5
    for refine in (False, True):
        scaled = r.indirect_diffuse_scaled(hits, 2, base=rgb, bounces=2, refine=refine, **kw)
        assert_same(r.indirect_diffuse_scaled(hits, 2, base=rgb, bounces=2, refine=refine, compact=True, **kw), scaled,
                    f"indirect_diffuse_scaled(bounces=2, refine={refine}, compact=True)")
        assert_same(r.render_indirect(W, H, depth, scale=2, refine=refine, bounces=2, compact=True, **kw), scaled,
                    f"render_indirect(scale=2, refine={refine}, bounces=2, compact=True)")


def test_the_executable_writes_the_same_frame_with_the_flag(tmp_path):
    exe = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
    W, H, depth = 40, 36, 3
    plain_txt, compact_txt = tmp_path / "plain.txt", tmp_path / "compact.txt"
    common = [exe, "--width", str(W), "--height", str(H), "--depth", str(depth), "--indirect", "2:1:1:0", "--indirect-bounces", "2"]
    p = subprocess.run(common + ["--out", str(plain_txt)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Indirect paths" in p.stdout and "compact" not in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    p = subprocess.run(common + ["--indirect-compact", "--out", str(compact_txt)], cwd=tmp_path, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0 and "Indirect paths (compact)" in p.stdout and "syncs" in p.stdout and "alive" in p.stdout, \
        (p.returncode, p.stdout[-500:], p.stderr[-500:])
    got_lines, want_lines = compact_txt.read_text().splitlines()[10:], plain_txt.read_text().splitlines()[10:]
    assert len(got_lines) == W * H and got_lines == want_lines
