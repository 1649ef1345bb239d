"""Diffuse light paths of more than one bounce (include/rt_paths.h) on the GPU against their definition: rt_indirect_paths against
paths_ref on the CPU oracle where the oracle covers the scene, else against paths_ref's step over the handle's own
rt_indirect_rays, rt_trace_rays and rt_intersect_rays (pinned by their own tests); alive[] against the reference's counts.  The
conditions these comparisons rest on -- every compared bounce changes at least half of the live records -- are asserted on the
reference by tests/test_paths_cpu.py.  Bar: BIT-EXACT."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import adaptive_frames
import ao_ref
import indirect_ref
import paths_ref
import poisoned
from tilecoderaytracer_amd import HostScene, Renderer, RtError, capi, indirect_rays
from tilecoderaytracer_amd.renderer import HIT_DTYPE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W61, H37 = 61, 37
STRIPS = ((0, 20), (20, 21), (21, 61))
FRAME = {f[0]: f for f in indirect_ref.FRAMES}
BUILTIN = FRAME["builtin"]
frame_id = lambda f: f"{f[0]}{f[1]}x{f[2]}"      # noqa: E731


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)
    if not same.all():
        bad = np.argwhere(~same.all(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} cells differ, first at {bad[0].tolist()}: gpu={got[tuple(bad[0])]} "
                             f"ref={want[tuple(bad[0])]}")


def records(frame=BUILTIN):
    """the oracle's records of a frame, writable and C-contiguous"""
    return np.array(indirect_ref.oracle_gather(*frame)[1], dtype=HIT_DTYPE, order="C")


def alive(info, B):
    return [int(v) for v in info.alive[:B]], [int(v) for v in info.alive[B:]]


def own_walk(r, hits, kd, n, gather_depth, seed, gain=1.0, key0=0):
    """paths_ref's step over the handle's own public calls: rt_indirect_rays, rt_trace_rays, rt_intersect_rays"""
    return paths_ref.Walk(paths_ref.renderer_tracer(r, gather_depth), hits, n, kd, gain, seed, key0,
                          raygen=lambda rec, n_, seed_, key_: indirect_rays(rec, n_, seed=seed_, key0=key_))


def check_oracle_frame(frame, B, emitters, with_base):
    key, W, H, depth, n, seed, gather_depth = frame
    rgb = indirect_ref.oracle_gather(*frame)[0]
    want = paths_ref.oracle_term(frame, B, emitters, with_base)
    r = Renderer(adaptive_frames.host_scene(key))
    got = r.indirect_paths(records(frame), B, n, gather_depth, seed=seed, emitters=emitters, base=rgb if with_base else None)
    assert_same(got, want, f"{key} {W}x{H} n{n} B{B} emitters {emitters} base {with_base}")
    info = r.paths_info()
    assert (info.records, info.rays, info.chunks) == (W * H, W * H * n * n * B, 1)
    assert alive(info, B) == (paths_ref.oracle_walk(frame).counts(B), [0] * (8 - B))
    assert info.raygen_ms > 0 and info.trace_ms > 0 and info.query_ms > 0 and info.step_ms > 0 and info.resolve_ms > 0
    # (B >= 2: a query is launched at every bounce but, with emitters, the last)
    assert r.launch_info().kernel.decode().endswith("_rays" if emitters else "_hits")


# ---- 1. every word against the CPU oracle ---------------------------------------------------------------------------------------

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


def test_one_sample_a_record_at_three_bounces():
    key, W, H, depth, _, seed, gather_depth = BUILTIN
    check_oracle_frame((key, W, H, depth, 1, seed, gather_depth), 3, False, True)


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
            r.indirect_paths_device(N, d_hits.data_ptr(), base, two.data_ptr(), poisoned._stream(), bounces=1, **kw)
            torch.cuda.synchronize()
            assert torch.equal(one, two), (key, emitters, bool(base))
            info = r.paths_info()
            assert (info.records, info.rays, info.chunks) == (N, N * n * n, 1) and (info.query_ms > 0) == (not emitters)
            assert alive(info, 1) == (paths_ref.oracle_walk(frame).counts(1), [0] * 7)
    assert_same(one.cpu().numpy().view(F).reshape(W, H, 3), indirect_ref.oracle_term(frame, True, True, 0.75), f"{key}: one bounce")


# ---- 2. records whose lanes straddle workgroups; paths that all end early ----------------------------------------------------------

@pytest.mark.parametrize("n", [6, 7])
def test_handmade_records_whose_lanes_straddle_workgroups(n):
    """the hand-made records -- misses, lights, inside hits, an unknown object -- at S = 36 and 49 with key0 = 0xFFFFFFF0: a
    record's paths straddle the step's workgroups (256 paths: 7.1 and 5.2 records) and the resolve's (28 and 20 records), and the
    keys -- the records' and, times S, the paths' -- wrap inside the batch.  Against the handle's own ray batches and queries."""
    import oracle_lib
    r = Renderer(HostScene.builtin())
    kd = indirect_ref.object_diffuse(oracle_lib.OracleScene.builtin())
    hits = indirect_ref.handmade_records()
    S, key0 = n * n, 0xFFFFFFF0
    live = ao_ref.live_records(hits)
    assert len(hits) % (1024 // S) != 0 and (len(hits) * S) % 256 != 0
    base = np.random.RandomState(n).uniform(0, 1, (len(hits), 3)).astype(F)
    walk = own_walk(r, hits, kd, n, 1, 0xC0FFEE, 0.75, key0)
    for emitters in (False, True):
        got = r.indirect_paths(hits, 2, n, 1, 0.75, seed=0xC0FFEE, key0=key0, emitters=emitters, base=base)
        assert_same(got, walk.term(2, emitters, base), f"handmade n{n} emitters {emitters}")
        assert_same(got[~live], base[~live], "dead records return the base")
        assert alive(r.paths_info(), 2) == (walk.counts(2), [0] * 6)
    counts = walk.counts(2)
    assert counts[0] == S * live.sum() and 0 < counts[1] < counts[0]
    assert not indirect_ref.same_bits(got, r.indirect_paths(hits, 1, n, 1, 0.75, seed=0xC0FFEE, key0=key0, emitters=True, base=base))


def test_paths_that_all_end_at_their_first_ray():
    """records high above the built-in scene that look away from it: every gather ray misses, every path ends after bounce 0,
    and three bounces are one bounce bit for bit"""
    rng = np.random.RandomState(8)
    hits = np.zeros(300, dtype=HIT_DTYPE)
    hits["object"] = 4
    hits["point"] = (np.array([0.0, 0.0, 1000.0]) + rng.uniform(-5, 5, (300, 3))).astype(F)
    hits["normal"] = (0.0, 0.0, 1.0)
    hits["color"] = rng.uniform(0.2, 1, (300, 3)).astype(F)
    hits["distance"] = F(1.0)
    r = Renderer(HostScene.builtin())
    one = r.indirect_paths(hits, 1, 3, 1, seed=2)
    assert (r.intersect_rays(indirect_rays(hits, 3, seed=2).reshape(-1, 6))["object"] < 0).all()
    for emitters in (False, True):
        three = r.indirect_paths(hits, 3, 3, 1, seed=2, emitters=emitters)
        assert_same(three, one, f"all paths end early, emitters {emitters}")
        assert alive(r.paths_info(), 3) == ([300 * 9, 0, 0], [0] * 5)
    assert_same(one, r.indirect_diffuse(hits, 3, 1, seed=2), "one bounce")
    assert (one > 0).all()                                                   # the sky's colour, weighted


# ---- 3. scenes the oracle does not cover: the composition of the public calls -----------------------------------------------------

def test_an_image_textured_scene_against_its_own_ray_batches():
    import texture_ref
    from test_texture_gpu import Desc, image_planes
    host, floor, wall = image_planes(HostScene.empty())
    texels = np.random.RandomState(5).uniform(0, 1, (16, 16, 3)).astype(F)
    d = Desc(host)
    d.objs[floor].texture = 0
    d.objs[wall].texture = 0
    r = d.make(images=[(texels, F(5.0), F(3.5), texture_ref.REPEAT)])
    kd = np.array([d.objs[i].diffuse for i in range(d.n)], dtype=F)
    W, H, depth, n = 45, 34, 3, 3
    rgb, hits = r.render_gbuffer(W, H, depth)
    walk = own_walk(r, hits, kd, n, 2, 3, 1.25)
    for B, emitters in ((2, False), (3, False), (3, True)):
        got = r.indirect_paths(hits, B, n, 2, 1.25, seed=3, emitters=emitters, base=rgb)
        assert_same(got, walk.term(B, emitters, rgb), f"image planes B{B} emitters {emitters}")
        assert alive(r.paths_info(), B) == (walk.counts(B), [0] * (8 - B))
    assert r.kernel_name() == "rt_render_kernel_rays_image"
    assert paths_ref.differing_share(walk.term(1), walk.term(2), hits) >= 0.5
    assert len(np.unique(walk.w[0][walk.alive[1]], axis=0)) > 50             # the paths' weights are texels


def test_a_refractive_scene_against_its_own_ray_batches():
    from test_refract_gpu import glass_builtin, make
    from test_texture_gpu import Desc
    host = HostScene.builtin()
    refr = glass_builtin(host)
    d = Desc(host)
    r = make(d, refractive=refr)
    kd = np.array([d.objs[i].diffuse for i in range(d.n)], dtype=F)
    W, H, depth, n = 48, 36, 4, 2
    rgb, hits = r.render_gbuffer(W, H, depth)
    walk = own_walk(r, hits, kd, n, 3, 0)
    for B, emitters in ((2, False), (3, False), (3, True)):
        got = r.indirect_paths(hits, B, n, 3, seed=0, emitters=emitters, base=rgb)
        assert_same(got, walk.term(B, emitters, rgb), f"glass B{B} emitters {emitters}")
        assert alive(r.paths_info(), B) == (walk.counts(B), [0] * (8 - B))
    assert r.kernel_name() == "rt_render_kernel_rays_refract"
    assert paths_ref.differing_share(walk.term(1), walk.term(2), hits) >= 0.5


# ---- 4. chunks, strips, the base, poisoned outputs ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n,emitters,B", [(2, False, 3), (3, True, 2)])
def test_chunks_and_strips_never_change_a_bit(n, emitters, B):
    r = Renderer(HostScene.builtin())
    hits = records()
    N, S = hits.size, n * n
    kw = dict(bounces=B, samples=n, gather_depth=2, seed=11, emitters=emitters)
    want = r.indirect_paths(hits, **kw)
    info = r.paths_info()
    counts = alive(info, B)
    assert info.chunks == 1 and counts[0][0] == S * int(ao_ref.live_records(hits).sum()) and 0 < counts[0][B - 1] < counts[0][0]
    for chunk in (1013, 1, 0):                                             # two sizes and the default on the one handle
        got = r.indirect_paths(hits, chunk_records=chunk, **kw)
        assert_same(got, want, f"n{n} B{B} chunk_records {chunk}")
        info = r.paths_info()
        assert info.chunks == (-(-N // chunk) if chunk else 1), (chunk, info.chunks)
        assert (info.records, info.rays) == (N, N * S * B) and alive(info, B) == counts
    parts, sums = [], [0] * B
    for x0, x1 in STRIPS:
        parts.append(r.indirect_paths(np.ascontiguousarray(hits[x0:x1]), key0=x0 * H37, chunk_records=13 * H37, **kw))
        sums = [a + b for a, b in zip(sums, alive(r.paths_info(), B)[0])]
    assert r.paths_info().records == 40 * H37 and r.paths_info().chunks == 4
    assert_same(np.concatenate(parts), want, f"n{n} B{B} strips")
    assert sums == counts[0]
    launches = r.timing().launches
    assert r.indirect_paths(hits[:0], **kw).shape == (0, H37, 3)            # an empty batch launches nothing
    r.indirect_paths_device(0, 0, 0, 0)
    assert r.timing().launches == launches and r.paths_info().records == 40 * H37


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
    term = r.indirect_paths(hits, **kw)
    assert not term[~live].view(np.uint32).any() and (term[live] != 0).any()           # a dead record, no base: +0.0
    want = rgb + term                                                      # numpy fp32: one add a word
    assert_same(r.indirect_paths(hits, base=rgb, **kw), want, "host, with a base")
    assert_same(want[~live], rgb[~live], "dead records return the base")
    d_hits = poisoned._on_device(hits.view(np.int32))
    d_base = poisoned._on_device(rgb.view(np.int32))
    for with_base in (True, False):
        what = f"rt_indirect_paths_device 61x37 n={n} B={B} base {with_base}"
        ref = want if with_base else term
        poisoned.assert_reference_has_no_sentinel(ref, what)
        o = poisoned._Outputs([(N * 3, 3, poisoned.RGB, False)])
        r.indirect_paths_device(N, d_hits.data_ptr(), d_base.data_ptr() if with_base else 0, o.ptrs()[0], poisoned._stream(), **kw)
        out, = o.checked(r, H37, 0, 1, what)                                # every word written, none beside
        assert_same(out.view(F).reshape(ref.shape), ref, what)
    assert np.array_equal(d_base.cpu().numpy().view(F).reshape(rgb.shape).view(np.uint32), rgb.view(np.uint32))   # the base unchanged
    in_place = d_base.clone()
    r.indirect_paths_device(N, d_hits.data_ptr(), in_place.data_ptr(), in_place.data_ptr(), poisoned._stream(), **kw)
    torch.cuda.synchronize()
    assert_same(in_place.cpu().numpy().view(F).reshape(rgb.shape), want, "in place")
    info = r.paths_info()
    stages = (info.raygen_ms, info.trace_ms, info.query_ms, info.step_ms, info.resolve_ms)
    assert all(t > 0 for t in stages)
    assert r.timing().last_kernel_ms == pytest.approx(sum(stages), rel=1e-12)
    r.render(W61, H37, 2)                                                  # another launch: the timing is that launch's again
    assert r.timing().last_kernel_ms != pytest.approx(sum(stages), rel=1e-12)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------

def test_a_soft_shadow_scene_is_refused_and_the_handle_renders_on():
    import oracle_lib
    from test_soft_gpu import lights_of, make
    from test_texture_gpu import Desc
    area = [(i, 2, 0.6) for i in lights_of(oracle_lib.OracleScene.builtin())]
    r = make(Desc(HostScene.builtin()), area)
    W, H, depth = 40, 32, 2
    before, hits = r.render_gbuffer(W, H, depth)
    for kw in (dict(samples=2), dict(samples=1, emitters=True, bounces=8)):
        with pytest.raises(RtError) as e:
            r.indirect_paths(hits, **kw)
        assert e.value.code == capi.RT_ERR_INVALID and "area lights" in e.value.message and "chunk_records" in e.value.message
    with pytest.raises(RtError) as e:                                     # the last check: a misaligned base is reported before it
        r.indirect_paths_device(hits.size, 0x10000, 0x10002, 0x10000)
    assert e.value.code == capi.RT_ERR_INVALID and "d_base_rgb" in e.value.message
    with pytest.raises(RtError) as e:
        r.indirect_paths_device(hits.size, 0x10000, 0x10000, 0x10000)
    assert e.value.code == capi.RT_ERR_INVALID and "area lights" in e.value.message
    assert_same(r.render(W, H, depth), before, "the handle after the refusal")
    hard = make(Desc(HostScene.builtin()), [])                            # rt_scene_create_soft without an area light: accepted
    plain = Renderer(HostScene.builtin())
    assert_same(hard.indirect_paths(hits, 2, 2), plain.indirect_paths(hits, 2, 2), "no area light")


def test_argument_errors_leave_the_handle_usable():
    r = Renderer(HostScene.builtin())
    hits = records()
    want = r.indirect_paths(hits, 2, 2)
    launches = r.timing().launches
    for kw, word in ((dict(bounces=0), "bounces"), (dict(bounces=9), "bounces"), (dict(bounces=9, samples=9), "samples"),
                     (dict(bounces=8, gather_depth=-1), "gather_depth")):
        with pytest.raises(RtError) as e:
            r.indirect_paths(hits, **kw)
        assert e.value.code == capi.RT_ERR_INVALID and word in e.value.message, (kw, e.value.message)
    with pytest.raises(RtError) as e:
        r.indirect_diffuse(hits, bounces=0)                                # any count but 1 is the new call's to judge
    assert "bounces" in e.value.message
    assert r.timing().launches == launches
    assert_same(r.indirect_paths(hits, 2, 2), want, "after the refusals")


# ---- 6. speed-only options ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", [{"cull": 0}, {"fast": 0}, {"tables": 2}])
@pytest.mark.parametrize("emitters", [False, True])
def test_speed_only_options_never_change_a_bit(options, emitters):
    key, W, H, depth, n, seed, gather_depth = BUILTIN
    rgb = indirect_ref.oracle_gather(*BUILTIN)[0]
    want = paths_ref.oracle_term(BUILTIN, 3, emitters, True)
    r = Renderer(HostScene.builtin())
    r.indirect_paths(records(), 3, n, gather_depth, seed=seed, emitters=emitters, base=rgb)
    default = r.kernel_name()
    for name, value in options.items():
        r.set_option(name, value)
    got = r.indirect_paths(records(), 3, n, gather_depth, seed=seed, emitters=emitters, base=rgb)
    if emitters and "fast" not in options:                              # (the ray batch's kernel, as test_lens_gpu.py names them)
        assert r.kernel_name() != default and r.kernel_name().endswith("_rays")
    assert_same(got, want, f"{options} emitters {emitters}")
    assert alive(r.paths_info(), 3) == (paths_ref.oracle_walk(BUILTIN).counts(3), [0] * 5)


# ---- 7. the second of two calls on one handle across a change of stream -------------------------------------------------------------

def test_two_calls_of_one_handle_across_a_change_of_stream():
    """test_stream_order_gpu.py's pattern and its run_held(): stream A is held busy, call 1 is issued on it, and with nothing
    synchronised call 2 -- other seed, other key0, so that it generates other rays into the same scratch -- on stream B"""
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
        case, handle, reset, waits = "paths", None, None, False
        want = tuple((paths_ref.paths(orc, recs, I["samples"], 2, I["gather_depth"], 1.0, c["seed"], c["key0"])[0],) for c in I["calls"])

        def __init__(self):
            self.out = (Outputs(self.want[0]), Outputs(self.want[1]))

        def issue(self, k, stream):
            r.indirect_paths_device(N, d_hits.data_ptr(), 0, self.out[k].ptrs()[0], stream, bounces=2, samples=I["samples"],
                                    gather_depth=I["gather_depth"], **I["calls"][k])

    assert refs.differing_share(Pair.want[0], Pair.want[1]) > 0.5
    run_held(Pair(), st["side"], st["other"], "paths side-then-other")


# ---- 8. composition -----------------------------------------------------------------------------------------------------------------

def test_render_indirect_with_bounces_is_the_composition_of_the_public_calls():
    r = Renderer(HostScene.builtin())
    W, H, depth = 40, 36, 3
    kw = dict(samples=2, gather_depth=1, gain=1.0, seed=0)
    rgb, hits = r.render_gbuffer(W, H, depth)
    want = r.indirect_paths(hits, 2, base=rgb, **kw)
    assert_same(r.render_indirect(W, H, depth, bounces=2, **kw), want, "render_indirect(bounces=2)")
    assert_same(r.indirect_diffuse(hits, base=rgb, bounces=2, **kw), want, "indirect_diffuse(bounces=2)")
    one = r.render_indirect(W, H, depth, **kw)
    assert_same(one, r.indirect_diffuse(hits, base=rgb, **kw), "render_indirect, one bounce")
    assert paths_ref.differing_share(one, want, hits) >= 0.5
    scaled = r.indirect_diffuse_scaled(hits, 2, base=rgb, bounces=2, refine=True, **kw)
    assert_same(r.render_indirect(W, H, depth, scale=2, refine=True, bounces=2, **kw), scaled, "render_indirect(scale=2, bounces=2)")
    assert not indirect_ref.same_bits(scaled, r.indirect_diffuse_scaled(hits, 2, base=rgb, refine=True, **kw))
    from tilecoderaytracer_amd import subsample_hits, upsample_guided
    lo = r.indirect_paths(subsample_hits(hits, 2, True), 2, **kw)
    assert_same(r.indirect_diffuse_scaled(hits, 2, base=rgb, bounces=2, **kw),
                upsample_guided(hits, lo, 2, 3, False, True, 0.0, 0.0, rgb, True)[0], "indirect_diffuse_scaled(bounces=2)")


def test_render_indirect_with_mirrors_and_bounces_gathers_at_the_terminal_records():
    import mirror_scenes
    r = Renderer(mirror_scenes.host_scene("room"))
    mirrors = dict(max_bounces=3, min_reflective=1.0)
    kw = dict(samples=2, gather_depth=1, gain=1.25, seed=3)
    rgb, hits, _, weight, path = r.render_gbuffer_mirrored(W61, H37, 2, **mirrors)
    term = r.indirect_paths(np.ascontiguousarray(hits), 2, **kw)
    assert_same(r.render_indirect(W61, H37, 2, mirrors=mirrors, bounces=2, **kw), rgb + weight * term, "render_indirect(mirrors, bounces=2)")
    assert not indirect_ref.same_bits(term, r.indirect_diffuse(np.ascontiguousarray(hits), **kw))


def test_the_executable_writes_that_frame(tmp_path):
    from tilecoderaytracer_amd.host import write_screen_txt
    exe = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
    W, H, depth = 40, 36, 3
    out_txt, one_txt, want_txt = (tmp_path / name for name in ("out.txt", "one.txt", "want.txt"))
    common = [exe, "--width", str(W), "--height", str(H), "--depth", str(depth)]
    p = subprocess.run(common + ["--indirect", "2:1:1:0", "--indirect-bounces", "2", "--out", str(out_txt)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Indirect paths" in p.stdout and "alive" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    p = subprocess.run(common + ["--indirect", "2:1:1:0", "--indirect-bounces", "1", "--out", str(one_txt)], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "Indirect diffuse" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    write_screen_txt(str(want_txt), Renderer(HostScene.builtin()).render_indirect(W, H, depth, samples=2, bounces=2))
    got_lines, want_lines = out_txt.read_text().splitlines()[10:], want_txt.read_text().splitlines()[10:]
    assert len(got_lines) == W * H and got_lines == want_lines
    assert got_lines != one_txt.read_text().splitlines()[10:]
