"""Adaptive supersampling (include/rt_capi_adaptive.h) on the GPU against its definition: the frame is where(flags,
rt_render_ssaa, rt_render) with the flags adaptive_ref's -- built from the CPU oracle's frames and query_ref's records where the
oracle covers the scene, else from the GPU's own rt_render_ssaa, rt_render and rt_render_gbuffer, each pinned by its own tests.
Bar: BIT-EXACT, colours and flags."""
import numpy as np
import pytest

import adaptive_frames
import adaptive_ref
import cameras
import poisoned
from test_adaptive_cpu import clause_rectangles
from tilecoderaytracer_amd import HostScene, Renderer, RtError, adaptive_flags, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

pytestmark = pytest.mark.gpu

F = np.float32


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)
    if not same.all():
        bad = np.argwhere(~same.all(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at {bad[0].tolist()}: gpu={got[tuple(bad[0])]} "
                             f"ref={want[tuple(bad[0])]}")


def assert_flags(got, want, what):
    assert got.dtype == np.bool_ and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint8), want.astype(np.uint8)), \
        (what, "first difference at", np.argwhere(got != want)[0].tolist(), "gpu", int(got.sum()), "ref", int(want.sum()))


def check_info(r, flags, k, what):
    info = r.adaptive_info()
    assert (info.pixels, info.flagged) == (flags.size, int(flags.sum())), (what, info.pixels, info.flagged, int(flags.sum()))
    assert info.rays == (info.flagged * k * k if k > 1 else 0), (what, info.rays)
    assert (info.chunks > 0) == (info.rays > 0), (what, info.chunks)
    stages = (info.first_pass_ms, info.flag_ms, info.trace_ms, info.resolve_ms)
    assert info.first_pass_ms > 0 and info.flag_ms > 0 and all(t >= 0 for t in stages), (what, stages)
    assert r.timing().last_kernel_ms == pytest.approx(sum(stages), rel=1e-12), what
    return info


def own_reference(r, W, H, depth, k, **kw):
    """(expected frame, flags) from the handle's own rt_render_ssaa, rt_render and rt_render_gbuffer"""
    plain, hits = r.render_gbuffer(W, H, depth)
    assert_same(plain, r.render(W, H, depth), "the G-buffer's colours are rt_render's")
    flags = adaptive_ref.flags(plain, hits, **kw)
    return adaptive_ref.expected_frame(flags, r.render_ssaa(W, H, depth, k), plain), flags


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("key,W,H,depth,share", adaptive_frames.FRAMES)
def test_against_the_oracle(key, W, H, depth, share, k):
    what = f"{key} {W}x{H} d{depth} k{k}"
    plain, hits = adaptive_frames.first_pass(key, W, H, depth)
    flags = adaptive_ref.flags(plain, hits)
    want = adaptive_ref.expected_frame(flags, adaptive_frames.supersampled(key, W, H, depth, k), plain)
    r = Renderer(adaptive_frames.host_scene(key))
    got, got_flags = r.render_adaptive(W, H, depth, samples=k, return_flags=True)
    assert_flags(got_flags, flags, what)
    assert_same(got, want, what)
    check_info(r, flags, k, what)
    assert r.launch_info().kernel.decode().endswith("_rays")             # the call's last render-kernel launch
    assert_same(r.render_adaptive(W, H, depth, samples=k), want, what + " (no flags asked for)")


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("frame,options,first,second", [
    (adaptive_frames.OPTION_FRAMES[0], {"tables": 2}, "rt_render_kernel_large_gbuffer", "rt_render_kernel_large_rays"),
    (adaptive_frames.OPTION_FRAMES[1], {"cull": 0}, "rt_render_kernel_items_gbuffer", "rt_render_kernel_items_rays"),
])
def test_against_the_oracle_through_other_kernels(frame, options, first, second, k):
    key, W, H, depth = frame
    what = f"{key} {options} k{k}"
    plain, hits = adaptive_frames.first_pass(key, W, H, depth)
    flags = adaptive_ref.flags(plain, hits)
    adaptive_ref.assert_share(flags, what)
    want = adaptive_ref.expected_frame(flags, adaptive_frames.supersampled(key, W, H, depth, k), plain)
    r = Renderer(adaptive_frames.host_scene(key))
    for name, value in options.items():
        r.set_option(name, value)
    r.render_gbuffer(W, H, depth)
    assert r.kernel_name() == first
    got, got_flags = r.render_adaptive(W, H, depth, samples=k, return_flags=True)
    assert r.kernel_name() == second
    assert_flags(got_flags, flags, what)
    assert_same(got, want, what)
    check_info(r, flags, k, what)


# ---- 2. flag_all is rt_render_ssaa, samples = 1 is rt_render ---------------------------------------------------------------------

def pitched_and_rolled():
    a = cameras.ANCHORS["builtin"]
    focus = np.array(a["focus"])
    return cameras.camera(focus + a["unit"] * np.array([-0.5, -1.5, 3.5]), focus, roll=0.6)      # "pitched_down", rolled


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("camera", [None, "pitched_down", "rolled_1p45", "pitched_and_rolled"])
def test_flag_all_is_rt_render_ssaa_on_every_pixel(camera, k):
    """holds the ray generation at every pixel, the borders included"""
    host = HostScene.builtin()
    if camera is not None:
        cam = pitched_and_rolled() if camera == "pitched_and_rolled" else cameras.catalogue("builtin")[camera]
        cameras.put(cam, host=host)
    so = np.array(list(host.camera.contents.screen_origin), dtype=F)
    assert not (np.signbit(so) & (so == 0)).any(), so                    # no -0.0: rt_trace_rays would read it as +0.0
    r = Renderer(host)
    W, H, depth = 61, 37, 4
    want = r.render_ssaa(W, H, depth, k)
    got, flags = r.render_adaptive(W, H, depth, samples=k, flag_all=True, return_flags=True)
    assert flags.all()
    assert_same(got, want, f"flag_all {camera} k{k}")
    info = r.adaptive_info()
    assert (info.pixels, info.flagged, info.rays) == (W * H, W * H, W * H * k * k)


@pytest.mark.parametrize("halo", [False, True], ids=["last-columns", "halo"])
@pytest.mark.parametrize("k", [2, 4])
def test_flag_all_is_rt_render_ssaa_where_k_x_exceeds_2_24(k, halo):
    """the last 8 columns of a frame as wide as rt_render_ssaa admits (k W = 2^31 - k): (float)((x << kl) + i) rounds far above
    2^24 and must round as the supersampling kernels' own pixel numbers do (those are held to the oracle by
    test_large_extents_gpu.py); and the 8 columns before them, which bring a halo column and the scratch copy"""
    W, H, depth = (1 << 31) // k - 1, 37, 3
    x1 = W - 8 if halo else W
    x0 = x1 - 8
    assert k * x0 > 1 << 24 and k * W <= 0x7fffffff < k * (W + 1)
    r = Renderer(HostScene.builtin())
    want = r.render_ssaa(W, H, depth, k, x0=x0, x1=x1)
    got, flags = r.render_adaptive(W, H, depth, samples=k, flag_all=True, x0=x0, x1=x1, return_flags=True)
    assert flags.all()
    assert_same(got, want, f"flag_all W={W} k{k} columns {x0}:{x1}")
    info = r.adaptive_info()
    assert (info.pixels, info.flagged, info.rays) == (8 * H, 8 * H, 8 * H * k * k)
    assert len(np.unique(np.ascontiguousarray(want).view(np.uint32).reshape(-1, 3), axis=0)) >= 2       # (not one flat colour)


@pytest.mark.parametrize("key,W,H,depth", [("builtin", 61, 37, 4), ("grid16", 50, 44, 5)])
def test_one_sample_is_rt_render_with_the_flags_still_reported(key, W, H, depth):
    r = Renderer(adaptive_frames.host_scene(key))
    plain, hits = r.render_gbuffer(W, H, depth)
    want_flags = adaptive_ref.flags(plain, hits)
    got, flags = r.render_adaptive(W, H, depth, samples=1, return_flags=True)
    assert_same(got, r.render(W, H, depth), f"{key} k1")
    assert_flags(flags, want_flags, f"{key} k1")
    r.render_adaptive(W, H, depth, samples=1)
    info = r.adaptive_info()
    assert (info.flagged, info.rays, info.chunks) == (int(want_flags.sum()), 0, 0)
    assert 0 < want_flags.sum() < want_flags.size


# ---- 3. the flag pass alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(clause_rectangles()))
def test_flags_of_the_hand_built_rectangles(name):
    rgb, hits, kw, want = clause_rectangles()[name]
    assert_flags(adaptive_flags(rgb, hits, **kw), want, name)


@pytest.mark.parametrize("Wn,H", [(1, 1), (1, 300), (300, 1), (67, 131), (257, 3), (5, 255), (129, 130)])
def test_flags_of_synthetic_rectangles(Wn, H):
    """random objects, normals and colours in runs, with NaN, inf and misses sprinkled in; sizes that are no multiple of the
    wavefront or the workgroup"""
    rng = np.random.RandomState(Wn * 1000 + H)
    coarse = lambda lo, hi, n: rng.randint(lo, hi, (-(-Wn // n), -(-H // n))).repeat(n, 0).repeat(n, 1)[:Wn, :H]
    hits = np.zeros((Wn, H), HIT_DTYPE)
    hits["object"] = coarse(-1, 4, 5)
    normal = rng.normal(size=(Wn, H, 3)).astype(F) * F(0.15) + np.array([0, 0, 1], F)
    hits["normal"] = normal / np.linalg.norm(normal, axis=-1, keepdims=True).astype(F)
    rgb = (coarse(0, 3, 7)[..., None] * F(0.25) + rng.uniform(0, 0.04, (Wn, H, 3))).astype(F)
    for value in (np.nan, np.inf, -np.inf):
        rgb[rng.uniform(size=(Wn, H)) < 0.01, rng.randint(3)] = value
    hits["normal"][rng.uniform(size=(Wn, H)) < 0.01, 1] = np.nan
    for kw in ({}, dict(color_threshold=0.0, normal_cos=1.0), dict(color_threshold=1e30, normal_cos=-1.0),
               dict(color_threshold=0.3, normal_cos=0.97), dict(flag_all=True)):
        want = adaptive_ref.flags(rgb, hits, **kw)
        assert_flags(adaptive_flags(rgb, hits, **kw), want, f"{Wn}x{H} {kw}")
    if Wn * H > 1000:
        assert 0.05 < adaptive_ref.flags(rgb, hits).mean() < 0.95


def test_flags_device_entry_on_a_stream_into_poisoned_bytes():
    import torch
    r = Renderer(HostScene.builtin())
    Wn, H = 77, 53
    rgb, hits = r.render_gbuffer(Wn, H, 3)
    want = adaptive_ref.flags(rgb, hits)
    what = "rt_adaptive_flags_device 77x53"
    poisoned.assert_reference_has_no_sentinel(want.view(np.uint8), what, poisoned.SENTINEL_BYTE)
    d_rgb, d_hits = poisoned._on_device(rgb), poisoned._on_device(hits)
    o = poisoned._Outputs([(Wn * H, 1, ("flag",), True)])
    params = capi.RtAdaptiveParams(1, 0, 0, 1 / 32, 0.9)
    import ctypes as C
    capi.check(capi.load_library().rt_adaptive_flags_device(0, C.byref(params), Wn, H, d_rgb.data_ptr(), d_hits.data_ptr(),
                                                            o.ptrs()[0], poisoned._stream()))
    flags, = o.checked(r, H, 0, 1, what)
    assert_flags(flags.reshape(Wn, H).view(np.bool_), want, what)
    del torch


# ---- 4. strips and chunks -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k", [("builtin", 2), ("builtin", 4), ("grid16", 2)])
def test_strips_equal_the_whole_frames_columns(name, k):
    """the cut at 61 and the one-column strips are the halo cases: the strip's last column is flagged by the column after it"""
    r = Renderer(HostScene.named(name))
    W, H, depth = 150, 90, 5
    full, full_flags = r.render_adaptive(W, H, depth, samples=k, return_flags=True)
    adaptive_ref.assert_share(full_flags, f"{name} 150x90")
    plain, hits = r.render_gbuffer(W, H, depth)
    assert_flags(full_flags, adaptive_ref.flags(plain, hits), f"{name} k{k} whole frame")
    for x0, x1 in ((0, 24), (24, 61), (61, 150), (149, 150), (13, 14), (1, 149), (7, 7)):
        got, flags = r.render_adaptive(W, H, depth, samples=k, x0=x0, x1=x1, return_flags=True)
        assert_flags(flags, full_flags[x0:x1], f"{name} k{k} strip {x0}:{x1}")
        assert_same(got, full[x0:x1], f"{name} k{k} strip {x0}:{x1}")
        if x1 > x0:
            assert r.adaptive_info().pixels == (x1 - x0) * H
    # the halo decides something: without it, the last column of the strip ending at 61 would be flagged differently
    assert not np.array_equal(adaptive_ref.flags(plain[24:61], hits[24:61])[-1], full_flags[60])


@pytest.mark.parametrize("k", [2, 4])
def test_chunk_pixels_never_changes_a_result(k):
    r = Renderer(HostScene.builtin())
    W, H, depth = 40, 26, 4
    want, want_flags = r.render_adaptive(W, H, depth, samples=k, chunk_pixels=0, return_flags=True)
    flagged = int(want_flags.sum())
    assert r.adaptive_info().chunks == 1 and 64 < flagged < W * H
    for chunk in (1, 7, 64):
        got, flags = r.render_adaptive(W, H, depth, samples=k, chunk_pixels=chunk, return_flags=True)
        assert_flags(flags, want_flags, f"chunk {chunk}")
        assert_same(got, want, f"k{k} chunk {chunk}")
        info = r.adaptive_info()
        assert info.chunks == -(-flagged // chunk) and info.rays == flagged * k * k, (chunk, info.chunks, flagged)


# ---- 5. the device entry point ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,x0,x1,with_flags", [(2, 0, 70, True), (4, 9, 41, True), (2, 33, 70, False), (1, 5, 50, True)])
def test_device_entry_on_a_stream_into_poisoned_outputs(k, x0, x1, with_flags):
    """every colour word and every flag byte is written, nothing before, between or after; d_out_flags = NULL is accepted"""
    r = Renderer(HostScene.builtin())
    W, H, depth = 70, 45, 4
    want, want_flags = r.render_adaptive(W, H, depth, samples=k, x0=x0, x1=x1, return_flags=True)
    what = f"rt_render_adaptive_device {W}x{H} k={k} columns {x0}:{x1}"
    poisoned.assert_reference_has_no_sentinel(want, what)
    n = (x1 - x0) * H
    specs = [(n * 3, 3, poisoned.RGB, False)] + ([(n, 1, ("flag",), True)] if with_flags else [])
    o = poisoned._Outputs(specs)
    ptrs = o.ptrs()
    r.render_adaptive_device(W, H, depth, x0, x1, ptrs[0], ptrs[1] if with_flags else 0, poisoned._stream(), samples=k)
    outs = o.checked(r, H, x0, 1, what)
    assert_same(outs[0].view(F).reshape(x1 - x0, H, 3), want, what)
    if with_flags:
        assert_flags(outs[1].reshape(x1 - x0, H).view(np.bool_), want_flags, what)
    assert r.adaptive_info().flagged == int(want_flags.sum())


def test_device_entry_on_a_side_stream_and_argument_errors():
    import torch
    r = Renderer(HostScene.builtin())
    W, H, depth = 64, 40, 3
    want, want_flags = r.render_adaptive(W, H, depth, samples=2, return_flags=True)
    rgb = torch.zeros((W, H, 3), dtype=torch.float32, device="cuda:0")
    flags = torch.zeros((W, H), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        r.render_adaptive_device(W, H, depth, 0, W, rgb.data_ptr(), flags.data_ptr(), stream.cuda_stream, samples=2)
    stream.synchronize()
    assert_same(rgb.cpu().numpy(), want, "side stream")
    assert_flags(flags.cpu().numpy().view(np.bool_), want_flags, "side stream")
    # the checks that need a scene, in the header's order: rt_render's before the params', the params' before the sizes
    for kw, word in ((dict(samples=3, x1=W + 1), "x0 <= x1"), (dict(samples=3, flag_all=2), "samples"),
                     (dict(flag_all=2, chunk_pixels=-1), "flag_all"), (dict(chunk_pixels=-1, color_threshold=-1.0), "chunk_pixels"),
                     (dict(color_threshold=float("nan"), normal_cos=2.0), "color_threshold"), (dict(normal_cos=2.0), "normal_cos")):
        with pytest.raises(RtError) as e:
            r.render_adaptive(W, H, depth, **kw)
        assert e.value.code == capi.RT_ERR_INVALID and word in e.value.message, (kw, e.value.message)
    with pytest.raises(RtError) as e:
        r.render_adaptive_device(W, H, depth, 0, W, rgb.data_ptr() + 2, 0, 0)
    assert e.value.code == capi.RT_ERR_INVALID and "4-byte" in e.value.message
    assert r.render_adaptive(W, H, depth, x0=7, x1=7).shape == (0, H, 3)         # an empty strip launches nothing
    assert_same(r.render_adaptive(W, H, depth, samples=2), want, "after the refusals")


# ---- 6. the other shadings -------------------------------------------------------------------------------------------------------

def test_an_image_textured_scene():
    import texture_ref
    from test_texture_gpu import Desc, image_planes
    host, floor, wall = image_planes(HostScene.empty())
    texels = np.random.RandomState(5).uniform(0, 1, (16, 16, 3)).astype(F)
    d = Desc(host)
    d.objs[floor].texture = 0
    d.objs[wall].texture = 0
    r = d.make(images=[(texels, F(5.0), F(3.5), texture_ref.REPEAT)])
    W, H, depth = 72, 50, 3
    for k in (2, 4):
        want, flags = own_reference(r, W, H, depth, k)
        adaptive_ref.assert_share(flags, "image planes")
        got, got_flags = r.render_adaptive(W, H, depth, samples=k, return_flags=True)
        assert r.kernel_name() == "rt_render_kernel_rays_image"
        assert_flags(got_flags, flags, f"image planes k{k}")
        assert_same(got, want, f"image planes k{k}")


def test_a_refractive_scene():
    from test_refract_gpu import glass_builtin, make
    from test_texture_gpu import Desc
    host = HostScene.builtin()
    refr = glass_builtin(host)
    r = make(Desc(host), refractive=refr)
    W, H, depth = 64, 48, 4
    for k in (2, 4):
        want, flags = own_reference(r, W, H, depth, k)
        adaptive_ref.assert_share(flags, "glass")
        got, got_flags = r.render_adaptive(W, H, depth, samples=k, return_flags=True)
        assert r.kernel_name() == "rt_render_kernel_rays_refract"
        assert_flags(got_flags, flags, f"glass k{k}")
        assert_same(got, want, f"glass k{k}")


def test_a_soft_shadow_scene_is_refused_and_the_handle_renders_on():
    import oracle_lib
    from test_soft_gpu import lights_of, make
    from test_texture_gpu import Desc
    area = [(i, 2, 0.6) for i in lights_of(oracle_lib.OracleScene.builtin())]
    r = make(Desc(HostScene.builtin()), area)
    W, H, depth = 40, 32, 2
    before = r.render(W, H, depth)
    for kw in (dict(samples=2), dict(samples=1), dict(samples=4, flag_all=True)):
        with pytest.raises(RtError) as e:
            r.render_adaptive(W, H, depth, **kw)
        assert e.value.code == capi.RT_ERR_INVALID and "area lights" in e.value.message and "chunk_pixels" in e.value.message
    assert_same(r.render(W, H, depth), before, "the handle after the refusal")
    hard = make(Desc(HostScene.builtin()), [])                            # rt_scene_create_soft without an area light: accepted
    plain = Renderer(HostScene.builtin())
    assert_same(hard.render_adaptive(W, H, depth), plain.render_adaptive(W, H, depth), "no area light")


# ---- 7. one larger frame ---------------------------------------------------------------------------------------------------------

def test_a_larger_frame_in_several_chunks():
    """1024 x 1024, k = 2: several queue entries per wavefront in both passes, and a list of more than one chunk"""
    r = Renderer(HostScene.builtin())
    W = H = 1024
    depth = 3
    want, flags = own_reference(r, W, H, depth, 2)
    flagged = int(flags.sum())
    assert 20000 < flagged < W * H // 4
    got, got_flags = r.render_adaptive(W, H, depth, samples=2, chunk_pixels=16384, return_flags=True)
    assert_flags(got_flags, flags, "builtin 1024^2")
    assert_same(got, want, "builtin 1024^2 k2")
    info = check_info(r, flags, 2, "builtin 1024^2")
    assert info.chunks == -(-flagged // 16384) > 1
