"""The thin-lens camera (include/rt_capi_lens.h) on the GPU against its definition: rt_lens_rays against lens_ref.rays word for
word, rt_render_lens against lens_ref.resolve of the CPU oracle's colours of those rays where the oracle covers the scene, else
of the GPU's own rt_trace_rays (pinned by its own tests), and against rt_render_ssaa / rt_render where the lens is a pinhole.
Bar: BIT-EXACT."""
import numpy as np
import pytest

import adaptive_frames
import cameras
import lens_ref
import poisoned
from tilecoderaytracer_amd import HostScene, Renderer, RtError, capi, lens_rays

pytestmark = pytest.mark.gpu

F = np.float32
W61, H37 = 61, 37                       # partial tiles on both axes, an odd column count for the chunker
STRIPS = ((0, 20), (20, 21), (21, 61))
APERTURE, FOCUS = lens_ref.lens_of("builtin", cameras.ANCHORS["builtin"]["focus"])


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)
    if not same.all():
        bad = np.argwhere(~same.all(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} cells differ, first at {bad[0].tolist()}: gpu={got[tuple(bad[0])]} "
                             f"ref={want[tuple(bad[0])]}")


def camera_of(name):
    """None: the built-in scene's own camera; else one of cameras.catalogue("builtin") -> a HostScene carrying it"""
    host = HostScene.builtin()
    if name is not None:
        cameras.put(cameras.catalogue("builtin")[name], host=host)
    return host


def own_reference(r, cam, W, H, depth, n, seed, aperture, focus):
    """lens_ref.resolve of the handle's own rt_trace_rays of lens_ref's rays"""
    rays = lens_ref.rays(cam, W, H, 0, W, n, seed, aperture, focus)
    return lens_ref.resolve(r.trace_rays(np.ascontiguousarray(rays.reshape(W, H * n * n, 6)), depth).reshape(W, H, n * n, 3), n)


# ---- 1. ray generation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("camera,seed", [(None, 0), ("pitched_down", 0), ("rolled_1p45", 0xC0FFEE), ("left_handed", 0)])
def test_rays_are_the_definitions_word_for_word(camera, seed, n):
    cam = lens_ref.camera_copy(camera_of(camera))
    want = lens_ref.rays(cam, W61, H37, 0, W61, n, seed, APERTURE, FOCUS)
    got = lens_rays(cam, W61, H37, samples=n, aperture=APERTURE, focus=FOCUS, seed=seed)
    assert_same(got, want, f"rays {camera} n{n}")
    for x0, x1 in STRIPS:
        assert_same(lens_rays(cam, W61, H37, samples=n, aperture=APERTURE, focus=FOCUS, seed=seed, x0=x0, x1=x1), want[x0:x1],
                    f"rays {camera} n{n} strip {x0}:{x1}")
    if n == 3:                                                            # a pinhole: every origin is the eye itself
        pin = lens_rays(cam, W61, H37, samples=n, aperture=0.0, focus=FOCUS, seed=seed)
        assert_same(pin, lens_ref.rays(cam, W61, H37, 0, W61, n, seed, 0.0, FOCUS), f"rays {camera} n{n} aperture 0")


def test_rays_device_entry_into_poisoned_words():
    import ctypes as C
    cam = lens_ref.camera_copy(camera_of("pitched_down"))
    n, x0, x1 = 3, 20, 61
    want = lens_ref.rays(cam, W61, H37, x0, x1, n, 5, APERTURE, FOCUS)
    what = "rt_lens_rays_device 61x37 n3 columns 20:61"
    poisoned.assert_reference_has_no_sentinel(want, what)
    o = poisoned._Outputs([(want.size, 6, ("O.x", "O.y", "O.z", "T.x", "T.y", "T.z"), False)])
    params = capi.RtLensParams(n, 0, 5, APERTURE, FOCUS)
    capi.check(capi.load_library().rt_lens_rays_device(C.byref(cam), W61, H37, x0, x1, C.byref(params), 0, o.ptrs()[0],
                                                       poisoned._stream()))
    got, = o.checked(Renderer(HostScene.builtin()), H37 * n * n, 0, 1, what)
    assert_same(got.view(F).reshape(want.shape), want, what)


W24 = (1 << 24) + 43
W28 = (1 << 28) + 5
WRAP = (1 << 32) // H37                   # the first column whose pixel keys x * H + z pass 2^32


@pytest.mark.parametrize("W,n,x0,x1", [(W24, 3, 0, 8), (W24, 3, W24 - 8, W24), (W28, 2, WRAP - 8, WRAP + 8)],
                         ids=["first-columns", "3x-above-2^24", "key-wraps-2^32"])
def test_rays_of_strips_of_very_wide_frames(W, n, x0, x1):
    """W = 2^24 + 43, n = 3: in the last columns n x + i is above 2^24, where (float) rounds, and must round as lens_ref's
    int -> float32 does.  W = 2^28 + 5, H = 37: around column 2^32 // 37 the pixel key x H + z passes 2^32 and is taken modulo 2^32
    (include/rt_capi_lens.h); the lens is open, so a key computed otherwise moves every origin."""
    cam = lens_ref.camera_copy(camera_of("pitched_down"))
    if W == W24 and x0 > 0:
        assert n * x0 > 1 << 24 and len(np.unique((n * np.arange(x0, x1)[:, None] + np.arange(n)).astype(F))) < n * (x1 - x0)
    if W == W28:
        assert x0 * H37 < 1 << 32 < (x1 - 1) * H37
    want = lens_ref.rays(cam, W, H37, x0, x1, n, 0xC0FFEE, APERTURE, FOCUS)
    got = lens_rays(cam, W, H37, samples=n, aperture=APERTURE, focus=FOCUS, seed=0xC0FFEE, x0=x0, x1=x1)
    assert_same(got, want, f"rays W={W} n{n} columns {x0}:{x1}")
    assert len(np.unique(got[..., :3].reshape(-1, 3), axis=0)) > (x1 - x0) * H37 * n * n // 2       # the lens is open


# ---- 2. frames against the CPU oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,W,H,depth,n,seed,point", lens_ref.FRAMES)
def test_against_the_oracle(key, W, H, depth, n, seed, point):
    aperture, focus = lens_ref.lens_of(key, point)
    want = lens_ref.oracle_frame(key, W, H, depth, n, seed, aperture, focus)
    r = Renderer(adaptive_frames.host_scene(key))
    got = r.render_lens(W, H, depth, samples=n, aperture=aperture, focus=focus, seed=seed)
    assert_same(got, want, f"{key} {W}x{H} d{depth} n{n}")
    info = r.lens_info()
    assert (info.pixels, info.rays, info.chunks) == (W * H, W * H * n * n, 1)
    assert r.launch_info().kernel.decode().endswith("_rays")


def test_against_the_oracle_at_five_by_five():
    """S = 25 is no power of two and no divisor of 1024: a pixel's lanes straddle wavefronts and workgroups in the ray generation,
    and the resolve's workgroups take 40 pixels and leave 24 sample slots over.  The smallest frame of lens_ref.FRAMES."""
    key, W, H, depth, _, seed, point = min(lens_ref.FRAMES, key=lambda f: f[1] * f[2])
    n = 5
    aperture, focus = lens_ref.lens_of(key, point)
    want = lens_ref.oracle_frame(key, W, H, depth, n, seed, aperture, focus)
    r = Renderer(adaptive_frames.host_scene(key))
    got = r.render_lens(W, H, depth, samples=n, aperture=aperture, focus=focus, seed=seed)
    assert_same(got, want, f"{key} {W}x{H} d{depth} n{n}")
    assert (W * H) % (1024 // (n * n)) != 0
    info = r.lens_info()
    assert (info.pixels, info.rays, info.chunks) == (W * H, W * H * n * n, 1)


def test_an_image_textured_scene_against_its_own_ray_batches():
    import texture_ref
    from test_texture_gpu import Desc, image_planes
    host, floor, wall = image_planes(HostScene.empty())
    texels = np.random.RandomState(5).uniform(0, 1, (16, 16, 3)).astype(F)
    d = Desc(host)
    d.objs[floor].texture = 0
    d.objs[wall].texture = 0
    r = d.make(images=[(texels, F(5.0), F(3.5), texture_ref.REPEAT)])
    W, H, depth, n = 45, 34, 3, 3
    want = own_reference(r, d.cam, W, H, depth, n, 3, 0.3, 6.0)
    got = r.render_lens(W, H, depth, samples=n, aperture=0.3, focus=6.0, seed=3)
    assert r.kernel_name() == "rt_render_kernel_rays_image"
    assert_same(got, want, "image planes")
    assert lens_ref.changed_share(got, r.render_lens(W, H, depth, samples=n, aperture=0.0, focus=6.0, seed=3)) >= 0.05


def test_a_refractive_scene_against_its_own_ray_batches():
    from test_refract_gpu import glass_builtin, make
    from test_texture_gpu import Desc
    host = HostScene.builtin()
    refr = glass_builtin(host)
    r = make(Desc(host), refractive=refr)
    W, H, depth, n = 48, 36, 4, 2
    want = own_reference(r, host.camera.contents, W, H, depth, n, 0, APERTURE, FOCUS)
    got = r.render_lens(W, H, depth, samples=n, aperture=APERTURE, focus=FOCUS)
    assert r.kernel_name() == "rt_render_kernel_rays_refract"
    assert_same(got, want, "glass")
    assert lens_ref.changed_share(got, r.render_lens(W, H, depth, samples=n, aperture=0.0, focus=FOCUS)) >= 0.05


# ---- 3. the anchors: a pinhole at the screen's distance is rt_render_ssaa and rt_render -------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("camera", [None, "pitched_down", "rolled_1p45", "left_handed"])
def test_a_pinhole_focused_on_the_screen_is_rt_render_ssaa(camera, n):
    host = camera_of(camera)
    so = np.array(list(host.camera.contents.screen_origin), dtype=F)
    assert not (np.signbit(so) & (so == 0)).any(), so                    # no -0.0: rt_trace_rays would read it as +0.0
    r = Renderer(host)
    depth = 4
    got = r.render_lens(W61, H37, depth, samples=n, aperture=0.0, focus=1.0, seed=99)
    assert_same(got, r.render_ssaa(W61, H37, depth, n), f"pinhole {camera} n{n} against rt_render_ssaa")
    if n == 1:
        assert_same(got, r.render(W61, H37, depth), f"pinhole {camera} against rt_render")


# ---- 4. chunks and strips -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 5, 7])
def test_chunks_and_strips_never_change_a_bit(n):
    r = Renderer(HostScene.builtin())
    depth = 3
    kw = dict(samples=n, aperture=APERTURE, focus=FOCUS, seed=11)
    want = r.render_lens(W61, H37, depth, **kw)
    assert r.lens_info().chunks == 1
    for chunk in (1, 7, 61, 0):
        assert (chunk * H37) % (1024 // (n * n)) != 0 or chunk == 0      # no chunk ends on a seam of the resolve's workgroups
        got = r.render_lens(W61, H37, depth, chunk_columns=chunk, **kw)
        assert_same(got, want, f"n{n} chunk_columns {chunk}")
        info = r.lens_info()
        assert info.chunks == (-(-W61 // chunk) if chunk else 1), (chunk, info.chunks)
        assert (info.pixels, info.rays) == (W61 * H37, W61 * H37 * n * n)
    parts = [r.render_lens(W61, H37, depth, x0=x0, x1=x1, chunk_columns=13, **kw) for x0, x1 in STRIPS]
    assert r.lens_info().pixels == 40 * H37 and r.lens_info().chunks == 4
    assert_same(np.concatenate(parts), want, f"n{n} strips")
    assert r.render_lens(W61, H37, depth, x0=7, x1=7, **kw).shape == (0, H37, 3)      # an empty strip launches nothing


# ---- 5. the device entry point ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,x0,x1,chunk", [(2, 0, 61, 0), (3, 20, 61, 7), (4, 20, 21, 0)])
def test_device_entry_on_a_stream_into_poisoned_outputs(n, x0, x1, chunk):
    """every colour word of the strip is written, nothing before or after it"""
    r = Renderer(HostScene.builtin())
    depth = 3
    kw = dict(samples=n, aperture=APERTURE, focus=FOCUS, seed=4, chunk_columns=chunk)
    want = r.render_lens(W61, H37, depth, x0=x0, x1=x1, **kw)
    what = f"rt_render_lens_device 61x37 n={n} columns {x0}:{x1}"
    poisoned.assert_reference_has_no_sentinel(want, what)
    o = poisoned._Outputs([((x1 - x0) * H37 * 3, 3, poisoned.RGB, False)])
    r.render_lens_device(W61, H37, depth, x0, x1, o.ptrs()[0], poisoned._stream(), **kw)
    rgb, = o.checked(r, H37, x0, 1, what)
    assert_same(rgb.view(F).reshape(x1 - x0, H37, 3), want, what)
    info = r.lens_info()
    stages = (info.raygen_ms, info.trace_ms, info.resolve_ms)
    assert all(t > 0 for t in stages), stages
    assert r.timing().last_kernel_ms == pytest.approx(sum(stages), rel=1e-12)
    assert r.launch_info().kernel.decode().endswith("_rays")
    r.render(W61, H37, depth)                                             # another launch: the timing is that launch's again
    assert r.timing().last_kernel_ms != pytest.approx(sum(stages), rel=1e-12)


def test_argument_errors_that_need_a_scene_and_the_handle_renders_on():
    r = Renderer(HostScene.builtin())
    depth = 3
    want = r.render_lens(W61, H37, depth, samples=2, aperture=APERTURE, focus=FOCUS)
    for kw, word in ((dict(samples=9, x1=W61 + 1), "x0 <= x1"), (dict(samples=9, chunk_columns=-1), "samples"),
                     (dict(chunk_columns=-1, aperture=-1.0), "chunk_columns"), (dict(aperture=float("nan"), focus=0.0), "aperture"),
                     (dict(focus=0.0), "focus")):
        with pytest.raises(RtError) as e:
            r.render_lens(W61, H37, depth, **kw)
        assert e.value.code == capi.RT_ERR_INVALID and word in e.value.message, (kw, e.value.message)
    with pytest.raises(RtError) as e:
        r.render_lens_device(W61, H37, depth, 0, W61, 0x10002, 0)
    assert e.value.code == capi.RT_ERR_INVALID and "4-byte" in e.value.message
    assert_same(r.render_lens(W61, H37, depth, samples=2, aperture=APERTURE, focus=FOCUS), want, "after the refusals")


# ---- 6. other kernels, and the scenes that are refused ---------------------------------------------------------------------------

@pytest.mark.parametrize("options,kernel", [({"tables": 2}, "rt_render_kernel_large_rays"), ({"cull": 0}, "rt_render_kernel_items_rays")])
def test_the_same_bits_through_other_kernels(options, kernel):
    key, W, H, depth, n, seed, point = lens_ref.FRAMES[0]
    aperture, focus = lens_ref.lens_of(key, point)
    r = Renderer(adaptive_frames.host_scene(key))
    want = r.render_lens(W, H, depth, samples=n, aperture=aperture, focus=focus, seed=seed)
    default = r.kernel_name()
    for name, value in options.items():
        r.set_option(name, value)
    got = r.render_lens(W, H, depth, samples=n, aperture=aperture, focus=focus, seed=seed)
    assert r.kernel_name() == kernel != default
    assert_same(got, want, f"{options}")


def test_a_soft_shadow_scene_is_refused_and_the_handle_renders_on():
    import oracle_lib
    from test_soft_gpu import lights_of, make
    from test_texture_gpu import Desc
    area = [(i, 2, 0.6) for i in lights_of(oracle_lib.OracleScene.builtin())]
    r = make(Desc(HostScene.builtin()), area)
    W, H, depth = 40, 32, 2
    before = r.render(W, H, depth)
    for kw in (dict(samples=2, aperture=0.1), dict(samples=1)):
        with pytest.raises(RtError) as e:
            r.render_lens(W, H, depth, **kw)
        assert e.value.code == capi.RT_ERR_INVALID and "area lights" in e.value.message and "chunk_columns" in e.value.message
    assert_same(r.render(W, H, depth), before, "the handle after the refusal")
    hard = make(Desc(HostScene.builtin()), [])                            # rt_scene_create_soft without an area light: accepted
    plain = Renderer(HostScene.builtin())
    kw = dict(samples=2, aperture=APERTURE, focus=FOCUS)
    assert_same(hard.render_lens(W, H, depth, **kw), plain.render_lens(W, H, depth, **kw), "no area light")


def test_render_image_takes_a_lens():
    from tilecoderaytracer_amd import encode_image
    r = Renderer(HostScene.builtin())
    W, H, depth = 48, 36, 3
    lens = dict(aperture=APERTURE, focus=FOCUS, seed=2)
    want = encode_image(r.render_lens(W, H, depth, samples=2, **lens))
    assert np.array_equal(r.render_image(W, H, depth, samples=2, lens=lens), want)
    assert np.array_equal(r.render_image(W, H, depth, lens=dict(samples=2, **lens)), want)
    assert not np.array_equal(r.render_image(W, H, depth, samples=2), want)          # without it: rt_render_ssaa's frame
