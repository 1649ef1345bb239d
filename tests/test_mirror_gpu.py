"""Mirror records (include/rt_mirror.h) on the GPU against their definition: rt_mirror_records and rt_mirror_records_device
against mirror_ref word for word -- terminal records, guide records, weights and path words -- on the built-in scene and the
room of mirror_scenes.py (whose chains test_mirror_cpu.py counts), over bounce limits, both reflectivity floors, chunks, rows,
strips, absent outputs, a non-null stream and sentinel-filled guarded outputs, and the Renderer's composed calls against the
formulae composed from the separate calls.  Bar: BIT-EXACT."""
import ctypes as C

import numpy as np
import pytest

import mirror_ref
import mirror_scenes
import poisoned
import temporal_ref
from tilecoderaytracer_amd import Renderer, capi, temporal_accumulate
from tilecoderaytracer_amd.renderer import HIT_DTYPE, mirror_params

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("hits", "guide", "weight", "path")
W61, H37 = mirror_scenes.SIZES[0]


def assert_same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)
    unit = np.uint8 if got.dtype.itemsize == 1 else np.uint32
    a, b = got.reshape(-1).view(unit), want.reshape(-1).view(unit)
    bad = np.flatnonzero(a != b)
    if len(bad):
        cell = int(bad[0]) * unit().itemsize // got.dtype.itemsize
        raise AssertionError(f"{what}: {len(bad)} words differ, first in cell {cell} of shape {got.shape}: "
                             f"gpu={got.reshape(-1)[cell]} ref={want.reshape(-1)[cell]}")


def assert_all_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert_same(g, w, f"{what}: {name}")


@pytest.fixture(scope="module")
def renderers():
    made = {key: Renderer(mirror_scenes.host_scene(key)) for key in ("builtin", "room")}
    yield made
    for r in made.values():
        r.close()


def rays_of(key, W, H):
    return np.array(mirror_scenes.pixel_rays(key, W, H), dtype=F, order="C")


# ---- 1. every output word against the definition --------------------------------------------------------------------------------

@pytest.mark.parametrize("floor", [1.0, 0.5])
@pytest.mark.parametrize("bounces", [0, 1, 3, 8])
@pytest.mark.parametrize("W,H", mirror_scenes.SIZES)
@pytest.mark.parametrize("key", ["builtin", "room"])
def test_every_output_word_is_the_definitions(renderers, key, W, H, bounces, floor):
    want = mirror_scenes.reference(key, W, H, bounces, floor)
    got = renderers[key].mirror_records(rays_of(key, W, H), bounces, floor)
    assert_all_same(got, want, f"{key} {W}x{H} bounces {bounces} floor {floor}")


def handmade_rays():
    """the room's pixel rays thinned to an odd count, with rays that miss everything (straight up from above either scene) and
    one E == T ray"""
    rays = rays_of("room", W61, H37).reshape(-1, 6)[::7].copy()
    up = np.zeros((39, 6), dtype=F)
    up[:, 0], up[:, 2] = np.arange(39) * F(0.1) - 2, 1000
    up[:, 3:] = up[:, :3] + F([0.0, 0.0, 1.0])
    same = rays[:1].copy()
    same[:, 3:] = same[:, :3]
    out = np.ascontiguousarray(np.concatenate([rays[:100], same, up, rays[100:]]))
    assert len(out) % 2 == 1
    return out


@pytest.mark.parametrize("key", ["builtin", "room"])
def test_a_batch_with_misses_and_a_degenerate_ray(renderers, key):
    rays = handmade_rays()
    want = mirror_ref.records(mirror_scenes.ref_scene(key), rays, 3, 0.5)
    assert (want[0]["object"] < 0).sum() >= 40                                # misses, the E == T ray among them
    assert want[0]["object"][100] == -1 and want[3][100] == 0
    assert_all_same(renderers[key].mirror_records(rays, 3, 0.5), want, f"handmade {key}")


# ---- 2. what never changes a bit ------------------------------------------------------------------------------------------------

def test_chunks_rows_and_strips_never_change_a_bit(renderers):
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    want = mirror_scenes.reference("room", W61, H37, 3, 0.5)[:4]
    n = W61 * H37
    for chunk in (1000, 7, 1):
        sub = {1000: slice(0, None), 7: slice(5, 15), 1: slice(20, 23)}[chunk]   # (few rays a launch: some columns are enough)
        got = r.mirror_records(np.ascontiguousarray(rays[sub]), 3, 0.5, chunk_rays=chunk)
        assert_all_same(got, [w[sub] for w in want], f"chunk_rays {chunk}")
        info = r.mirror_info()
        m = rays[sub].size // 6
        assert (info.rays, info.chunks, info.queries) == (m, -(-m // chunk), -(-m // chunk) * 4), chunk
    for rows in (1, H37, n):
        assert_all_same(r.mirror_records(rays, 3, 0.5, rows=rows), want, f"rows {rows}")
    for x0, x1 in ((0, 23), (23, W61)):                                       # two strips against the frame
        assert_all_same(r.mirror_records(np.ascontiguousarray(rays[x0:x1]), 3, 0.5), [w[x0:x1] for w in want], f"strip {x0}:{x1}")
    info = r.mirror_info()
    assert (info.rays, info.chunks, info.queries) == ((W61 - 23) * H37, 1, 4) and info.query_ms > 0 and info.step_ms > 0
    assert "hits" in r.kernel_name()


def test_each_optional_output_may_be_absent(renderers):
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    want = mirror_scenes.reference("room", W61, H37, 3, 1.0)[:4]
    for absent in Renderer.MIRROR_OUTPUTS + (None,):
        asked = tuple(o for o in Renderer.MIRROR_OUTPUTS if o != absent) if absent else ()
        got = r.mirror_records(rays, 3, 1.0, outputs=asked)
        for name, g, w in zip(NAMES, got, want):
            if name == "hits" or name in asked:
                assert_same(g, w, f"without {absent}: {name}")
            else:
                assert g is None


# ---- 3. the device entry point --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,bounces,floor,chunk", [("room", 3, 0.5, 0), ("room", 2, 1.0, 300), ("builtin", 0, 1.0, 0)])
def test_device_entry_into_poisoned_words_on_a_stream_of_its_own(renderers, key, bounces, floor, chunk):
    import torch
    r = renderers[key]
    rays = rays_of(key, W61, H37)
    n = W61 * H37
    want = mirror_scenes.reference(key, W61, H37, bounces, floor)[:4]
    what = f"rt_mirror_records_device {key} bounces {bounces} chunk {chunk}"
    poisoned.assert_reference_has_no_sentinel([np.ascontiguousarray(w) for w in want], what)
    d_rays = poisoned._on_device(rays)
    o = poisoned._Outputs([(n * 12, 12, poisoned.HIT_FIELDS, False), (n * 12, 12, poisoned.HIT_FIELDS, False),
                           (n * 3, 3, poisoned.RGB, False), (n, 1, ("path",), False)])
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    stream.wait_stream(torch.cuda.current_stream())
    r.mirror_records_device(n, H37, d_rays.data_ptr(), *o.ptrs(), stream=stream.cuda_stream, max_bounces=bounces,
                            min_reflective=floor, chunk_rays=chunk)
    stream.synchronize()
    hits, guide, weight, path = o.checked(r, H37, 0, 1, what)
    got = (hits.view(HIT_DTYPE).reshape(W61, H37), guide.view(HIT_DTYPE).reshape(W61, H37), weight.view(F).reshape(W61, H37, 3),
           path.reshape(W61, H37))
    assert_all_same(got, want, what)
    info = r.mirror_info()
    chunks = -(-n // chunk) if chunk else 1
    assert (info.rays, info.chunks, info.queries) == (n, chunks, chunks * (bounces + 1))


def test_device_entry_refuses_misaligned_outputs_and_the_next_call_is_unharmed(renderers):
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    d_rays = poisoned._on_device(rays)
    lib, p = capi.load_library(), mirror_params(3, 1.0)
    rc = lib.rt_mirror_records_device(r._scene, C.byref(p), 4, 4, d_rays.data_ptr(), d_rays.data_ptr() + 8, None, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "d_out_hits" in lib.rt_last_error().decode()
    assert_all_same(r.mirror_records(rays, 3, 1.0), mirror_scenes.reference("room", W61, H37, 3, 1.0)[:4], "after a refusal")


@pytest.mark.parametrize("n", [2 ** 31 - 1, 2 ** 31 - 64])
def test_a_batch_too_large_for_its_rows_is_refused_and_the_next_call_is_unharmed(renderers, n):
    """the header's check of the batch's size, "ray batch too large for its rows", with rows = 1: the largest int, and 2^31 - 64,
    one cell over rt_trace_rays' grid limit of 0x7fffffff - 64 cells.  The checks precede all device work, so aligned dummy
    addresses are never read.  (The last admitted size, 2^31 - 65 rays, is 51 GB of rays alone and is not launched.)"""
    r = renderers["room"]
    lib, p = capi.load_library(), mirror_params(3, 1.0)
    dummy = 0x10000
    assert n >= (0x7fffffff - 64) + 1 and n * 3.0 <= 8.0e9                    # the cells refuse it, not the floats
    before = r.mirror_info().rays
    rc = lib.rt_mirror_records_device(r._scene, C.byref(p), n, 1, C.c_void_p(dummy), C.c_void_p(dummy), None, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "ray batch too large for its rows" in lib.rt_last_error().decode()
    rc = lib.rt_mirror_records(r._scene, C.byref(p), n, 1, C.c_void_p(dummy), C.c_void_p(dummy), None, None, None)
    assert rc == capi.RT_ERR_INVALID and "ray batch too large for its rows" in lib.rt_last_error().decode()
    assert r.mirror_info().rays == before                                     # (a refused call is not the handle's last call)
    assert_all_same(r.mirror_records(rays_of("room", W61, H37), 3, 1.0), mirror_scenes.reference("room", W61, H37, 3, 1.0)[:4],
                    "after a refusal")


# ---- 4. the composed calls ------------------------------------------------------------------------------------------------------

def test_render_gbuffer_mirrored_is_the_gbuffer_where_no_mirror_is_followed(renderers):
    r = renderers["room"]
    W, H = mirror_scenes.SIZES[1]
    rgb, hits, guide, weight, path = r.render_gbuffer_mirrored(W, H, 3, max_bounces=3, min_reflective=1.0)
    plain_rgb, plain = r.render_gbuffer(W, H, 3)
    assert_same(rgb, plain_rgb, "colours")
    k = mirror_ref.unpack(path)[0]
    assert (k == 0).sum() > 1000 and (k >= 1).sum() > 1000
    assert_same(hits[k == 0], plain[k == 0], "terminal records of the pixels that follow no mirror")
    assert_all_same((hits, guide, weight, path), mirror_scenes.reference("room", W, H, 3, 1.0)[:4], "render_gbuffer_mirrored")
    strip = r.render_gbuffer_mirrored(W, H, 3, max_bounces=3, min_reflective=1.0, x0=17, x1=50)
    assert_all_same(strip[1:], [a[17:50] for a in (hits, guide, weight, path)], "columns 17:50")


def test_render_indirect_and_render_ao_gather_at_the_terminal_records(renderers):
    r = renderers["room"]
    mirrors = dict(max_bounces=3, min_reflective=1.0)
    kw = dict(samples=2, gather_depth=1, gain=1.25, seed=3)
    rgb, hits, _, weight, path = r.render_gbuffer_mirrored(W61, H37, 2, **mirrors)
    term = r.indirect_diffuse(np.ascontiguousarray(hits), **kw)
    assert_same(r.render_indirect(W61, H37, 2, mirrors=mirrors, **kw), rgb + weight * term, "render_indirect(mirrors)")
    seen = (mirror_ref.unpack(path)[0] >= 1) & (term > 0).any(-1)
    assert seen.sum() > 100                                                    # a bounce where the plain call adds nothing
    plain = r.render_indirect(W61, H37, 2, **kw)
    assert (plain[seen] == rgb[seen]).all() and not (plain == rgb).all()
    ao = r.ambient_occlusion(np.ascontiguousarray(hits), 2, radius=1.5, seed=4)
    assert_same(r.render_ao(W61, H37, 2, radius=1.5, seed=4, mirrors=mirrors), ao, "render_ao(mirrors)")
    with pytest.raises(ValueError):
        r.render_indirect(W61, H37, 2, mirrors=mirrors, scale=2)


def test_render_accumulated_with_and_without_mirrors(renderers):
    r = renderers["room"]
    W, H, depth = 45, 38, 2
    cams = list(mirror_scenes.room_cameras())
    kw = dict(max_history=3, plane_eps=0.02)
    mirrors = dict(max_bounces=3, min_reflective=1.0)
    state, state_m, own = None, None, r._cam
    for k, cam in enumerate(cams):
        r._cam = C.pointer(cam)
        rgb, hits = r.render_gbuffer(W, H, depth)
        cur = r.indirect_diffuse(hits, 1, seed=k, base=rgb, gain=1.25)
        out = temporal_accumulate(cur, hits, cam, state, **kw)
        state = (cam, hits, out[0], out[1], out[2])
        rgb, terminal, guide, weight, _ = r.render_gbuffer_mirrored(W, H, depth, **mirrors)
        cur = rgb + weight * r.indirect_diffuse(np.ascontiguousarray(terminal), 1, seed=k, gain=1.25)
        out_m = temporal_accumulate(cur, np.ascontiguousarray(guide), cam, state_m, **kw)
        state_m = (cam, np.ascontiguousarray(guide), out_m[0], out_m[1], out_m[2])
    r._cam = own
    got = r.render_accumulated(cams, W, H, depth, term="indirect", samples=1, mirrors=None, gain=1.25, **kw)
    for name, g, w in zip(("value", "variance", "flags"), got, (out[0], out[3], out[4])):
        assert_same(g.view(np.uint8) if g.dtype == bool else g, w.view(np.uint8) if w.dtype == bool else w, f"mirrors=None: {name}")
    got = r.render_accumulated(cams, W, H, depth, term="indirect", samples=1, mirrors=mirrors, gain=1.25, **kw)
    for name, g, w in zip(("value", "variance", "flags"), got, (out_m[0], out_m[3], out_m[4])):
        assert_same(g.view(np.uint8) if g.dtype == bool else g, w.view(np.uint8) if w.dtype == bool else w, f"mirrors: {name}")
    assert r._cam is own and (~out_m[4]).sum() > 100 and not temporal_ref.dead_records(guide).all()
