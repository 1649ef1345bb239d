"""Glass records (include/rt_glass.h) on the GPU against their definition: rt_glass_records and rt_glass_records_device against
glass_ref word for word -- terminal records, guide records, weights and path words -- on the glass room of glass_scenes.py
(whose chains test_glass_cpu.py counts) and on the room without glass, over bounce limits, both reflectivity floors, glass
looked through and not, chunks, rows, strips, absent outputs, a non-null stream, sentinel-filled guarded outputs and a captured
graph, against rt_mirror_records where nothing is looked through, and the Renderer's composed calls against the formulae
composed from the separate calls; then (section 5) on the scenes "edges" and "open", which run what the glass room never
does: min_transmissive on a tf and one ulp above it, a tf of 0 in the list, glass that is a mirror as well, a candidate without
a child followed as a mirror, planes finite and infinite as glass, an ior of 1, a pane's ior, followed chains that end in a
miss, and the size refusal from a real handle.  Bar: BIT-EXACT."""
import ctypes as C
import itertools

import numpy as np
import pytest

import glass_ref
import glass_scenes
import poisoned
import temporal_ref
from test_refract_gpu import make
from test_texture_gpu import Desc
from tilecoderaytracer_amd import Renderer, capi, temporal_accumulate
from tilecoderaytracer_amd.renderer import HIT_DTYPE, glass_params

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
NAMES = ("hits", "guide", "weight", "path")
W61, H37 = glass_scenes.SIZES[0]


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


def renderer_of(key):
    host, refr = glass_scenes.host_scene(key)
    return make(Desc(host), refractive=refr) if refr else Renderer(host)


@pytest.fixture(scope="module")
def renderers():
    made = {key: renderer_of(key) for key in ("glass", "room", "edges", "open")}
    yield made
    for r in made.values():
        r.close()


def rays_of(key, W, H):
    return np.array(glass_scenes.pixel_rays(key, W, H), dtype=F, order="C")


def device_records(r, rays, stream=None, **kw):
    """rt_glass_records_device of float32 rays (..., 6) on torch's current stream (or `stream`) -> the four outputs, downloaded"""
    import torch
    shape = rays.shape[:-1]
    n = int(np.prod(shape))
    d_rays = poisoned._on_device(rays)
    bufs = [torch.zeros((n * w,), dtype=torch.int32, device="cuda") for w in (12, 12, 3, 1)]
    s = stream if stream is not None else torch.cuda.current_stream()
    s.wait_stream(torch.cuda.current_stream())
    r.glass_records_device(n, shape[-1] if len(shape) > 1 else max(n, 1), d_rays.data_ptr(), *[b.data_ptr() for b in bufs],
                           stream=s.cuda_stream, **kw)
    s.synchronize()
    h, g, w, p = (b.cpu().numpy() for b in bufs)
    return (h.view(HIT_DTYPE).reshape(shape), g.view(HIT_DTYPE).reshape(shape), w.view(F).reshape(shape + (3,)),
            p.view(np.uint32).reshape(shape))


def poisoned_device_records(r, rays, want, what, **kw):
    """rt_glass_records_device of a frame's rays (W, H, 6) on a stream of its own into sentinel-filled, guarded outputs: the
    reference `want` holds no sentinel, the guards are untouched, every needed word was written and no slack word was -> the
    four outputs, downloaded"""
    import torch
    W, H = rays.shape[:2]
    n = W * H
    poisoned.assert_reference_has_no_sentinel([np.ascontiguousarray(w) for w in want], what)
    d_rays = poisoned._on_device(rays)
    o = poisoned._Outputs([(n * 12, 12, poisoned.HIT_FIELDS, False), (n * 12, 12, poisoned.HIT_FIELDS, False),
                           (n * 3, 3, poisoned.RGB, False), (n, 1, ("path",), False)])
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    stream.wait_stream(torch.cuda.current_stream())
    r.glass_records_device(n, H, d_rays.data_ptr(), *o.ptrs(), stream=stream.cuda_stream, **kw)
    stream.synchronize()
    hits, guide, weight, path = o.checked(r, H, 0, 1, what)
    return (hits.view(HIT_DTYPE).reshape(W, H), guide.view(HIT_DTYPE).reshape(W, H), weight.view(F).reshape(W, H, 3),
            path.reshape(W, H))


# ---- 1. every output word against the definition --------------------------------------------------------------------------------

@pytest.mark.parametrize("look", [0.5, INF])
@pytest.mark.parametrize("floor", [1.0, 0.5])
@pytest.mark.parametrize("bounces", [0, 1, 3, 8])
@pytest.mark.parametrize("W,H", glass_scenes.SIZES)
def test_every_output_word_is_the_definitions(renderers, W, H, bounces, floor, look):
    r = renderers["glass"]
    rays = rays_of("glass", W, H)
    want = glass_scenes.reference("glass", W, H, bounces, floor, look)
    what = f"glass {W}x{H} bounces {bounces} floor {floor} look {look}"
    assert_all_same(r.glass_records(rays, bounces, floor, look), want, what + " (host)")
    assert_all_same(device_records(r, rays, max_bounces=bounces, min_reflective=floor, min_transmissive=look), want,
                    what + " (device)")
    if look == INF:                                                           # nothing looked through: the mirror call's words
        assert_all_same(r.glass_records(rays, bounces, floor, look), r.mirror_records(rays, bounces, floor), what + " (mirror)")


@pytest.mark.parametrize("look", [0.5, 0.0, INF])
@pytest.mark.parametrize("bounces,floor", [(0, 1.0), (3, 1.0), (8, 0.5)])
def test_a_scene_without_glass_gives_the_mirror_calls_words(renderers, bounces, floor, look):
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    want = glass_scenes.reference("room", W61, H37, bounces, floor, look)
    got = r.glass_records(rays, bounces, floor, look)
    assert_all_same(got, want, f"room bounces {bounces} floor {floor} look {look}")
    assert_all_same(got, r.mirror_records(rays, bounces, floor), f"room bounces {bounces} floor {floor} look {look} (mirror)")


def handmade_rays():
    """the glass room's pixel rays thinned to an odd count, with rays that miss everything (straight up from above the scene),
    one E == T ray, rays that start inside the glass sphere, and rays from the eye across the bubble's rim: impact parameters
    round 0.375 (0.75 of the radius: total reflection begins) and round the radius 0.5 (the silhouette)"""
    rays = rays_of("glass", W61, H37).reshape(-1, 6)[::7].copy()
    up = np.zeros((39, 6), dtype=F)
    up[:, 0], up[:, 2] = np.arange(39) * F(0.1) - 2, 1000
    up[:, 3:] = up[:, :3] + F([0.0, 0.0, 1.0])
    same = rays[:1].copy()
    same[:, 3:] = same[:, :3]
    rng = np.random.default_rng(5)
    inside = np.zeros((24, 6), dtype=F)
    inside[:, :3] = F([1.0, 3.0, 1.4]) + rng.uniform(-0.3, 0.3, (24, 3)).astype(F)
    inside[:, 3:] = inside[:, :3] + rng.normal(size=(24, 3)).astype(F)
    eye, centre = np.array([0.0, -1.0, 2.5]), np.array([2.2, 4.5, 1.6])
    axis = (centre - eye) / np.linalg.norm(centre - eye)
    u = np.cross(axis, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(axis, u)
    b = np.concatenate([0.375 + np.linspace(-2e-3, 2e-3, 41), 0.5 + np.linspace(-1e-4, 1e-4, 41), 0.5 + np.linspace(-2e-6, 2e-6, 21)])
    phi = np.arange(len(b)) * 2.399963
    rim = np.zeros((len(b), 6), dtype=F)
    rim[:, :3] = eye
    rim[:, 3:] = centre + b[:, None] * (np.cos(phi)[:, None] * u + np.sin(phi)[:, None] * v)
    out = np.ascontiguousarray(np.concatenate([rays[:100], same, up, inside, rim, rays[100:]]))
    return out if len(out) % 2 == 1 else out[:-1]


def test_a_batch_with_misses_a_degenerate_ray_inside_starts_and_the_bubbles_rim(renderers):
    rays = handmade_rays()
    scene = glass_scenes.ref_scene("glass")
    want = glass_ref.records(scene, rays, 3, 0.5, 0.5, details=True)
    d = want[4]
    assert (want[0]["object"] < 0).sum() >= 40                                # misses, the E == T ray among them
    assert want[0]["object"][100] == -1 and want[3][100] == 0
    # the rays that start inside the glass sphere and head towards its centre's side meet it from inside (the others leave it
    # unseen: the reference's sphere test): t < 0, no child, the mirror rule, the terminal
    inside = np.arange(140, 164)
    inside = inside[(want[0]["object"][inside] == glass_scenes.GLASS_SPHERE) & (want[0]["flags"][inside] & 1 == 1)]
    assert len(inside) >= 8 and (want[0]["distance"][inside] < 0).all()
    assert (d["childless"][inside] == 1).all() and (d["k"][inside] == 0).all()
    rim = slice(164, 164 + 103)
    through = d["chain"][rim, 0] == glass_scenes.BUBBLE
    ended = (want[0]["object"][rim] == glass_scenes.BUBBLE) & (d["childless"][rim] >= 1)
    assert through.sum() >= 10 and ended.sum() >= 20 and (want[0]["object"][rim] != glass_scenes.BUBBLE).sum() >= 10
    r = renderers["glass"]
    assert_all_same(r.glass_records(rays, 3, 0.5, 0.5), want[:4], "handmade")
    assert_all_same(device_records(r, rays, max_bounces=3, min_reflective=0.5, min_transmissive=0.5), want[:4], "handmade (device)")


# ---- 2. what never changes a bit ------------------------------------------------------------------------------------------------

def test_chunks_rows_and_strips_never_change_a_bit(renderers):
    r = renderers["glass"]
    rays = rays_of("glass", W61, H37)
    want = glass_scenes.reference("glass", W61, H37, 3, 0.5, 0.5)[:4]
    n = W61 * H37
    for chunk in (1000, 7, 1):
        sub = {1000: slice(0, None), 7: slice(14, 24), 1: slice(20, 23)}[chunk]   # (few rays a launch: some columns are enough)
        got = r.glass_records(np.ascontiguousarray(rays[sub]), 3, 0.5, 0.5, chunk_rays=chunk)
        assert_all_same(got, [w[sub] for w in want], f"chunk_rays {chunk}")
        info = r.glass_info()
        m = rays[sub].size // 6
        assert (info.rays, info.chunks, info.queries) == (m, -(-m // chunk), -(-m // chunk) * 4), chunk
    for rows in (1, H37, n):
        assert_all_same(r.glass_records(rays, 3, 0.5, 0.5, rows=rows), want, f"rows {rows}")
    for x0, x1 in ((0, 23), (23, W61)):                                       # two strips against the frame
        assert_all_same(r.glass_records(np.ascontiguousarray(rays[x0:x1]), 3, 0.5, 0.5), [w[x0:x1] for w in want], f"strip {x0}:{x1}")
    info = r.glass_info()
    assert (info.rays, info.chunks, info.queries) == ((W61 - 23) * H37, 1, 4) and info.query_ms > 0 and info.step_ms > 0
    assert "hits" in r.kernel_name()
    before = r.mirror_info().rays                                             # the mirror call's bookkeeping is its own
    r.glass_records(np.ascontiguousarray(rays[:5]), 1, 1.0, 0.5)
    assert r.mirror_info().rays == before and r.glass_info().rays == 5 * H37


def test_each_subset_of_the_optional_outputs_may_be_absent(renderers):
    r = renderers["glass"]
    rays = rays_of("glass", W61, H37)
    want = glass_scenes.reference("glass", W61, H37, 3, 1.0, 0.5)[:4]
    for size in range(len(Renderer.MIRROR_OUTPUTS) + 1):
        for asked in itertools.combinations(Renderer.MIRROR_OUTPUTS, size):
            got = r.glass_records(rays, 3, 1.0, 0.5, outputs=asked)
            for name, g, w in zip(NAMES, got, want):
                if name == "hits" or name in asked:
                    assert_same(g, w, f"asked {asked}: {name}")
                else:
                    assert g is None


# ---- 3. the device entry point --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,bounces,floor,look,chunk", [("glass", 3, 0.5, 0.5, 0), ("glass", 4, 1.0, 0.5, 300),
                                                          ("glass", 0, 1.0, 0.5, 0), ("room", 2, 1.0, 0.5, 0)])
def test_device_entry_into_poisoned_words_on_a_stream_of_its_own(renderers, key, bounces, floor, look, chunk):
    r = renderers[key]
    n = W61 * H37
    want = glass_scenes.reference(key, W61, H37, bounces, floor, look)[:4]
    what = f"rt_glass_records_device {key} bounces {bounces} chunk {chunk}"
    got = poisoned_device_records(r, rays_of(key, W61, H37), want, what, max_bounces=bounces, min_reflective=floor,
                                  min_transmissive=look, chunk_rays=chunk)
    assert_all_same(got, want, what)
    info = r.glass_info()
    chunks = -(-n // chunk) if chunk else 1
    assert (info.rays, info.chunks, info.queries) == (n, chunks, chunks * (bounces + 1))


def test_device_entry_refuses_bad_arguments_and_the_next_call_is_unharmed(renderers):
    r = renderers["glass"]
    rays = rays_of("glass", W61, H37)
    d_rays = poisoned._on_device(rays)
    lib, p = capi.load_library(), glass_params(3, 1.0, 0.5)
    rc = lib.rt_glass_records_device(r._scene, C.byref(p), 4, 4, d_rays.data_ptr(), d_rays.data_ptr() + 8, None, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "d_out_hits" in lib.rt_last_error().decode()
    p = glass_params(3, 1.0, float("nan"))
    rc = lib.rt_glass_records_device(r._scene, C.byref(p), 4, 4, d_rays.data_ptr(), d_rays.data_ptr(), None, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "min_transmissive" in lib.rt_last_error().decode()
    assert_all_same(r.glass_records(rays, 3, 1.0, 0.5), glass_scenes.reference("glass", W61, H37, 3, 1.0, 0.5)[:4], "after a refusal")


def captured_and_replayed_once(key, want, **kw):
    """the device call on scene `key`'s 61 x 37 pixel rays, eager and then captured on the same side stream and replayed once:
    the replayed words are the eager call's and the definition's (`want`).  The Renderer is this call's own."""
    import torch
    r = renderer_of(key)
    try:
        rays = rays_of(key, W61, H37)
        n = W61 * H37
        d_rays = poisoned._on_device(rays)
        eager = [torch.zeros((n * w,), dtype=torch.int32, device="cuda") for w in (12, 12, 3, 1)]
        replayed = [torch.zeros((n * w,), dtype=torch.int32, device="cuda") for w in (12, 12, 3, 1)]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        r.glass_records_device(n, H37, d_rays.data_ptr(), *[b.data_ptr() for b in eager], stream=side.cuda_stream, **kw)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            r.glass_records_device(n, H37, d_rays.data_ptr(), *[b.data_ptr() for b in replayed],
                                   stream=torch.cuda.current_stream().cuda_stream, **kw)
        torch.cuda.synchronize()
        assert all(int(b.abs().max()) == 0 for b in replayed)                 # captured, not run
        graph.replay()
        torch.cuda.synchronize()
        shapes = ((HIT_DTYPE, (W61, H37)), (HIT_DTYPE, (W61, H37)), (F, (W61, H37, 3)), (np.uint32, (W61, H37)))
        for name, e, g, w, (dtype, shape) in zip(NAMES, eager, replayed, want, shapes):
            assert_same(g.cpu().numpy(), e.cpu().numpy(), f"replayed against eager: {name}")
            assert_same(g.cpu().numpy().view(dtype).reshape(shape), w, f"replayed against the definition: {name}")
        info = r.glass_info()
        del graph
        return info
    finally:
        r.close()


def test_the_device_call_captured_into_a_graph_and_replayed_once_gives_the_eager_words():
    """The call enqueues only: captured on a side stream and replayed once, its words are the eager call's.  The eager call comes
    first, on the same stream, and grows the scratch and uploads the object tables; the capture then allocates nothing.  (Once:
    a captured hit query holds its launch's place in the handle's counter ring.)  The Renderer is this test's own."""
    captured_and_replayed_once("glass", glass_scenes.reference("glass", W61, H37, 3, 1.0, 0.5)[:4], max_bounces=3,
                               min_reflective=1.0, min_transmissive=0.5)


# ---- 4. the composed calls ------------------------------------------------------------------------------------------------------

def test_render_gbuffer_mirrored_looks_through_glass_when_asked(renderers):
    r = renderers["glass"]
    W, H = glass_scenes.SIZES[1]
    rgb, hits, guide, weight, path = r.render_gbuffer_mirrored(W, H, 3, max_bounces=3, min_reflective=1.0, min_transmissive=0.5)
    plain_rgb, plain = r.render_gbuffer(W, H, 3)
    assert_same(rgb, plain_rgb, "colours")
    k, _, g, _ = glass_ref.unpack(path)
    assert (k == 0).sum() > 1000 and g.sum() > 1000
    assert_same(hits[k == 0], plain[k == 0], "terminal records of the pixels that follow nothing")
    assert_all_same((hits, guide, weight, path), glass_scenes.reference("glass", W, H, 3, 1.0, 0.5)[:4], "render_gbuffer_mirrored")
    strip = r.render_gbuffer_mirrored(W, H, 3, max_bounces=3, min_reflective=1.0, x0=17, x1=50, min_transmissive=0.5)
    assert_all_same(strip[1:], [a[17:50] for a in (hits, guide, weight, path)], "columns 17:50")
    default = r.render_gbuffer_mirrored(W, H, 3, max_bounces=3, min_reflective=1.0)        # every default is the mirror call
    assert_all_same(default[1:], r.mirror_records(rays_of("glass", W, H), 3, 1.0), "without the keyword")
    with pytest.raises(ValueError):
        r.render_gbuffer_mirrored(W, H, 3, max_bounces=3, min_transmissive=0.5, compact=True)


def test_render_indirect_and_render_ao_gather_behind_the_glass(renderers):
    r = renderers["glass"]
    mirrors = dict(max_bounces=3, min_reflective=1.0, min_transmissive=0.5)
    kw = dict(samples=2, gather_depth=1, gain=1.25, seed=3)
    rgb, hits, _, weight, path = r.render_gbuffer_mirrored(W61, H37, 2, **mirrors)
    term = r.indirect_diffuse(np.ascontiguousarray(hits), **kw)
    assert_same(r.render_indirect(W61, H37, 2, mirrors=mirrors, **kw), rgb + weight * term, "render_indirect(mirrors)")
    assert (glass_ref.unpack(path)[2] & (term > 0).any(-1)).sum() > 100       # a bounce gathered behind glass
    ao = r.ambient_occlusion(np.ascontiguousarray(hits), 2, radius=1.5, seed=4)
    assert_same(r.render_ao(W61, H37, 2, radius=1.5, seed=4, mirrors=mirrors), ao, "render_ao(mirrors)")
    with pytest.raises(ValueError):
        r.render_indirect(W61, H37, 2, mirrors=dict(mirrors, compact=True), **kw)
    with pytest.raises(ValueError, match="mirrors takes max_bounces, min_reflective and compact"):
        r.render_ao(W61, H37, 2, mirrors=dict(mirrors, min_refractive=0.5))


def test_render_accumulated_steers_the_history_by_the_guide_behind_the_glass(renderers):
    r = renderers["glass"]
    W, H, depth = 45, 38, 2
    cams = list(glass_scenes.room_cameras())
    kw = dict(max_history=3, plane_eps=0.02)
    mirrors = dict(max_bounces=3, min_reflective=1.0, min_transmissive=0.5)
    state, own = None, r._cam
    for k, cam in enumerate(cams):
        r._cam = C.pointer(cam)
        rgb, terminal, guide, weight, _ = r.render_gbuffer_mirrored(W, H, depth, **mirrors)
        cur = rgb + weight * r.indirect_diffuse(np.ascontiguousarray(terminal), 1, seed=k, gain=1.25)
        out = temporal_accumulate(cur, np.ascontiguousarray(guide), cam, state, **kw)
        state = (cam, np.ascontiguousarray(guide), out[0], out[1], out[2])
    r._cam = own
    got = r.render_accumulated(cams, W, H, depth, term="indirect", samples=1, mirrors=mirrors, gain=1.25, **kw)
    for name, g, w in zip(("value", "variance", "flags"), got, (out[0], out[3], out[4])):
        assert_same(g.view(np.uint8) if g.dtype == bool else g, w.view(np.uint8) if w.dtype == bool else w, f"mirrors: {name}")
    assert r._cam is own and (~out[4]).sum() > 100 and not temporal_ref.dead_records(guide).all()


# ---- 5. the rule's edges: scenes "edges" and "open" of glass_scenes.py, whose categories test_glass_cpu.py counts ----------------

def edges_both_ways(r, bounces, floor, look):
    rays = rays_of("edges", W61, H37)
    want = glass_scenes.reference("edges", W61, H37, bounces, floor, look)
    what = f"edges bounces {bounces} floor {floor} look {look!r}"
    assert_all_same(r.glass_records(rays, bounces, floor, look), want, what + " (host)")
    assert_all_same(device_records(r, rays, max_bounces=bounces, min_reflective=floor, min_transmissive=look), want,
                    what + " (device)")


@pytest.mark.parametrize("floor", glass_scenes.EDGES_FLOORS)
def test_edges_over_the_floors_and_min_transmissive_on_every_threshold_and_one_ulp_above(renderers, floor):
    """tf >= min_transmissive at equality and one ulp above, tf > 0 under min_transmissive <= 0, several tf in one scene, glass
    that is a mirror as well, a finite and an infinite plane as glass, an ior of 1: every word, host and device"""
    for look in glass_scenes.EDGES_LOOKS:
        edges_both_ways(renderers["edges"], 4, floor, look)


@pytest.mark.parametrize("floor,look", [(0.05, 0.3), (1.0, -INF)])
@pytest.mark.parametrize("bounces", [0, 8])
def test_edges_at_no_bounce_and_at_eight(renderers, bounces, floor, look):
    edges_both_ways(renderers["edges"], bounces, floor, look)


def test_edges_the_rim_of_a_bubble_that_is_a_mirror_is_followed_and_so_are_inside_starts(renderers):
    """handmade_rays() on "edges": a candidate without a child falls to the mirror rule, which now follows -- across the bubble's
    rim (rf 1) and from inside the glass sphere (t < 0; rf 0.7 against a floor of 0.5) -- in the lane that ran the child"""
    rays = handmade_rays()
    scene = glass_scenes.ref_scene("edges")
    want = glass_ref.records(scene, rays, 3, 0.5, 0.2, details=True)
    d = want[4]
    inside, rim = slice(140, 164), slice(164, 164 + 103)
    fell = lambda o, part: ((d["chain"][part] == o) & ~d["glass"][part]).any(-1) & (d["childless"][part] >= 1)
    counts = int(fell(glass_scenes.BUBBLE, rim).sum()), int(fell(glass_scenes.GLASS_SPHERE, inside).sum())
    through = int(((d["chain"][rim] == glass_scenes.BUBBLE) & d["glass"][rim]).any(-1).sum())
    assert counts[0] >= 20 and counts[1] >= 8 and through >= 10, (counts, through)
    r = renderers["edges"]
    assert_all_same(r.glass_records(rays, 3, 0.5, 0.2), want[:4], "edges, handmade")
    assert_all_same(device_records(r, rays, max_bounces=3, min_reflective=0.5, min_transmissive=0.2), want[:4],
                    "edges, handmade (device)")
    got = r.glass_records(rays, 3, 0.5, 0.2, outputs=("path",))               # GUIDE = false on both branches
    assert_same(got[0], want[0], "edges, handmade, hits and path only: hits")
    assert_same(got[3], want[3], "edges, handmade, hits and path only: path")


def test_edges_in_chunks_of_seven_rays_and_with_hits_and_path_only(renderers):
    """a slice whose rays take the both-qualify branch and the fall-to-mirror branch, walked seven rays a launch, and the frame
    with hits and path alone: the GUIDE = false instantiations of the step"""
    r = renderers["edges"]
    rays = rays_of("edges", W61, H37)
    want = glass_scenes.reference("edges", W61, H37, 4, 0.5, 0.3)
    d = want[4]
    fell = ((d["chain"] >= 0) & ~d["glass"] & np.isin(d["chain"], (glass_scenes.BUBBLE, glass_scenes.GLASS_SPHERE))).any(-1)
    fell &= d["childless"] >= 1
    x = int(np.flatnonzero(fell.any(1))[0])
    sub = slice(max(x - 1, 0), max(x - 1, 0) + 3)                             # three columns, 111 rays, 16 launches a bounce
    both = (d["glass"] & np.isin(d["chain"], (glass_scenes.GLASS_SPHERE, glass_scenes.FAR_MIRROR, glass_scenes.FLOOR))).any(-1)
    assert fell[sub].sum() >= 1 and both[sub].sum() >= 10
    for asked in (Renderer.MIRROR_OUTPUTS, ("path",)):
        got = r.glass_records(np.ascontiguousarray(rays[sub]), 4, 0.5, 0.3, chunk_rays=7, outputs=asked)
        for name, g, w in zip(NAMES, got, want):
            if name == "hits" or name in asked:
                assert_same(g, w[sub], f"edges chunk_rays 7 asked {asked}: {name}")
        m = 3 * H37
        info = r.glass_info()
        assert (info.rays, info.chunks, info.queries) == (m, -(-m // 7), -(-m // 7) * 5)
    got = r.glass_records(rays, 4, 0.5, 0.3, outputs=("path",))
    assert got[1] is None and got[2] is None
    assert_same(got[0], want[0], "edges, hits and path only: hits")
    assert_same(got[3], want[3], "edges, hits and path only: path")


@pytest.mark.parametrize("ior", [2.0, 0.5])
def test_a_panes_ior_is_never_read(renderers, ior):
    """"ior is read for spheres only": the glass room with its pane's ior changed gives the words of ior 1"""
    host, refr = glass_scenes.host_scene("glass")
    refr = [(o, tf, ior if o == glass_scenes.PANE else i) for o, tf, i in refr]
    assert sum(1 for o, _, i in refr if o == glass_scenes.PANE and i == ior) == 1
    rays = rays_of("glass", W61, H37)
    want = glass_scenes.reference("glass", W61, H37, 4, 1.0, 0.5)
    assert ((want[4]["chain"] == glass_scenes.PANE) & want[4]["glass"]).any(-1).sum() >= 400
    r = make(Desc(host), refractive=refr)
    try:
        got = r.glass_records(rays, 4, 1.0, 0.5)
        assert_all_same(got, want, f"pane ior {ior}")
        assert_all_same(got, renderers["glass"].glass_records(rays, 4, 1.0, 0.5), f"pane ior {ior} against ior 1 on the GPU")
        assert_all_same(device_records(r, rays, max_bounces=4, min_reflective=1.0, min_transmissive=0.5), want,
                        f"pane ior {ior} (device)")
    finally:
        r.close()


@pytest.mark.parametrize("bounces", [1, 3])
def test_open_chains_that_followed_something_and_end_in_a_miss(renderers, bounces):
    """object < 0 with k >= 1: the guide is the record itself, L is not advanced, the weight and the tag are carried"""
    r = renderers["open"]
    rays = rays_of("open", W61, H37)
    want = glass_scenes.reference("open", W61, H37, bounces, 1.0, 0.5)
    k, _, g, _ = glass_ref.unpack(want[3])
    miss = (k >= 1) & (want[0]["object"] < 0)
    assert miss.sum() >= 400 and (miss & g).sum() >= 300
    what = f"open bounces {bounces}"
    assert_all_same(r.glass_records(rays, bounces, 1.0, 0.5), want, what + " (host)")
    assert_all_same(device_records(r, rays, max_bounces=bounces, min_reflective=1.0, min_transmissive=0.5), want, what + " (device)")
    got = poisoned_device_records(r, rays, want[:4], what + " (device, poisoned)", max_bounces=bounces, min_reflective=1.0,
                                  min_transmissive=0.5)
    assert_all_same(got, want, what + " (device, poisoned)")
    assert_all_same(r.glass_records(rays, bounces, 1.0, 0.5, chunk_rays=1000, outputs=("path",))[::3], want[:4:3], what + " (no guide)")


def test_edges_captured_in_three_chunks_and_replayed_once_gives_the_eager_words():
    """test_the_device_call_captured_into_a_graph_and_replayed_once_gives_the_eager_words on "edges", the chunk loop captured:
    three chunks of 1000 rays, glass that is a mirror and the fall to the mirror rule among them.  Once, for that test's reason."""
    want = glass_scenes.reference("edges", W61, H37, 4, 0.05, 0.3)[:4]
    info = captured_and_replayed_once("edges", want, max_bounces=4, min_reflective=0.05, min_transmissive=0.3, chunk_rays=1000)
    assert (info.rays, info.chunks, info.queries) == (W61 * H37, 3, 15)


@pytest.mark.parametrize("n", [2 ** 31 - 1, 2 ** 31 - 64])
def test_a_batch_too_large_for_its_rows_is_refused_and_the_next_call_is_unharmed(renderers, n):
    """the header's check (9), "ray batch too large for its rows", with rows = 1, from a real handle: the largest int, and
    2^31 - 64, one cell over rt_trace_rays' grid limit of 0x7fffffff - 64 cells.  The checks precede all device work, so aligned
    dummy addresses are never read, and nothing is launched."""
    r = renderers["glass"]
    lib, p = capi.load_library(), glass_params(3, 1.0, 0.5)
    dummy = 0x10000
    assert n >= (0x7fffffff - 64) + 1 and n * 3.0 <= 8.0e9                    # the cells refuse it, not the floats
    r.glass_records(np.ascontiguousarray(rays_of("glass", W61, H37)[:5]), 1, 1.0, 0.5)
    before = r.glass_info().rays
    assert before == 5 * H37
    rc = lib.rt_glass_records_device(r._scene, C.byref(p), n, 1, C.c_void_p(dummy), C.c_void_p(dummy), None, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "ray batch too large for its rows" in lib.rt_last_error().decode()
    rc = lib.rt_glass_records(r._scene, C.byref(p), n, 1, C.c_void_p(dummy), C.c_void_p(dummy), None, None, None)
    assert rc == capi.RT_ERR_INVALID and "ray batch too large for its rows" in lib.rt_last_error().decode()
    assert r.glass_info().rays == before                                      # (a refused call is not the handle's last call)
    assert_all_same(r.glass_records(rays_of("glass", W61, H37), 3, 1.0, 0.5), glass_scenes.reference("glass", W61, H37, 3, 1.0, 0.5)[:4],
                    "after a refusal")
