"""Compact mirror records (include/rt_mirror_compact.h) on the GPU: rt_mirror_records_compact and its device entry against
mirror_ref word for word AND against rt_mirror_records of the same handle -- the header adds no definition --, and the info
struct's counts (alive, rays_queried, queries, syncs, chunks) against the numbers the reference's path words give: over bounce
limits up to 64, both reflectivity floors, lists whose sizes sit at the edges of a wavefront and a workgroup, more live rays than
one step of the scan covers (kScanBlock * 256 = 262 144, the constants of csrc/rt_scan.h), chunks, rows, strips, absent
outputs, a non-null stream into sentinel-filled guarded outputs, the Renderer's composed calls, the refusal of a batch too large
for its rows, and the unit's scan on its own (rt_internal_mirror_compact_scan) up to three trips of its second level, which no
batch that fits a device reaches through the call.  Bar: BIT-EXACT."""
import ctypes as C

import numpy as np
import pytest

import large_extents as le
import mirror_ref
import mirror_scenes
import poisoned
from mirror_large import expected_info
from tilecoderaytracer_amd import Renderer, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE, mirror_params

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = ("hits", "guide", "weight", "path")
W61, H37 = mirror_scenes.SIZES[0]
W96, H80 = mirror_scenes.SIZES[1]


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


def info_of(r):
    i = r.mirror_compact_info()
    assert i.reserved == 0 and i.query_ms > 0 and (i.step_ms > 0 or i.rays == 0)
    return i.rays, i.rays_queried, i.chunks, i.queries, i.syncs, list(i.alive)


# ---- 1. every output word is the definition's, and rt_mirror_records' ---------------------------------------------------------

@pytest.mark.parametrize("floor", [1.0, 0.5])
@pytest.mark.parametrize("bounces", [0, 1, 3, 8, 64])
@pytest.mark.parametrize("W,H", mirror_scenes.SIZES)
@pytest.mark.parametrize("key", ["builtin", "room"])
def test_every_output_word_is_the_definitions_and_rt_mirror_records(renderers, key, W, H, bounces, floor):
    what = f"{key} {W}x{H} bounces {bounces} floor {floor}"
    want = mirror_scenes.reference(key, W, H, bounces, floor)
    rays = rays_of(key, W, H)
    got = renderers[key].mirror_records(rays, bounces, floor, compact=True)
    assert_all_same(got, want, what)
    assert info_of(renderers[key]) == expected_info(want[3], bounces), what
    assert_all_same(got, renderers[key].mirror_records(rays, bounces, floor), what + " against rt_mirror_records")


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
    return out, up


@pytest.mark.parametrize("key", ["builtin", "room"])
def test_a_batch_with_misses_and_a_degenerate_ray(renderers, key):
    rays, _ = handmade_rays()
    want = mirror_ref.records(mirror_scenes.ref_scene(key), rays, 3, 0.5)
    assert (want[0]["object"] < 0).sum() >= 40                                # misses, the E == T ray among them
    assert want[0]["object"][100] == -1 and want[3][100] == 0
    assert_all_same(renderers[key].mirror_records(rays, 3, 0.5, compact=True), want, f"handmade {key}")
    assert info_of(renderers[key]) == expected_info(want[3], 3)


# ---- 2. the info struct -------------------------------------------------------------------------------------------------------

def test_queries_and_syncs_at_the_ends_of_the_bounce_range(renderers):
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    n = W61 * H37
    r.mirror_records(rays, 0, 0.5, compact=True)                              # no bounce: one query and nothing to wait for
    assert info_of(r) == (n, n, 1, 1, 0, [n] + [0] * 64)
    for key, floor, first_empty in (("room", 0.5, 15), ("builtin", 1.0, 3)):  # (test_mirror_compact_cpu.py holds these)
        renderers[key].mirror_records(rays_of(key, W61, H37), 64, floor, compact=True)
        rays_, queried, chunks, queries, syncs, alive = info_of(renderers[key])
        assert (queries, syncs, chunks) == (first_empty, first_empty, 1) and queries < 65
        assert alive[first_empty - 1] > 0 and alive[first_empty:] == [0] * (65 - first_empty) and queried == sum(alive)
    _, up = handmade_rays()                                                   # every ray misses: the chunk ends after one query
    hits, _, weight, path = r.mirror_records(up, 8, 0.5, compact=True)
    assert (hits["object"] == -1).all() and (path == 0).all() and (weight == 1).all()
    assert info_of(r) == (39, 39, 1, 1, 1, [39] + [0] * 64)


def test_the_two_calls_infos_do_not_touch_each_other(renderers):
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    as_bytes = lambda info: bytes(memoryview(info))
    r.mirror_records(rays[:30], 2, 1.0)
    before = as_bytes(r.mirror_info())
    assert r.mirror_info().rays == 30 * H37
    r.mirror_records(rays, 5, 0.5, compact=True)
    assert as_bytes(r.mirror_info()) == before
    mine = as_bytes(r.mirror_compact_info())
    assert r.mirror_compact_info().rays == W61 * H37 and "hits" in r.kernel_name()
    r.mirror_records(rays[:11], 1, 1.0)
    assert as_bytes(r.mirror_compact_info()) == mine and r.mirror_info().rays == 11 * H37


# ---- 3. list sizes at the edges of a wavefront and a workgroup ------------------------------------------------------------------

def interleave(few, many):
    """the indices `few` spread evenly among the indices `many`, both kept in their order"""
    out = list(many)
    for j, i in enumerate(few):
        out.insert((j * (len(many) + 1)) // max(len(few), 1) + j, i)
    return np.array(out, dtype=np.int64)


@pytest.fixture(scope="module")
def room_chains():
    """the room's 96 x 80 rays at floor 0.5, flat, their reference, and the indices of the rays with k = 0, k = 1, k >= 2"""
    want = [np.asarray(a).reshape((W96 * H80,) + np.asarray(a).shape[2:]) for a in mirror_scenes.reference("room", W96, H80, 8, 0.5)[:4]]
    k = mirror_ref.unpack(want[3])[0]
    groups = [np.flatnonzero(k == 0), np.flatnonzero(k == 1), np.flatnonzero(k >= 2)]
    assert [len(g) for g in groups] == [3938, 2321, 1421]
    return rays_of("room", W96, H80).reshape(-1, 6), want, groups


@pytest.mark.parametrize("c", [0, 1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("bounce", [1, 2])
def test_list_sizes_at_the_edges_of_a_wavefront_and_a_workgroup(renderers, room_chains, bounce, c):
    """c rays whose chain reaches query `bounce` among 300 whose chain ends one query sooner: the list of that bounce has
    exactly c entries"""
    rays, want, (k0, k1, k2) = room_chains
    go_on, end = (np.concatenate([k1, k2]), k0) if bounce == 1 else (k2, k1)
    pick = interleave(go_on[:: len(go_on) // 257][:c], end[:: len(end) // 300][:300])
    assert len(pick) == 300 + c and len(set(pick.tolist())) == 300 + c
    got = renderers["room"].mirror_records(np.ascontiguousarray(rays[pick]), 8, 0.5, compact=True)
    assert_all_same(got, [w[pick] for w in want], f"{c} live rays at bounce {bounce}")
    info = info_of(renderers["room"])
    assert info == expected_info(want[3][pick], 8) and info[5][bounce] == c and info[5][bounce - 1] == 300 + c


def test_a_batch_in_which_every_ray_is_alive_after_bounce_0(renderers, room_chains):
    rays, want, (_, k1, k2) = room_chains
    pick = np.sort(np.concatenate([k1, k2]))
    got = renderers["room"].mirror_records(np.ascontiguousarray(rays[pick]), 8, 0.5, compact=True)
    assert_all_same(got, [w[pick] for w in want], "every ray alive after bounce 0")
    info = info_of(renderers["room"])
    assert info == expected_info(want[3][pick], 8) and info[5][0] == info[5][1] == len(pick) == 3742


# ---- 4. more live rays than one step of the scan covers -------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [0, 100000])
def test_more_rays_than_one_step_of_the_scan_covers(renderers, chunk):
    """523 x 509 = 266 207 rays are 1040 workgroups' counts: two groups of the scan's first level (kScanBlock 1024, 256 rays a
    workgroup: the constants of csrc/rt_scan.h are rt_adaptive.hip's).  As one chunk, and as three."""
    W, H, n = 523, 509, 523 * 509
    assert n > 1024 * 256
    want = mirror_scenes.reference("room", W, H, 8, 0.5)
    got = renderers["room"].mirror_records(rays_of("room", W, H), 8, 0.5, chunk_rays=chunk, compact=True)
    assert_all_same(got, want, f"{W}x{H} chunk_rays {chunk}")
    info = info_of(renderers["room"])
    assert info == expected_info(want[3], 8, chunk) and info[2] == (3 if chunk else 1)


# ---- 5. what never changes a bit ------------------------------------------------------------------------------------------------

def test_chunks_rows_and_strips_never_change_a_bit(renderers):
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    want = mirror_scenes.reference("room", W61, H37, 3, 0.5)[:4]
    n = W61 * H37
    for chunk in (1000, 7, 1):
        sub = {1000: slice(0, None), 7: slice(5, 15), 1: slice(20, 23)}[chunk]   # (few rays a launch: some columns are enough)
        got = r.mirror_records(np.ascontiguousarray(rays[sub]), 3, 0.5, chunk_rays=chunk, compact=True)
        assert_all_same(got, [w[sub] for w in want], f"chunk_rays {chunk}")
        assert info_of(r) == expected_info(want[3][sub], 3, chunk), chunk      # alive and queries summed per chunk
    for rows in (1, H37, n):
        assert_all_same(r.mirror_records(rays, 3, 0.5, rows=rows, compact=True), want, f"rows {rows}")
    for x0, x1 in ((0, 23), (23, W61)):                                       # two strips against the frame
        got = r.mirror_records(np.ascontiguousarray(rays[x0:x1]), 3, 0.5, compact=True)
        assert_all_same(got, [w[x0:x1] for w in want], f"strip {x0}:{x1}")
        assert info_of(r) == expected_info(want[3][x0:x1], 3)


def test_each_optional_output_may_be_absent(renderers):
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    want = mirror_scenes.reference("room", W61, H37, 3, 1.0)[:4]
    for absent in Renderer.MIRROR_OUTPUTS + (None,):
        asked = tuple(o for o in Renderer.MIRROR_OUTPUTS if o != absent) if absent else ()
        got = r.mirror_records(rays, 3, 1.0, outputs=asked, compact=True)
        for name, g, w in zip(NAMES, got, want):
            if name == "hits" or name in asked:
                assert_same(g, w, f"without {absent}: {name}")
            else:
                assert g is None
        assert info_of(r) == expected_info(want[3], 3)


# ---- 6. the device entry point --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,bounces,floor,chunk", [("room", 8, 0.5, 0), ("room", 2, 1.0, 300), ("builtin", 0, 1.0, 0)])
def test_device_entry_into_poisoned_words_on_a_stream_of_its_own(renderers, key, bounces, floor, chunk):
    """every output word is written -- exactly once, by the step that ends its ray: no later step can mend a sentinel -- and
    no guard word is touched"""
    import torch
    r = renderers[key]
    rays = rays_of(key, W61, H37)
    n = W61 * H37
    want = mirror_scenes.reference(key, W61, H37, bounces, floor)[:4]
    what = f"rt_mirror_records_compact_device {key} bounces {bounces} chunk {chunk}"
    poisoned.assert_reference_has_no_sentinel([np.ascontiguousarray(w) for w in want], what)
    d_rays = poisoned._on_device(rays)
    o = poisoned._Outputs([(n * 12, 12, poisoned.HIT_FIELDS, False), (n * 12, 12, poisoned.HIT_FIELDS, False),
                           (n * 3, 3, poisoned.RGB, False), (n, 1, ("path",), False)])
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    stream.wait_stream(torch.cuda.current_stream())
    r.mirror_records_device(n, H37, d_rays.data_ptr(), *o.ptrs(), stream=stream.cuda_stream, max_bounces=bounces,
                            min_reflective=floor, chunk_rays=chunk, compact=True)
    stream.synchronize()                                                      # (the call returns with its last step enqueued)
    hits, guide, weight, path = o.checked(r, H37, 0, 1, what)
    got = (hits.view(HIT_DTYPE).reshape(W61, H37), guide.view(HIT_DTYPE).reshape(W61, H37), weight.view(F).reshape(W61, H37, 3),
           path.reshape(W61, H37))
    assert_all_same(got, want, what)
    assert info_of(r) == expected_info(want[3], bounces, chunk)


def test_device_entry_refuses_misaligned_outputs_and_the_next_call_is_unharmed(renderers):
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    d_rays = poisoned._on_device(rays)
    lib, p = capi.load_library(), mirror_params(3, 1.0)
    rc = lib.rt_mirror_records_compact_device(r._scene, C.byref(p), 4, 4, d_rays.data_ptr(), d_rays.data_ptr() + 8, None, None, None,
                                              None)
    assert rc == capi.RT_ERR_INVALID and "d_out_hits" in lib.rt_last_error().decode()
    rc = lib.rt_mirror_records_compact_device(r._scene, C.byref(p), 4, 4, d_rays.data_ptr(), d_rays.data_ptr(),
                                              d_rays.data_ptr() + 4, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "d_out_guide" in lib.rt_last_error().decode()
    want = mirror_scenes.reference("room", W61, H37, 3, 1.0)[:4]
    assert_all_same(r.mirror_records(rays, 3, 1.0, compact=True), want, "after a refusal")


# ---- 7. the Renderer's composed calls -------------------------------------------------------------------------------------------

def test_render_gbuffer_mirrored_compact_is_the_default_call_bit_for_bit(renderers):
    r = renderers["room"]
    plain = r.render_gbuffer_mirrored(W96, H80, 3, max_bounces=3, min_reflective=1.0)
    compact = r.render_gbuffer_mirrored(W96, H80, 3, max_bounces=3, min_reflective=1.0, compact=True)
    for name, g, w in zip(("rgb",) + NAMES, compact, plain):
        assert_same(g, w, f"render_gbuffer_mirrored(compact=True): {name}")
    assert_all_same(compact[1:], mirror_scenes.reference("room", W96, H80, 3, 1.0)[:4], "render_gbuffer_mirrored(compact=True)")
    assert info_of(r) == expected_info(plain[4], 3)
    strip = r.render_gbuffer_mirrored(W96, H80, 3, max_bounces=3, min_reflective=1.0, x0=17, x1=50, compact=True)
    assert_all_same(strip[1:], [a[17:50] for a in plain[1:]], "columns 17:50")


def test_mirrors_compact_through_the_composed_renders(renderers):
    r = renderers["room"]
    mirrors = dict(max_bounces=3, min_reflective=1.0)
    compact = dict(mirrors, compact=True)
    kw = dict(samples=2, gather_depth=1, gain=1.25, seed=3)
    assert_same(r.render_indirect(W61, H37, 2, mirrors=compact, **kw), r.render_indirect(W61, H37, 2, mirrors=mirrors, **kw),
                "render_indirect")
    assert r.mirror_compact_info().rays == W61 * H37
    assert_same(r.render_ao(W61, H37, 2, radius=1.5, seed=4, mirrors=compact), r.render_ao(W61, H37, 2, radius=1.5, seed=4, mirrors=mirrors),
                "render_ao")
    cams = list(mirror_scenes.room_cameras())
    acc = dict(term="indirect", samples=1, gain=1.25, max_history=3, plane_eps=0.02)
    want = r.render_accumulated(cams, 45, 38, 2, mirrors=mirrors, **acc)
    got = r.render_accumulated(cams, 45, 38, 2, mirrors=compact, **acc)
    for name, g, w in zip(("value", "variance", "flags"), got, want):
        assert_same(g.view(np.uint8) if g.dtype == bool else g, w.view(np.uint8) if w.dtype == bool else w, f"render_accumulated: {name}")
    assert r.mirror_compact_info().rays == 45 * 38
    with pytest.raises(ValueError):
        r.render_indirect(W61, H37, 2, mirrors=dict(mirrors, compacted=True), **kw)


# ---- 8. the size refusal ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2 ** 31 - 1, 2 ** 31 - 64])
def test_a_batch_too_large_for_its_rows_is_refused_and_the_next_call_is_unharmed(renderers, n):
    """rt_mirror.h's check (9)/(10) of the batch's size, "ray batch too large for its rows", with rows = 1: the largest int, and
    2^31 - 64, one cell over rt_trace_rays' grid limit of 0x7fffffff - 64 cells.  The checks precede all device work, so aligned
    dummy addresses are never read.  (The last admitted size, 2^31 - 65 rays, is 51 GB of rays alone and is not launched.)"""
    r = renderers["room"]
    rays = rays_of("room", W61, H37)
    lib, p = capi.load_library(), mirror_params(3, 1.0)
    dummy = 0x10000
    assert n >= (0x7fffffff - 64) + 1 and n * 3.0 <= 8.0e9                    # the cells refuse it, not the floats
    rc = lib.rt_mirror_records_compact_device(r._scene, C.byref(p), n, 1, C.c_void_p(dummy), C.c_void_p(dummy), None, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "ray batch too large for its rows" in lib.rt_last_error().decode()
    rc = lib.rt_mirror_records_compact(r._scene, C.byref(p), n, 1, C.c_void_p(dummy), C.c_void_p(dummy), None, None, None)
    assert rc == capi.RT_ERR_INVALID and "ray batch too large for its rows" in lib.rt_last_error().decode()
    want = mirror_scenes.reference("room", W61, H37, 3, 1.0)[:4]
    assert_all_same(r.mirror_records(rays, 3, 1.0, compact=True), want, "after a refusal")
    assert info_of(r) == expected_info(want[3], 3)


# ---- 9. the scan on its own, past what a batch that fits a device gives it -------------------------------------------------------

SCAN_GROUP = 1024                                                             # kScanBlock of csrc/rt_scan.h
SCAN_MOST = 256                                                               # kRankBlock: the most a workgroup can report
SCAN_SIZES = [1, 63, 64, 1023, 1024, 1025, 1024 ** 2 - 1, 1024 ** 2, 1024 ** 2 + 1, 2 * 1024 ** 2 + 1537]


def scan_counts(n, pattern):
    if pattern == "all 256":
        return np.full(n, SCAN_MOST, dtype=np.uint32)
    if pattern == "a single 1 at the end":
        c = np.zeros(n, dtype=np.uint32)
        c[-1] = 1
        return c
    assert pattern == "random with runs"
    rng = np.random.default_rng(n)
    c = rng.integers(0, SCAN_MOST + 1, size=n).astype(np.uint32)
    for value in (0, SCAN_MOST) * 6:                                          # runs longer than a group, so that whole groups sum
        start = int(rng.integers(0, n))                                       # to 0 and to 1024 x 256, and shorter ones
        c[start:start + int(rng.integers(1, 3 * SCAN_GROUP + 2))] = value
    return c


@pytest.mark.parametrize("pattern", ["all 256", "random with runs", "a single 1 at the end"])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_the_scan_on_its_own_up_to_three_trips_of_its_second_level(n, pattern):
    """rt_internal_mirror_compact_scan (csrc/rt_internal.h) -- the function rt_mirror_records_compact enqueues its scan through --
    against numpy in uint64.  More than 1024 groups (n > 1024^2 counts, more than 2^28 live rays of one chunk) take
    rt_scan_total_kernel round its loop again: the carried base, the barrier that guards wave_sum between the trips, and
    group_base past entry 1023, which no batch within a test's 48 GB reaches through the call.  Every output lies in a guarded,
    sentinel-filled buffer of exactly its words; no sum here reaches the sentinel's value (the largest is 2^29 + 393 472)."""
    import torch
    lib = capi.load_library()
    scan = lib.rt_internal_mirror_compact_scan
    scan.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
    scan.restype = C.c_int
    groups = -(-n // SCAN_GROUP)
    counts = scan_counts(n, pattern)
    assert counts.max() <= SCAN_MOST and len(counts) == n
    c64 = counts.astype(np.uint64)
    assert int(c64.sum()) <= 2 ** 29 + 393472 < le.SENTINEL
    padded = np.zeros(groups * SCAN_GROUP, dtype=np.uint64)
    padded[:n] = c64
    in_group = padded.reshape(groups, SCAN_GROUP)
    want_offsets = (np.cumsum(in_group, axis=1) - in_group).reshape(-1)[:n]
    want_sums = in_group.sum(axis=1)
    want_base = np.cumsum(want_sums) - want_sums
    before_all = np.cumsum(c64) - c64                                         # the global exclusive sum
    d_counts = torch.from_numpy(counts.view(np.int32)).cuda()
    outs = [le.Guarded(n), le.Guarded(groups), le.Guarded(groups), le.Guarded(1)]
    try:
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        capi.check(scan(d_counts.data_ptr(), n, *[o.ptr for o in outs], stream.cuda_stream))
        stream.synchronize()
        what = f"the scan of {n} counts, {pattern}"
        for o, name in zip(outs, ("offsets", "group_sums", "group_base", "total")):
            o.assert_written(f"{what}: {name}")
        offsets, sums, base, total = (o.body.cpu().numpy().view(np.uint32).astype(np.uint64) for o in outs)
        assert np.array_equal(d_counts.cpu().numpy().view(np.uint32), counts), f"{what}: the counts changed"
        for name, got, want in (("offsets", offsets, want_offsets), ("group_sums", sums, want_sums), ("group_base", base, want_base),
                                ("total", total, c64.sum(keepdims=True))):
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, f"{what}: {len(bad)} of {name} differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"
        place = base[np.arange(n) // SCAN_GROUP] + offsets                    # what the step kernel adds a lane's rank to
        bad = np.flatnonzero(place != before_all)
        assert len(bad) == 0, f"{what}: group_base[i // 1024] + offsets[i] is not the exclusive sum at {bad[0]}"
    finally:
        for o in outs:
            o.free()
