"""Compact glass records (include/rt_glass_compact.h) on the GPU.  The header adds no definition: every output word of
rt_glass_records_compact* is held to glass_ref -- the definition of include/rt_glass.h -- and to rt_glass_records on the same
handle, word for word, on the scenes "glass", "edges" and "open" of glass_scenes.py (whose live rays per query
test_glass_compact_cpu.py counts): over bounce limits, reflectivity floors, min_transmissive at -inf, inside the tf values, one ulp
above one, on every threshold of "edges" and at +inf (where the words and the info's counts are rt_mirror_records_compact's
too), dense lists at the edges of a wavefront and a workgroup whose survivors are all glass steps or all mirror steps, a list
longer than one step of the scan covers, chunks, rows, strips, absent outputs, the device entry into sentinel-filled guarded
outputs, a capturing stream refused, a change of stream with the in-place call still held, and the Renderer's composed calls.
The info struct is held to the path words: alive[b] = |{i : (path[i] & 0xff) >= b}|.  Bar: BIT-EXACT."""
import ctypes as C

import numpy as np
import pytest

import glass_compact_batches as batches
import glass_ref
import glass_scenes
import poisoned
from mirror_large import expected_info
from test_glass_gpu import assert_all_same, assert_same, device_records, poisoned_device_records, rays_of, renderer_of
from tilecoderaytracer_amd import Renderer, capi
from tilecoderaytracer_amd.renderer import glass_params

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
NAMES = ("hits", "guide", "weight", "path")
W61, H37 = glass_scenes.SIZES[0]
W96, H80 = glass_scenes.SIZES[1]
LOOKS = (-INF, 0.5, glass_scenes.up(0.9), INF)


@pytest.fixture(scope="module")
def renderers():
    made = {key: renderer_of(key) for key in glass_scenes.KEYS}
    yield made
    for r in made.values():
        r.close()


def info_of(r):
    i = r.glass_compact_info()
    assert i.reserved == 0 and i.query_ms > 0 and (i.step_ms > 0 or i.rays == 0)
    return i.rays, i.rays_queried, i.chunks, i.queries, i.syncs, list(i.alive)


def mirror_info_of(r):
    i = r.mirror_compact_info()
    return i.rays, i.rays_queried, i.chunks, i.queries, i.syncs, list(i.alive)


# ---- 1. every output word is the definition's, and rt_glass_records' ----------------------------------------------------------------

@pytest.mark.parametrize("floor", [1.0, 0.5])
@pytest.mark.parametrize("bounces", [0, 1, 3, 8, 64])
@pytest.mark.parametrize("W,H", glass_scenes.SIZES)
@pytest.mark.parametrize("key", glass_scenes.KEYS)
def test_every_output_word_is_the_definitions_and_rt_glass_records(renderers, key, W, H, bounces, floor):
    r = renderers[key]
    rays = rays_of(key, W, H)
    for look in LOOKS + (glass_scenes.EDGES_LOOKS if key == "edges" else ()):
        what = f"{key} {W}x{H} bounces {bounces} floor {floor} look {look!r}"
        want = glass_scenes.reference(key, W, H, bounces, floor, look)
        got = r.glass_records(rays, bounces, floor, look, compact=True)
        assert_all_same(got, want, what)
        info = info_of(r)
        assert info == expected_info(want[3], bounces), what
        if look in LOOKS[:2]:                                                 # (the definition holds the others to it as well)
            assert_all_same(got, r.glass_records(rays, bounces, floor, look), what + " against rt_glass_records")
        if look == INF:                                                       # nothing looked through: the mirror compact call's
            assert_all_same(got, r.mirror_records(rays, bounces, floor, compact=True), what + " against rt_mirror_records_compact")
            assert mirror_info_of(r) == info, what


@pytest.mark.parametrize("floor,look", [(0.5, 0.5), (1.0, 0.2)])
@pytest.mark.parametrize("key", ["glass", "edges"])
def test_a_batch_with_misses_a_degenerate_ray_inside_starts_and_the_bubbles_rim(renderers, key, floor, look):
    """candidates without a child: across the bubble's rim and from inside the glass sphere -- on "edges" at floor 1.0 the rim goes
    on as a mirror and the inside starts end (test_glass_compact_cpu.py counts both), and the count must say of each what the
    step says"""
    rays = batches.handmade_rays()
    want = glass_ref.records(glass_scenes.ref_scene(key), rays, 3, floor, look)
    r = renderers[key]
    assert_all_same(r.glass_records(rays, 3, floor, look, compact=True), want, f"handmade {key}")
    assert info_of(r) == expected_info(want[3], 3)
    assert_all_same(device_records(r, rays, max_bounces=3, min_reflective=floor, min_transmissive=look, compact=True), want,
                    f"handmade {key} (device)")
    got = r.glass_records(rays, 3, floor, look, outputs=("path",), compact=True)             # GUIDE = false
    assert_same(got[0], want[0], f"handmade {key}, hits and path only: hits")
    assert_same(got[3], want[3], f"handmade {key}, hits and path only: path")


# ---- 2. the info struct -------------------------------------------------------------------------------------------------------------

def test_queries_and_syncs_at_the_ends_of_the_bounce_range(renderers):
    r = renderers["glass"]
    rays = rays_of("glass", W61, H37)
    n = W61 * H37
    r.glass_records(rays, 0, 0.5, 0.5, compact=True)                          # no bounce: one query and nothing to wait for
    assert info_of(r) == (n, n, 1, 1, 0, [n] + [0] * 64)
    renderers["open"].glass_records(rays_of("open", W61, H37), 8, 1.0, 0.5, compact=True)    # the early end: empty at query 4
    _, queried, chunks, queries, syncs, alive = info_of(renderers["open"])
    assert (queries, syncs, chunks) == (4, 4, 1) and alive[:5] == [2257, 1178, 332, 67, 0] and queried == sum(alive)
    r.glass_records(rays, 3, 0.5, 0.5, compact=True)                          # every bounce runs: no wait after the last
    _, queried, chunks, queries, syncs, alive = info_of(r)
    assert (queries, syncs, chunks) == (4, 3, 1) and alive[:5] == [2257, 1587, 782, 321, 0] and queried == sum(alive)
    r.glass_records(rays, 3, 0.5, 0.5, chunk_rays=1000, compact=True)
    assert info_of(r)[2:5] == (3, 12, 9)


def test_the_calls_infos_do_not_touch_each_other(renderers):
    r = renderers["glass"]
    rays = rays_of("glass", W61, H37)
    as_bytes = lambda info: bytes(memoryview(info))
    r.glass_records(rays[:30], 2, 1.0, 0.5)
    r.mirror_records(rays[:20], 2, 1.0, compact=True)
    glass, mirror = as_bytes(r.glass_info()), as_bytes(r.mirror_compact_info())
    assert r.glass_info().rays == 30 * H37 and r.mirror_compact_info().rays == 20 * H37
    r.glass_records(rays, 5, 0.5, 0.5, compact=True)
    assert as_bytes(r.glass_info()) == glass and as_bytes(r.mirror_compact_info()) == mirror
    mine = as_bytes(r.glass_compact_info())
    assert r.glass_compact_info().rays == W61 * H37 and "hits" in r.kernel_name()
    r.glass_records(rays[:11], 1, 1.0, 0.5)
    r.mirror_records(rays[:7], 1, 1.0, compact=True)
    assert as_bytes(r.glass_compact_info()) == mine
    assert r.glass_info().rays == 11 * H37 and r.mirror_compact_info().rays == 7 * H37


# ---- 3. list sizes at the edges of a wavefront and a workgroup ----------------------------------------------------------------------

@pytest.mark.parametrize("c", batches.LIST_SIZES)
@pytest.mark.parametrize("kind", batches.KINDS)
@pytest.mark.parametrize("bounce", [1, 2])
def test_list_sizes_at_the_edges_of_a_wavefront_and_a_workgroup(renderers, bounce, kind, c):
    """c rays whose chain reaches query `bounce` -- all by a glass step, or all by a mirror step -- among 300 whose chain ends one
    query sooner: the list of that bounce has exactly c entries"""
    ch = batches.chains()
    pick = batches.list_size_batch(bounce, c, kind)
    want = [w[pick] for w in ch["want"]]
    r = renderers["glass"]
    got = r.glass_records(np.ascontiguousarray(ch["rays"][pick]), batches.BOUNCES, batches.FLOOR, batches.LOOK, compact=True)
    assert_all_same(got, want, f"{c} live rays at bounce {bounce}, {kind} steps")
    info = info_of(r)
    assert info == expected_info(want[3], batches.BOUNCES) and info[5][bounce] == c and info[5][bounce - 1] == batches.ENDING + c


def test_a_batch_in_which_every_ray_is_alive_after_bounce_0(renderers):
    ch = batches.chains()
    pick = batches.all_alive_batch()
    want = [w[pick] for w in ch["want"]]
    r = renderers["glass"]
    got = r.glass_records(np.ascontiguousarray(ch["rays"][pick]), batches.BOUNCES, batches.FLOOR, batches.LOOK, compact=True)
    assert_all_same(got, want, "every ray alive after bounce 0")
    info = info_of(r)
    assert info == expected_info(want[3], batches.BOUNCES) and info[5][0] == info[5][1] == len(pick) == 5319


# ---- 4. more live entries than one step of the scan covers --------------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [0, 100000])
def test_more_live_entries_than_one_step_of_the_scan_covers(renderers, chunk):
    """the 96 x 80 frame 64 times: 491 520 rays, of which 340 416 are alive at query 1 -- 1330 workgroups' counts, two groups of
    the scan's first level (kScanBlock 1024, csrc/rt_scan.h).  As one chunk, and as five.  The reference is the tile's."""
    tiles = 64
    ch = batches.chains()
    rays = np.ascontiguousarray(np.tile(ch["rays"], (tiles, 1)))
    want = [np.tile(w, (tiles,) + (1,) * (w.ndim - 1)) for w in ch["want"]]
    assert len(rays) == 491520 and int(((want[3] & 0xff) >= 1).sum()) == 340416 > 1024 * 256
    r = renderers["glass"]
    got = r.glass_records(rays, batches.BOUNCES, batches.FLOOR, batches.LOOK, chunk_rays=chunk, compact=True)
    assert_all_same(got, want, f"{tiles} tiles, chunk_rays {chunk}")
    info = info_of(r)
    assert info == expected_info(want[3], batches.BOUNCES, chunk) and info[2] == (5 if chunk else 1)


# ---- 5. what never changes a bit ----------------------------------------------------------------------------------------------------

def test_chunks_rows_and_strips_never_change_a_bit(renderers):
    r = renderers["glass"]
    rays = rays_of("glass", W61, H37)
    want = glass_scenes.reference("glass", W61, H37, 3, 0.5, 0.5)[:4]
    n = W61 * H37
    for chunk in (300, 257, 256, 255, 1):
        got = r.glass_records(rays, 3, 0.5, 0.5, chunk_rays=chunk, compact=True)
        assert_all_same(got, want, f"chunk_rays {chunk}")
        assert info_of(r) == expected_info(want[3], 3, chunk), chunk           # alive and queries summed per chunk
    for rows in (1, H37, n):
        assert_all_same(r.glass_records(rays, 3, 0.5, 0.5, rows=rows, compact=True), want, f"rows {rows}")
    for x0, x1 in ((0, 23), (23, W61)):                                       # two strips against the frame
        got = r.glass_records(np.ascontiguousarray(rays[x0:x1]), 3, 0.5, 0.5, compact=True)
        assert_all_same(got, [w[x0:x1] for w in want], f"strip {x0}:{x1}")
        assert info_of(r) == expected_info(want[3][x0:x1], 3)


@pytest.mark.parametrize("key,floor,look", [("glass", 1.0, 0.5), ("edges", 0.5, 0.2)])
def test_each_optional_output_may_be_absent(renderers, key, floor, look):
    r = renderers[key]
    rays = rays_of(key, W61, H37)
    want = glass_scenes.reference(key, W61, H37, 3, floor, look)[:4]
    for absent in Renderer.MIRROR_OUTPUTS + (None, "all"):
        asked = () if absent == "all" else tuple(o for o in Renderer.MIRROR_OUTPUTS if o != absent)
        got = r.glass_records(rays, 3, floor, look, outputs=asked, compact=True)
        for name, g, w in zip(NAMES, got, want):
            if name == "hits" or name in asked:
                assert_same(g, w, f"without {absent}: {name}")
            else:
                assert g is None
        assert info_of(r) == expected_info(want[3], 3)


# ---- 6. the device entry point ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,bounces,floor,look,chunk", [("glass", 8, 0.5, 0.5, 0), ("edges", 4, 0.5, 0.2, 300),
                                                          ("glass", 0, 1.0, 0.5, 0), ("open", 8, 1.0, 0.5, 0)])
def test_device_entry_into_poisoned_words_on_a_stream_of_its_own(renderers, key, bounces, floor, look, chunk):
    """every output word is written -- exactly once, by the step that ends its ray: no later step can mend a sentinel -- and
    no guard word is touched"""
    r = renderers[key]
    want = glass_scenes.reference(key, W61, H37, bounces, floor, look)[:4]
    what = f"rt_glass_records_compact_device {key} bounces {bounces} chunk {chunk}"
    got = poisoned_device_records(r, rays_of(key, W61, H37), want, what, max_bounces=bounces, min_reflective=floor,
                                  min_transmissive=look, chunk_rays=chunk, compact=True)
    assert_all_same(got, want, what)
    assert info_of(r) == expected_info(want[3], bounces, chunk)


def test_a_capturing_stream_is_refused_and_the_next_call_is_unharmed():
    """the call waits for its stream, so it cannot be recorded: RT_ERR_INVALID before anything is enqueued -- the capture ends
    with an empty graph -- and the handle's next call gives the definition's words.  The Renderer is this test's own."""
    import torch
    r = renderer_of("glass")
    try:
        rays = rays_of("glass", W61, H37)
        n = W61 * H37
        want = glass_scenes.reference("glass", W61, H37, 3, 1.0, 0.5)[:4]
        assert_all_same(r.glass_records(rays, 3, 1.0, 0.5, compact=True), want, "before the capture")
        before = bytes(memoryview(r.glass_compact_info()))
        d_rays = poisoned._on_device(rays)
        bufs = [torch.zeros((n * w,), dtype=torch.int32, device="cuda") for w in (12, 12, 3, 1)]
        lib, p = capi.load_library(), glass_params(3, 1.0, 0.5)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            rc = lib.rt_glass_records_compact_device(r._scene, C.byref(p), n, H37, d_rays.data_ptr(), *[b.data_ptr() for b in bufs],
                                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
            message = lib.rt_last_error().decode()
        torch.cuda.synchronize()
        assert rc == capi.RT_ERR_INVALID and "capturing" in message, (rc, message)
        assert all(int(b.abs().max()) == 0 for b in bufs)                     # nothing was enqueued, nothing ran
        assert bytes(memoryview(r.glass_compact_info())) == before            # (a refused call is not the handle's last call)
        del graph
        assert_all_same(r.glass_records(rays, 3, 1.0, 0.5, compact=True), want, "after the refusal")
        assert_all_same(device_records(r, rays, max_bounces=3, min_reflective=1.0, min_transmissive=0.5, compact=True), want,
                        "after the refusal (device)")
    finally:
        r.close()


def test_device_entry_refuses_misaligned_outputs_and_the_next_call_is_unharmed(renderers):
    r = renderers["glass"]
    rays = rays_of("glass", W61, H37)
    d_rays = poisoned._on_device(rays)
    lib, p = capi.load_library(), glass_params(3, 1.0, 0.5)
    rc = lib.rt_glass_records_compact_device(r._scene, C.byref(p), 4, 4, d_rays.data_ptr(), d_rays.data_ptr() + 8, None, None, None,
                                             None)
    assert rc == capi.RT_ERR_INVALID and "d_out_hits" in lib.rt_last_error().decode()
    rc = lib.rt_glass_records_compact_device(r._scene, C.byref(p), 4, 4, d_rays.data_ptr(), d_rays.data_ptr(),
                                             d_rays.data_ptr() + 4, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "d_out_guide" in lib.rt_last_error().decode()
    p = glass_params(3, 1.0, float("nan"))
    rc = lib.rt_glass_records_compact_device(r._scene, C.byref(p), 4, 4, d_rays.data_ptr(), d_rays.data_ptr(), None, None, None, None)
    assert rc == capi.RT_ERR_INVALID and "min_transmissive" in lib.rt_last_error().decode()
    want = glass_scenes.reference("glass", W61, H37, 3, 1.0, 0.5)[:4]
    assert_all_same(r.glass_records(rays, 3, 1.0, 0.5, compact=True), want, "after a refusal")


def test_the_call_on_another_stream_than_a_held_glass_call_of_the_handle():
    """test_stream_order_gpu.py's pattern and its "glass" pair, call 2 through this header: stream A is held busy, call 1 --
    rt_glass_records_device, which never waits -- is issued on it and has not started when call 2 is issued on stream B with
    nothing synchronised.  Both calls' words are their own references': the new call waits for the handle's previous stream
    (rt_internal_order_stream) before it enqueues anything.  The handle is this test's own."""
    import held_stream
    import stream_order_refs as refs
    import test_stream_order_gpu as order
    G = refs.GLASS
    h = order.Handle(order.glass_renderer(), G["key"])
    try:
        d_rays = [order.on_device(glass_scenes.pixel_rays(G["key"], refs.W, refs.H, c["camera"])) for c in G["calls"]]

        def call(k, ptrs, stream):
            h.r.glass_records_device(refs.W * refs.H, refs.H, d_rays[k].data_ptr(), *ptrs, stream=stream, max_bounces=refs.BOUNCES,
                                     min_reflective=G["min_reflective"], min_transmissive=G["calls"][k]["min_transmissive"],
                                     compact=(k == 1))
        pair = order.Pair("glass", h, call)
        s = held_stream.streams()
        order.run_held(pair, s["side"], s["other"], "glass in place, then compact")
        assert h.r.glass_compact_info().rays == h.r.glass_info().rays == refs.W * refs.H
    finally:
        h.r.close()


# ---- 6b. between chunks, between calls, between handles -----------------------------------------------------------------------------

@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("floor", [1.0, 0.5])
@pytest.mark.parametrize("chunk", batches.OPEN_CHUNKS)
def test_chunks_that_end_at_different_bounces(renderers, chunk, floor, device):
    """"open" at max_bounces 8: chains end in misses and as one chunk the list is empty at query 4.  In chunks of 7, 64, 300 and
    1000 rays some chunks end after one query and others after four, and a chunk that ended early is followed by one that goes
    further (test_glass_compact_cpu.py holds that on the path words, and it is asserted here again): the next chunk starts at
    bounce 0 with cnt = its rays and the lists' roles by b & 1, whatever the bounce the chunk before stopped at.  No chunk of
    "open" runs all nine queries, so syncs == queries at max_bounces 8; at max_bounces 3 the chunks that run all four wait three
    times and the others once per query -- expected_info reckons both, per chunk."""
    r = renderers["open"]
    rays = rays_of("open", W61, H37)
    for bounces in (8, 3):
        want = glass_scenes.reference("open", W61, H37, bounces, floor, 0.5)[:4]
        q = batches.assert_chunks_end_at_different_bounces(np.asarray(want[3]).reshape(-1), bounces, chunk)
        what = f"open in chunks of {chunk}, max_bounces {bounces}, floor {floor}, {'device' if device else 'host'}"
        if device:
            got = poisoned_device_records(r, rays, want, what, max_bounces=bounces, min_reflective=floor, min_transmissive=0.5,
                                          chunk_rays=chunk, compact=True)
        else:
            got = r.glass_records(rays, bounces, floor, 0.5, chunk_rays=chunk, compact=True)
        assert_all_same(got, want, what)
        info = info_of(r)
        assert info == expected_info(want[3], bounces, chunk), what
        full = sum(1 for a in q if a == bounces + 1)
        assert info[2:5] == (len(q), sum(q), sum(q) - full) and (full == 0) == (bounces == 8), (what, q)


def test_one_handle_called_with_alternating_chunks_outputs_and_batches():
    """A fresh handle, called in turn with chunks, outputs and batches that change under scratch which only grows: the state
    buffer holds 4 or 14 planes of `stride = chunk` words, a stride that is not the one the buffer was grown for, and the batch
    of the third call (test_glass_gpu.py's handmade rays, an odd number that is no frame's) has another length.  First of all a
    call with max_bounces 0, which allocates no list.  Every call is bit-exact with its info."""
    rays = rays_of("glass", W61, H37)
    made = batches.handmade_rays()
    frame = lambda bounces: glass_scenes.reference("glass", W61, H37, bounces, 0.5, 0.5)[:4]
    made_want = glass_ref.records(glass_scenes.ref_scene("glass"), made, 3, 0.5, 0.5)[:4]
    assert len(made) % 2 == 1 and 257 < len(made) < 2 * 257 + 257
    #        rays, bounces, chunk_rays, outputs, reference
    calls = [(rays, 0, 0, NAMES[1:], frame(0)),                               # no list is allocated yet
             (rays, 8, 100, ("path",), frame(8)),
             (rays, 8, 0, NAMES[1:], frame(8)),
             (made, 3, 257, NAMES[1:], made_want),
             (rays, 8, 1000, ("path",), frame(8)),
             (rays, 8, 7, NAMES[1:], frame(8)),
             (rays, 8, 0, NAMES[1:], frame(8))]
    r = renderer_of("glass")
    try:
        for step, (batch, bounces, chunk, asked, want) in enumerate(calls):
            what = f"call {step} of one handle: {len(batch.reshape(-1, 6))} rays, max_bounces {bounces}, chunk_rays {chunk}, {asked}"
            got = r.glass_records(batch, bounces, 0.5, 0.5, chunk_rays=chunk, outputs=asked, compact=True)
            for name, g, w in zip(NAMES, got, want):
                if name == "hits" or name in asked:
                    assert_same(g, w, f"{what}: {name}")
                else:
                    assert g is None
            assert info_of(r) == expected_info(want[3], bounces, chunk), what
    finally:
        r.close()


def test_two_handles_on_two_streams_from_two_threads_at_once():
    """"glass" and "edges", a handle each, the compact device entry of each on a side stream of its own from a thread of its own,
    both started together, three rounds: every word of both is its own reference and each handle's info its own.  The scan's
    instantiation is shared code; its buffers, the device's total and the pinned word the host reads it through are a handle's."""
    import threading
    import torch
    keys = ("glass", "edges")
    n = W96 * H80
    want = {key: glass_scenes.reference(key, W96, H80, 8, 0.5, 0.5)[:4] for key in keys}
    assert expected_info(want["glass"][3], 8) != expected_info(want["edges"][3], 8)
    made = {key: renderer_of(key) for key in keys}
    try:
        d_rays = {key: poisoned._on_device(rays_of(key, W96, H80)) for key in keys}
        streams = {key: torch.cuda.Stream() for key in keys}
        assert len({s.cuda_stream for s in streams.values()} | {0}) == 3
        for rounds in range(3):
            bufs = {key: [torch.full((n * w,), poisoned.SENTINEL, dtype=torch.int32, device="cuda") for w in (12, 12, 3, 1)]
                    for key in keys}
            torch.cuda.synchronize()
            gate, errors = threading.Barrier(2), {}

            def work(key):
                try:
                    gate.wait(timeout=60)
                    made[key].glass_records_device(n, H80, d_rays[key].data_ptr(), *[b.data_ptr() for b in bufs[key]],
                                                   stream=streams[key].cuda_stream, max_bounces=8, min_reflective=0.5,
                                                   min_transmissive=0.5, compact=True)
                    streams[key].synchronize()
                except BaseException as e:                                    # (reported by the main thread)
                    errors[key] = e
            threads = [threading.Thread(target=work, args=(key,)) for key in keys]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, errors
            torch.cuda.synchronize()
            for key in keys:
                what = f"{key} beside {keys[1 - keys.index(key)]}, round {rounds}"
                for name, b, w in zip(NAMES, bufs[key], want[key]):
                    assert_same(b.cpu().numpy(), np.ascontiguousarray(w).reshape(-1).view(np.int32), f"{what}: {name}")
                assert info_of(made[key]) == expected_info(want[key][3], 8), what
    finally:
        for r in made.values():
            r.close()


# ---- 7. the Renderer's composed calls -----------------------------------------------------------------------------------------------

def test_render_gbuffer_mirrored_glass_compact_is_the_call_without_it_bit_for_bit(renderers):
    r = renderers["glass"]
    kw = dict(max_bounces=3, min_reflective=1.0, min_transmissive=0.5)
    plain = r.render_gbuffer_mirrored(W96, H80, 3, **kw)
    compact = r.render_gbuffer_mirrored(W96, H80, 3, glass_compact=True, **kw)
    for name, g, w in zip(("rgb",) + NAMES, compact, plain):
        assert_same(g, w, f"render_gbuffer_mirrored(glass_compact=True): {name}")
    assert_all_same(compact[1:], glass_scenes.reference("glass", W96, H80, 3, 1.0, 0.5)[:4], "render_gbuffer_mirrored(glass_compact=True)")
    assert info_of(r) == expected_info(plain[4], 3)
    strip = r.render_gbuffer_mirrored(W96, H80, 3, x0=17, x1=50, glass_compact=True, **kw)
    assert_all_same(strip[1:], [a[17:50] for a in plain[1:]], "columns 17:50")
    with pytest.raises(ValueError, match="glass_compact"):                    # only with min_transmissive
        r.render_gbuffer_mirrored(W96, H80, 3, max_bounces=3, min_reflective=1.0, glass_compact=True)
    with pytest.raises(ValueError, match="glass_compact"):                    # compact is the mirror call's; the text says which
        r.render_gbuffer_mirrored(W96, H80, 3, compact=True, **kw)


def test_mirrors_glass_compact_through_the_composed_renders(renderers):
    r = renderers["glass"]
    mirrors = dict(max_bounces=3, min_reflective=1.0, min_transmissive=0.5)
    compact = dict(mirrors, glass_compact=True)
    kw = dict(samples=2, gather_depth=1, gain=1.25, seed=3)
    assert_same(r.render_indirect(W61, H37, 2, mirrors=compact, **kw), r.render_indirect(W61, H37, 2, mirrors=mirrors, **kw),
                "render_indirect")
    assert r.glass_compact_info().rays == W61 * H37
    assert_same(r.render_ao(W61, H37, 2, radius=1.5, seed=4, mirrors=compact), r.render_ao(W61, H37, 2, radius=1.5, seed=4, mirrors=mirrors),
                "render_ao")
    cams = list(glass_scenes.room_cameras())
    acc = dict(term="indirect", samples=1, gain=1.25, max_history=3, plane_eps=0.02)
    want = r.render_accumulated(cams, 45, 38, 2, mirrors=mirrors, **acc)
    got = r.render_accumulated(cams, 45, 38, 2, mirrors=compact, **acc)
    for name, g, w in zip(("value", "variance", "flags"), got, want):
        assert_same(g.view(np.uint8) if g.dtype == bool else g, w.view(np.uint8) if w.dtype == bool else w, f"render_accumulated: {name}")
    assert r.glass_compact_info().rays == 45 * 38
    with pytest.raises(ValueError, match="glass_compact"):
        r.render_indirect(W61, H37, 2, mirrors=dict(max_bounces=3, min_reflective=1.0, glass_compact=True), **kw)
    with pytest.raises(ValueError, match="mirrors takes max_bounces, min_reflective and compact"):
        r.render_ao(W61, H37, 2, mirrors=dict(compact, glass_compacted=True))
