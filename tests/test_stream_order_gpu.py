"""One handle's device calls take effect in call order when the stream changes between them (INTEGRATION.md section 4,
rt_internal.h: THE STREAM RULE).  Every stream test of the rest of the suite synchronises its stream before the handle's next
call, so the earlier stream is idle when the rule's fence is reached.  Here it is not: every case

  1. holds stream A busy (held_stream.py), 2. issues call 1 on A, 3. asserts that the hold is still in force -- call 1 has not
  started -- and, with no synchronisation of any kind, issues call 2 on stream B, 4. synchronises both streams, checks that the
  hold lasted as long as planned, and 5. compares every word of both calls' outputs with that call's own reference, bit for bit.

Call 2 has call 1's shape, so no scratch grows and every access stays inside the handle's buffers; its parameters make its
reference differ from call 1's in more than half of the cells (tests/test_stream_order_cpu.py).  A library without the rule
lets call 2 overwrite the state call 1 has yet to read -- the lens camera's and the indirect term's generated rays first of all,
which those units write before their first launch -- and one call then traces the other's rays: the message of a wrong call
says how many of its wrong words equal the OTHER call's reference.  (On the library before rt_internal_order_stream() it was
call 2: its ray generation ran at once, the fence in its first launch waited for call 1, whose ray generation overwrote the
rays, and call 2 came out as call 1's reference word for word.)  The outputs are filled with poisoned.py's sentinel before the
calls.

Three calls cannot be held: rt_render_adaptive_device, rt_mirror_records_compact_device and rt_glass_records_compact_device wait
for their own stream inside the call (include/rt_capi_adaptive.h, include/rt_mirror_compact.h, include/rt_glass_compact.h), so
call 1 returns after the hold whatever the library does, and step 3 asserts that wait in place of the hold.  Their pairs still change streams with call 1's last stage in flight.

The stream pairs (A, B) are (side, other side), (side, null) and (null, side).  Bar: BIT-EXACT."""
import ctypes as C
import time

import numpy as np
import pytest

import glass_scenes
import held_stream
import mirror_scenes
import poisoned
import stream_order_refs as refs
from tilecoderaytracer_amd import HostScene, Renderer

pytestmark = pytest.mark.gpu

W, H, N = refs.W, refs.H, refs.W * refs.H
STREAM_PAIRS = (("side", "other"), ("side", "null"), ("null", "side"))
PAIR_IDS = [f"{a}-then-{b}" for a, b in STREAM_PAIRS]


@pytest.fixture(scope="module")
def streams():
    return held_stream.streams()


class Outputs:
    """device buffers of the shapes of a call's reference arrays, every word (byte) the sentinel"""

    def __init__(self, want):
        import torch
        self.want = want
        self.bufs = [torch.empty(a.nbytes // (1 if a.dtype.itemsize == 1 else 4), device="cuda",
                                 dtype=torch.uint8 if a.dtype.itemsize == 1 else torch.int32) for a in want]
        self.host = None
        self.refill()

    def refill(self):
        self.host = None
        for b in self.bufs:
            b.fill_(poisoned.SENTINEL_BYTE if b.element_size() == 1 else poisoned.SENTINEL)

    def ptrs(self):
        return [b.data_ptr() for b in self.bufs]

    def got(self):
        """the outputs as numpy arrays of the reference's shapes (a host call's: what it returned)"""
        if self.host is not None:
            return tuple(np.ascontiguousarray(a) for a in self.host)
        return tuple(b.cpu().numpy().view(w.dtype).reshape(w.shape) for b, w in zip(self.bufs, self.want))


class Pair:
    """two calls on one handle: call(k, ptrs, stream) issues call k (0 or 1) into the device addresses ptrs on the HIP stream
    `stream`, or -- a host call -- returns its outputs; reset() undoes what a call leaves set on the handle"""

    def __init__(self, case, handle, call, reset=None, waits=False):
        self.case, self.handle, self.call, self.reset, self.waits = case, handle, call, reset, waits
        self.want = (refs.reference(case, 0), refs.reference(case, 1))
        self.out = (Outputs(self.want[0]), Outputs(self.want[1]))

    def issue(self, k, stream):
        back = self.call(k, self.out[k].ptrs(), stream)
        if back is not None:
            self.out[k].host = back if isinstance(back, tuple) else (back,)


def mismatch(got, want, other):
    """-> None, or the text for outputs that are not their reference: how many words differ, how many of those equal the other
    call's reference and how many were never written"""
    wrong = mixed = unwritten = total = 0
    first = None
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (g.shape, w.shape)
        gw, ww = refs.words(g), refs.words(w)
        bad = gw != ww
        total += gw.size
        if not bad.any():
            continue
        wrong += int(bad.sum())
        unwritten += int((gw[bad] == (poisoned.SENTINEL_BYTE if gw.dtype == np.uint8 else poisoned.SENTINEL)).sum())
        if k < len(other) and other[k].shape == w.shape and other[k].dtype.itemsize == w.dtype.itemsize:
            mixed += int((gw[bad] == refs.words(other[k])[bad]).sum())
        if first is None:
            cell, word = (int(v[0]) for v in np.nonzero(bad))
            first = f"output {k}, cell (x={cell // H}, z={cell % H}) word {word}: got 0x{int(gw[cell, word]):x}, reference 0x{int(ww[cell, word]):x}"
    if wrong == 0:
        return None
    return (f"{wrong} of {total} words differ from the call's own reference; {mixed} of them equal the OTHER call's reference, "
            f"{unwritten} were never written; first at {first}")


def run_held(pair, a, b, what):
    """the pattern of the module's docstring on pair.handle, streams a then b"""
    import torch
    pair.issue(0, a.cuda_stream)                          # every scratch of both calls grown, every table uploaded
    a.synchronize()
    pair.issue(1, b.cuda_stream)
    torch.cuda.synchronize()
    if pair.reset:
        pair.reset()
    kernels_ms, wall_ms = held_stream.idle_times(lambda s: pair.issue(0, s), lambda s: pair.issue(1, s), a, b)
    if pair.reset:
        pair.reset()
    plan = held_stream.planned_ms(kernels_ms, wall_ms)
    for o in pair.out:
        o.refill()
    torch.cuda.synchronize()

    held = held_stream.hold(a, plan)
    pair.issue(0, a.cuda_stream)
    ended_early = held.query()
    if pair.waits:
        # rt_render_adaptive_device and rt_*_records_compact_device wait for their own stream by their definition (how many
        # pixels, how many rays the next stage has): the call returns after the hold, whatever the library does, and only its
        # last stage can still be in flight when call 2 is issued.  That wait is what is asserted of them.
        assert ended_early, f"{what}: call 1 is documented to wait for its stream and returned while that stream was held"
        ended_early = False
    pair.issue(1, b.cuda_stream)                          # no synchronisation of any kind between the two
    a.synchronize()
    b.synchronize()
    torch.cuda.synchronize()
    lasted = held.lasted_ms()
    note = (f"{what}: hold planned {plan:.3f} ms = max({held_stream.WALL_FACTOR:g} x {wall_ms:.3f} ms wall clock of call 2 on "
            f"the idle handle, {kernels_ms:.3f} ms of call 1's kernels on the idle stream), lasted {lasted:.3f} ms")
    print(note)
    assert not ended_early, f"{note}: the hold had ended before call 2 was issued, the test shows nothing"
    assert lasted >= plan, f"{note}: the hold was shorter than planned"
    got = (pair.out[0].got(), pair.out[1].got())
    bad1 = mismatch(got[0], pair.want[0], pair.want[1])
    assert bad1 is None, f"{note}: CALL 1 (stream A, held): {bad1}"
    bad2 = mismatch(got[1], pair.want[1], pair.want[0])
    assert bad2 is None, f"{note}: CALL 2 (stream B): {bad2}"


# ---- the handles and the calls ---------------------------------------------------------------------------------------------------

def camera_pointer(scene, camera):
    desc = refs.camera_desc(scene, camera)
    return None if desc is None else (C.pointer(desc), desc)


class Handle:
    """a Renderer whose calls can look through another camera than its scene's"""

    def __init__(self, r, scene="builtin"):
        self.r, self.scene, self.own, self.keep = r, scene, r._cam, {}

    def under(self, camera):
        if camera is None:
            self.r._cam = self.own
        else:
            if camera not in self.keep:
                self.keep[camera] = camera_pointer(self.scene, camera)
            self.r._cam = self.keep[camera][0]
        return self.r


def builtin():
    return Handle(Renderer(HostScene.builtin()))


def glass_renderer():
    from test_refract_gpu import make
    from test_texture_gpu import Desc
    host, refr = glass_scenes.host_scene("glass")
    return make(Desc(host), refractive=refr)


def on_device(a):
    a = np.ascontiguousarray(a)
    return poisoned._on_device(a.view(np.int32) if a.dtype.itemsize != 4 else a)


def lens_pair(chunk_columns=0, host_second=False):
    h = builtin()
    L = refs.LENS

    def call(k, ptrs, stream):
        kw = dict(samples=L["samples"], focus=refs.FOCUS, **L["calls"][k])
        if k == 1 and host_second:
            return h.r.render_lens(W, H, L["depth"], **kw)
        h.r.render_lens_device(W, H, L["depth"], 0, W, ptrs[0], stream, chunk_columns=chunk_columns if k == 0 else 0, **kw)
    return Pair("lens", h, call)


def indirect_pair(emitters, host_second=False):
    h = builtin()
    I = refs.INDIRECT
    records = refs.records()
    d_hits = on_device(records)

    def call(k, ptrs, stream):
        kw = dict(samples=I["samples"], gather_depth=I["gather_depth"], emitters=emitters, **I["calls"][k])
        if k == 1 and host_second:
            return h.r.indirect_diffuse(np.array(records), **kw)
        h.r.indirect_diffuse_device(N, d_hits.data_ptr(), 0, ptrs[0], stream, **kw)
    pair = Pair(f"indirect-emitters{int(emitters)}", h, call)
    pair.keep = d_hits
    return pair


def adaptive_pair():
    h = builtin()

    def call(k, ptrs, stream):
        h.under((None, refs.OTHER_CAMERA)[k]).render_adaptive_device(W, H, refs.ADAPTIVE["depth"], 0, W, ptrs[0], ptrs[1], stream,
                                                                     samples=refs.ADAPTIVE["samples"])
    return Pair("adaptive", h, call, waits=True)


def mirror_pair(compact):
    M = refs.MIRROR
    h = Handle(Renderer(mirror_scenes.host_scene(M["key"])), M["key"])
    d_rays = [on_device(mirror_scenes.pixel_rays(M["key"], W, H, c["camera"])) for c in M["calls"]]

    def call(k, ptrs, stream):
        h.r.mirror_records_device(N, H, d_rays[k].data_ptr(), *ptrs, stream=stream, max_bounces=refs.BOUNCES,
                                  min_reflective=M["calls"][k]["min_reflective"], compact=compact)
    pair = Pair("mirror", h, call, waits=compact)
    pair.keep = d_rays
    return pair


def glass_pair(compact=(False, False)):
    """compact[k]: call k is rt_glass_records_compact_device (include/rt_glass_compact.h), which waits for its own stream"""
    G = refs.GLASS
    h = Handle(glass_renderer(), G["key"])
    d_rays = [on_device(glass_scenes.pixel_rays(G["key"], W, H, c["camera"])) for c in G["calls"]]

    def call(k, ptrs, stream):
        h.r.glass_records_device(N, H, d_rays[k].data_ptr(), *ptrs, stream=stream, max_bounces=refs.BOUNCES,
                                 min_reflective=G["min_reflective"], min_transmissive=G["calls"][k]["min_transmissive"],
                                 compact=compact[k])
    pair = Pair("glass", h, call, waits=compact[0])
    pair.keep = d_rays
    return pair


def crossed_pair():
    X = refs.CROSSED
    h = Handle(glass_renderer(), X["key"])
    d_rays = [on_device(glass_scenes.pixel_rays(X["key"], W, H, c)) for c in X["cameras"]]

    def call(k, ptrs, stream):
        if k == 0:
            h.r.mirror_records_device(N, H, d_rays[0].data_ptr(), *ptrs, stream=stream, max_bounces=refs.BOUNCES,
                                      min_reflective=X["min_reflective"])
        else:
            h.r.glass_records_device(N, H, d_rays[1].data_ptr(), *ptrs, stream=stream, max_bounces=refs.BOUNCES,
                                     min_reflective=X["min_reflective"], min_transmissive=X["min_transmissive"])
    pair = Pair("crossed", h, call)
    pair.keep = d_rays
    return pair


def stack_pair():
    h = builtin()
    h.r.set_option("stack", 2)                            # the bounce stack in HBM: the buffer every launch of the handle shares

    def call(k, ptrs, stream):
        h.under((None, refs.OTHER_CAMERA)[k]).render_device(W, H, refs.STACK_DEPTH, 0, W, ptrs[0], stream)
    return Pair("stack", h, call)


def gbuffer_pair():
    h = builtin()

    def call(k, ptrs, stream):
        h.under((None, refs.OTHER_CAMERA)[k]).render_gbuffer_device(W, H, refs.DEPTH, 0, W, ptrs[0], ptrs[1], stream)
    return Pair("gbuffer", h, call)


def rays_queries_pair():
    h = builtin()
    d_rays = on_device(refs.pixel_rays())

    def call(k, ptrs, stream):
        if k == 0:
            h.r.trace_rays_device(N, H, d_rays.data_ptr(), refs.DEPTH, ptrs[0], stream)
        else:
            h.r.intersect_rays_device(N, H, d_rays.data_ptr(), ptrs[0], stream)
    pair = Pair("rays-queries", h, call)
    pair.keep = d_rays
    return pair


def ao_pair():
    h = builtin()
    d_hits = on_device(refs.records())

    def call(k, ptrs, stream):
        h.r.ambient_occlusion_device(N, H, d_hits.data_ptr(), ptrs[0], samples=refs.AO["samples"], channels=1, stream=stream,
                                     **refs.AO["calls"][k])
    pair = Pair("ao", h, call)
    pair.keep = d_hits
    return pair


def repack_pair():
    """call 2 is an rt_set_option that packs and uploads the tables anew -- the tables call 1, still held, has yet to read --
    and then the same frame through the kernel of the new tables"""
    h = builtin()

    def call(k, ptrs, stream):
        if k == 1:
            h.r.set_option("cull", 0)
        h.r.render_device(W, H, refs.DEPTH, 0, W, ptrs[0], stream)
    return Pair("repack", h, call, reset=lambda: h.r.set_option("cull", 1))


DEVICE_PAIRS = {
    "lens": lens_pair,
    "lens-call-1-in-four-chunks": lambda: lens_pair(chunk_columns=refs.LENS_CHUNK_COLUMNS),
    "indirect-emitters0": lambda: indirect_pair(False),
    "indirect-emitters1": lambda: indirect_pair(True),
    "adaptive": adaptive_pair,
    "mirror": lambda: mirror_pair(False),
    "mirror-compact": lambda: mirror_pair(True),
    "glass": glass_pair,
    "glass-compact": lambda: glass_pair((True, True)),
    "glass-compact-then-glass": lambda: glass_pair((True, False)),
    "mirror-then-glass": crossed_pair,
    "render-stack-in-hbm": stack_pair,
    "gbuffer": gbuffer_pair,
    "rays-then-queries": rays_queries_pair,
    "ao": ao_pair,
    "repack": repack_pair,
}
# the host variants work on the null stream: stream B is the null stream, A a side stream
HOST_PAIRS = {
    "lens": lambda: lens_pair(host_second=True),
    "indirect-emitters0": lambda: indirect_pair(False, host_second=True),
    "indirect-emitters1": lambda: indirect_pair(True, host_second=True),
}


@pytest.mark.parametrize("a,b", STREAM_PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("case", list(DEVICE_PAIRS))
def test_two_device_calls_of_one_handle_across_a_change_of_stream(streams, case, a, b):
    pair = DEVICE_PAIRS[case]()
    if case == "lens-call-1-in-four-chunks":
        assert -(-W // refs.LENS_CHUNK_COLUMNS) == 4
    try:
        run_held(pair, streams[a], streams[b], f"{case}, stream {a} then {b}")
        if case == "lens-call-1-in-four-chunks":
            assert pair.handle.r.lens_info().chunks == 1          # (call 2's; call 1's four are in the reference's bits)
    finally:
        pair.handle.r.close()


@pytest.mark.parametrize("case", list(HOST_PAIRS))
def test_a_host_call_after_a_device_call_on_a_side_stream(streams, case):
    pair = HOST_PAIRS[case]()
    try:
        run_held(pair, streams["side"], streams["null"], f"{case}, host variant after the device variant on a side stream")
    finally:
        pair.handle.r.close()


def test_two_handles_one_per_stream_never_wait_for_each_other(streams):
    """Two handles of different scenes, one on stream A, which is held, one on stream B; four calls interleaved, nothing
    synchronised between them.  The second handle's calls finish while the first handle's stream is still held (a handle waits
    for its OWN previous stream alone), the first handle's second call, on its previous stream, waits for nothing, and each
    of the four frames is its own reference."""
    import torch
    a, b = streams["side"], streams["other"]
    one, two = builtin(), Handle(Renderer(HostScene.named("grid16")), "grid16")
    want = [refs.two_handles_reference(i) for i in range(4)]
    out = [Outputs((w,)) for w in want]
    handles = (one, two, one, two)
    lanes = (a, b, a, b)

    def issue(i):
        scene, camera, depth = refs.TWO_HANDLES[i]
        assert handles[i].scene == scene
        handles[i].under(camera).render_device(W, H, depth, 0, W, out[i].ptrs()[0], lanes[i].cuda_stream)

    try:
        for i in range(4):                                # every buffer of both handles grown
            issue(i)
        torch.cuda.synchronize()
        t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0[0].record(a)
        issue(0), issue(2)
        t0[1].record(a)
        t0[1].synchronize()
        kernels_ms = t0[0].elapsed_time(t0[1])
        w0 = time.perf_counter()
        issue(1), issue(3)
        b.synchronize()
        wall_ms = (time.perf_counter() - w0) * 1.0e3
        plan = held_stream.planned_ms(kernels_ms, 2.0 * wall_ms)          # (both handles' host work lies inside the hold)
        for o in out:
            o.refill()
        torch.cuda.synchronize()

        held = held_stream.hold(a, plan)
        issue(0)
        issue(1)
        issue(2)
        returned_held = not held.query()                  # the first handle's call on its previous stream waited for nothing
        issue(3)
        b.synchronize()
        finished_held = not held.query()                  # the second handle's two frames are done, the hold is not
        a.synchronize()
        torch.cuda.synchronize()
        lasted = held.lasted_ms()
        note = (f"two handles: hold planned {plan:.3f} ms = max({held_stream.WALL_FACTOR:g} x 2 x {wall_ms:.3f} ms wall clock of the "
                f"second handle's calls, {kernels_ms:.3f} ms of the first handle's kernels), lasted {lasted:.3f} ms")
        print(note)
        assert lasted >= plan, f"{note}: the hold was shorter than planned"
        assert returned_held, f"{note}: the first handle's second call, on the stream of its first, returned after the hold"
        assert finished_held, f"{note}: the second handle's calls on stream B finished only after the hold on stream A"
        for i in range(4):
            others = tuple(w for j, w in enumerate(want) if j != i)
            bad = mismatch(out[i].got(), (want[i],), (others[0],))
            assert bad is None, f"{note}: frame {i} {refs.TWO_HANDLES[i]}: {bad}"
    finally:
        one.r.close()
        two.r.close()
