"""Temporal accumulation (include/rt_temporal.h) where a frame's records pass 2^32 bytes four times over, by
test_large_composed_gpu.py's ground rules: everything large stays on the device, every large output lies between sentinel guards,
and two references that do not share the addressing under test -- the same kernel on strips of at most 1024 columns, and
temporal_ref on a few columns."""
import ctypes as C
import time

import numpy as np
import pytest

import large_extents as le
import temporal_ref
from large_extents import Guarded, hashed
from tilecoderaytracer_amd import HostScene, Renderer, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE, temporal_params

pytestmark = pytest.mark.gpu
F = np.float32
B32 = 1 << 32


def test_accumulate_where_the_records_pass_2_32_bytes():
    """rt_temporal_accumulate_device on the records of a depth-0 rt_render_gbuffer_device at 18 944 x 18 944: 358 875 136 records,
    17.2 GB, so that the record plane passes byte 2^32, 2 * 2^32, 3 * 2^32 and 4 * 2^32; one channel, equal cameras (the identity
    path: a pixel's only tap is its own cell of the previous frame, whose records are the frame's own), max_history 4 over
    previous lengths 1..6, every output asked for.
    (1) every word of the value, the moments, the length and the variance and every flag byte equal the same kernel's on strips of
        1024 columns, written at offset 0 of small guarded buffers;
    (2) columns 0, the last one and those around each of the four boundaries equal temporal_ref, computed from those columns alone.
    The kernel indexes records, values and outputs by 64-bit ELEMENT numbers (a pixel number fits 32 bits at every size the call
    accepts; only byte offsets do not).  The one-line narrowing this is there for, of a record's address to 32 bits of BYTES --
    `hits + (uint32_t)(48 * index) / 16` for `hits + 3 * index` in load_rec (the pixel's own record and its taps') -- reads the
    records of column 4723's upper part and every later column from the frame's first columns, inside the buffer: a strip of (1)
    then reads its current records, at small offsets from its own pointer, rightly and its taps wrongly, so (1) differs wherever
    the two records differ, and (2), whose reference sees those columns alone, differs likewise.  (Derived from the code; the
    narrowed build was not run.)"""
    import torch
    W = H = 18944
    N = W * H
    assert 48 * N > 4 * B32
    need = Guarded.need(12 * N) + Guarded.need(3 * N) + 5 * 4 * N + 2 * Guarded.need(N) + Guarded.need(2 * N) + Guarded.need(N) \
        + Guarded.need(N, as_bytes=True) + 6 * Guarded.need(le.STRIP_COLUMNS * H * 2) + (3 << 30)
    le.require_device_memory(need)
    cols = le.boundary_columns([B32, 2 * B32, 3 * B32, 4 * B32], 48 * H, W)
    params = temporal_params(1, False, 4, 0.9, 0.05, 0.0, 0.25)
    lib = capi.load_library()
    host = HostScene.builtin()
    r = Renderer(host)
    cam = host.camera.contents
    cam_prev = type(cam)()
    C.memmove(C.byref(cam_prev), C.byref(cam), C.sizeof(cam))
    t0 = time.time()
    bufs = []
    try:
        hits, colours = Guarded(12 * N), Guarded(3 * N)
        bufs += [hits, colours]
        r.render_gbuffer_device(W, H, 0, 0, W, colours.ptr, hits.ptr)
        torch.cuda.synchronize()
        hits.assert_written("the frame's records")
        colours.free()
        torch.cuda.empty_cache()
        cur, p_value, p_len = hashed(N, 1), hashed(N, 2), hashed(N, 3, 5.0, 1.0)
        p_moments = hashed(2 * N, 4)
        out = [Guarded(N), Guarded(2 * N), Guarded(N), Guarded(N), Guarded(N, as_bytes=True)]
        bufs += out
        what = f"rt_temporal_accumulate_device {W}x{H}"

        def call(x0, x1, ptrs):
            capi.check(lib.rt_temporal_accumulate_device(0, C.byref(params), C.byref(cam_prev), C.byref(cam), W, H, x0, x1,
                                                         cur.data_ptr() + x0 * H * 4, hits.ptr + x0 * H * 48, hits.ptr,
                                                         p_value.data_ptr(), p_moments.data_ptr(), p_len.data_ptr(), *ptrs, None))

        call(0, W, [g.ptr for g in out])
        torch.cuda.synchronize()
        for g, name in zip(out, ("value", "moments", "length", "variance", "flags")):
            g.assert_written(f"{what}, {name}")
        without = le.count_equal(out[4].body, 1)
        assert without + le.count_equal(out[4].body, 0) == N and 1000 <= without <= N - 1000
        assert le.count_equal(out[2].body.view(torch.float32), 4.0) > 1000           # max_history reached
        # (1)
        per = (1, 2, 1, 1, 1)
        small = [Guarded(le.STRIP_COLUMNS * H * k, as_bytes=(n == 4)) for n, k in enumerate(per)]
        bufs += small
        for x0 in range(0, W, le.STRIP_COLUMNS):
            x1 = min(x0 + le.STRIP_COLUMNS, W)
            for s in small:
                s.refill()
            call(x0, x1, [s.ptr for s in small])
            torch.cuda.synchronize()
            for k, (big, s) in enumerate(zip(out, small)):
                words = (x1 - x0) * H * per[k]
                s.assert_written(f"{what}: output {k} of strip {x0}:{x1}", words)
                assert s.sentinels_left() == s.n - words, f"{what}: output {k} of strip {x0}:{x1} was written past its end"
                if k == 4:
                    assert torch.equal(big.body[x0 * H:x1 * H], s.body[:words]), f"{what}: flags of columns {x0}:{x1}"
                else:
                    text = le.device_difference(big.body[x0 * H * per[k]:x1 * H * per[k]], s.body[:words], H * per[k],
                                                f"{what}: output {k}, columns {x0}:{x1} against their own strip", x0)
                    assert text is None, text
        # (2)
        for c0, c1 in le.runs(cols):
            sl = lambda t, k: t[c0 * H * k:c1 * H * k].cpu().numpy()
            h = sl(hits.body, 12).view(HIT_DTYPE).reshape(c1 - c0, H)
            prev = (cam_prev, h, sl(p_value, 1).reshape(c1 - c0, H), sl(p_moments, 2).reshape(c1 - c0, H, 2), sl(p_len, 1).reshape(c1 - c0, H))
            want = temporal_ref.accumulate(sl(cur, 1).reshape(c1 - c0, H), h, cam, prev, max_history=4, alpha_moments=0.25)
            for k, (g, w) in enumerate(zip(out, want)):
                got = sl(g.body, per[k])
                w = np.ascontiguousarray(w).reshape(-1)
                d = le.first_difference(got.view(np.uint8 if k == 4 else np.int32), w.view(np.uint8 if k == 4 else np.int32))
                assert d is None, (f"{what}: output {k}, columns {c0}:{c1} against temporal_ref: {d[3]} words differ, first in "
                                   f"column {c0 + d[0] // (H * per[k])}, word {d[0] % (H * per[k])} of it")
        assert all(g.guards_untouched() for g in out) and hits.guards_untouched()
        print(f"[large temporal] {what}: {without} of {N} pixels without history, {time.time() - t0:.1f} s")
    finally:
        for g in bufs:
            g.free()
        cur = p_value = p_len = p_moments = None
        torch.cuda.empty_cache()
        r.close()
