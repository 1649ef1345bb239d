"""Guided upsampling (include/rt_capi_upsample.h) where a frame's records pass 2^32 bytes, by test_large_composed_gpu.py's ground
rules: everything large stays on the device, every large output lies between sentinel guards, and two references that do not
share the addressing under test -- the same kernel on strips of at most 1024 columns, and upsample_ref on a few columns."""
import ctypes as C
import time

import numpy as np
import pytest

import large_extents as le
import upsample_ref
from large_extents import Guarded
from tilecoderaytracer_amd import HostScene, Renderer, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE, upsample_params

pytestmark = pytest.mark.gpu
F = np.float32
B32 = 1 << 32


def test_upsample_where_the_records_pass_2_32_bytes():
    """rt_subsample_hits_device and rt_upsample_guided_device on the records of a depth-0 rt_render_gbuffer_device at 9600 x 9600:
    92 160 000 records, 4.42 GB, so that the records of columns 9320 on lie past byte 2^32; s = 4 (2400 x 2400 cells), three
    channels made on the device, modulate, a plane term, onto the frame's colours, with flags.
    (1) the white cells equal the records' own [::4, ::4] slice, taken by torch;
    (2) every word of the output and every flag byte equal the same kernel's on strips of 1024 columns, each with the one column
        more that carries its right-hand cell (1025 columns upsampled, 1024 compared), into small guarded buffers;
    (3) columns 0..3, the last four and those around byte 2^32 of the records equal upsample_ref.
    The kernels index records, values and outputs by 64-bit ELEMENT numbers (a pixel number fits 32 bits at every size the calls
    accept; only byte offsets do not).  Seen to fail, on an MI355X, under each of two one-line narrowings of a record's address to
    32 bits of BYTES, which read columns 9320 on from the frame's first columns:
      `hits + (uint32_t)(48 * index) / 16` for `hits + 3 * index` in load_rec (the subsample's and the pixel's own record): (1)
        fails, the cells differ from the records' slice;
      `hits[(uint32_t)(48 * (...)) / 16 + word]` for `hits[3 * (...) + word]` where the tile's taps are staged in LDS: (2) fails,
        78 306 of 11 059 200 words of columns 9216:9600 differ from their strip, the first in column 9317 (the first pixel whose
        right-hand cell, column 9320, lies past 2^32 bytes)."""
    import torch
    W = H = 9600
    s, N = 4, W * H
    Wl = Hl = W // s
    hw, cw = 12 * H, 3 * H
    assert 48 * N > B32
    need = Guarded.need(12 * N) + 2 * Guarded.need(3 * N) + Guarded.need(N, as_bytes=True) + 48 * Wl * Hl * 2 + 12 * Wl * Hl \
        + Guarded.need(1025 * cw) + Guarded.need(1025 * H, as_bytes=True) + (3 << 30)
    le.require_device_memory(need)
    cols = sorted(set(le.boundary_columns([B32], 48 * H, W)) | {1, 2, 3, W - 4, W - 3, W - 2})
    params = upsample_params(s, 3, 3, False, True, 0.05, 0.0)
    lib = capi.load_library()
    r = Renderer(HostScene.builtin())
    t0 = time.time()
    hits = base = out = flags = small = small_flags = cells = None
    try:
        hits, base = Guarded(12 * N), Guarded(3 * N)
        r.render_gbuffer_device(W, H, 0, 0, W, base.ptr, hits.ptr)
        torch.cuda.synchronize()
        hits.assert_written("the frame's records")
        base.assert_written("the frame's colours")
        # (1)
        cells = Guarded(12 * Wl * Hl)
        capi.check(lib.rt_subsample_hits_device(0, s, 1, W, H, hits.ptr, cells.ptr, None))
        torch.cuda.synchronize()
        cells.assert_written("the cells")
        want = hits.body.view(W, H, 12)[::s, ::s].contiguous()
        dead = (want[..., 0] < 0) | ((want[..., 11] & 2) != 0)
        want[..., 8:11] = torch.where(dead[..., None], want[..., 8:11], torch.tensor(0x3F800000, dtype=torch.int32, device="cuda"))
        assert torch.equal(cells.body.view(Wl, Hl, 12), want), "the cells differ from the records' [::4, ::4] slice"
        assert int(dead.sum()) > 1000 and int((~dead).sum()) > 1000
        del want, dead
        cells.free()
        # the low-resolution values: a hash of the cell's number, in [0, 1)
        k = torch.arange(3 * Wl * Hl, dtype=torch.int64, device="cuda")
        lo = (((k * 2654435761) >> 7) & 0xFFFF).to(torch.float32) / 65536.0
        del k
        out, flags = Guarded(3 * N), Guarded(N, as_bytes=True)
        what = f"rt_upsample_guided_device {W}x{H} s{s}"
        capi.check(lib.rt_upsample_guided_device(0, C.byref(params), W, H, hits.ptr, lo.data_ptr(), base.ptr, out.ptr, flags.ptr, None))
        torch.cuda.synchronize()
        out.assert_written(what)
        flags.assert_written(what + ", flags")
        holes = le.count_equal(flags.body, 1)
        assert holes + le.count_equal(flags.body, 0) == N and holes >= 1     # (85 on this frame)
        # (2)
        small, small_flags = Guarded(1025 * cw), Guarded(1025 * H, as_bytes=True)
        for x0 in range(0, W, le.STRIP_COLUMNS):
            x1 = min(x0 + le.STRIP_COLUMNS, W)
            x1h = min(x1 + 1, W)
            small.refill()
            small_flags.refill()
            capi.check(lib.rt_upsample_guided_device(0, C.byref(params), x1h - x0, H, hits.ptr + x0 * H * 48,
                                                     lo.data_ptr() + (x0 // s) * Hl * 12, base.ptr + x0 * H * 12, small.ptr,
                                                     small_flags.ptr, None))
            torch.cuda.synchronize()
            small.assert_written(f"{what}: strip {x0}:{x1h}", (x1h - x0) * cw)
            assert small.sentinels_left() == small.n - (x1h - x0) * cw, f"{what}: strip {x0}:{x1h} was written past its end"
            small_flags.assert_written(f"{what}: flags of strip {x0}:{x1h}", (x1h - x0) * H)
            text = le.device_difference(out.body[x0 * cw:x1 * cw], small.body[:(x1 - x0) * cw], cw,
                                        f"{what}: columns {x0}:{x1} against their own strip", x0)
            assert text is None, text
            assert torch.equal(flags.body[x0 * H:x1 * H], small_flags.body[:(x1 - x0) * H]), f"{what}: flags of columns {x0}:{x1}"
        # (3)
        lo_host = lo.cpu().numpy().reshape(Wl, Hl, 3)
        for c0, c1 in le.runs(cols):
            a0, a1 = (c0 // s) * s, min(W, ((c1 - 1) // s + 1) * s + 1)              # whole cells, and the right-hand cell's column
            h = hits.body[a0 * hw:a1 * hw].cpu().numpy().view(HIT_DTYPE).reshape(a1 - a0, H)
            b = base.body[a0 * cw:a1 * cw].cpu().numpy().view(F).reshape(a1 - a0, H, 3)
            part_lo = np.ascontiguousarray(lo_host[a0 // s:upsample_ref.cells_of(a1, s)])
            want, want_flags = upsample_ref.upsample(h, part_lo, s, 3, False, True, 0.05, 0.0, b)
            got = out.body[c0 * cw:c1 * cw].cpu().numpy().view(F).reshape(c1 - c0, H, 3)
            d = le.first_difference(got.view(np.int32), want[c0 - a0:c1 - a0].view(np.int32))
            assert d is None, (f"{what}: columns {c0}:{c1} against upsample_ref: {d[3]} words differ, first in column "
                               f"{c0 + d[0] // cw}, word {d[0] % cw} of it")
            got_flags = flags.body[c0 * H:c1 * H].cpu().numpy().reshape(c1 - c0, H)
            assert np.array_equal(got_flags.astype(bool), want_flags[c0 - a0:c1 - a0]), f"{what}: flags of columns {c0}:{c1}"
        assert out.guards_untouched() and flags.guards_untouched() and hits.guards_untouched() and base.guards_untouched()
        print(f"[large upsample] {what}: {holes} holes of {N} pixels, {time.time() - t0:.1f} s")
    finally:
        for g in (hits, base, out, flags, small, small_flags, cells):
            if g is not None:
                g.free()
        torch.cuda.empty_cache()
        r.close()

