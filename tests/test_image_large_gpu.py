"""The image encoder's addressing past 2^32 bytes, after the pattern of test_large_extents_gpu.py: the input is made on the
device, the output lies between two sentinel-filled guards (large_extents.Guarded) with a pitch 64 bytes wider than a row, and
there are two references, neither sharing the addressing under test:
  (a) image_ref on the column that straddles each multiple of 2^32 bytes of the input (and 2^31 in the smaller frame), its two
      neighbours, column 0 and the last column -- all H rows of each, so every row of the output, the ones past 2^32 bytes too;
  (b) the same kernel's strips of at most 1024 columns, each read from its own address and encoded at offset 0 of a small buffer,
      compared on the device with the matching columns of the large output -- every byte of it.
With 4 channels a pixel is one word {r, g, b, 255}, which is never the sentinel (0x7FC5A5A5): a word that still holds it was not
written, and exactly the 16 words after each row's end must."""
import ctypes as C
import time

import numpy as np
import pytest

import image_ref
import large_extents as le
from large_extents import Guarded
from tilecoderaytracer_amd import capi
from tilecoderaytracer_amd.renderer import image_params

pytestmark = pytest.mark.gpu
F = np.float32
B31, B32 = 1 << 31, 1 << 32
SLACK = 3 << 30
GAP = 64                                 # bytes between a row's end and the next row


@pytest.fixture(autouse=True)
def measured(request):
    import torch
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"[image, large] {request.node.name}: {time.time() - t0:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    torch.cuda.empty_cache()


def fill_colours(body):
    """uniform [-0.1, 1.2) floats into an int32 device view, a GiB at a time, with a NaN, an infinity and a -0.0 now and then"""
    import torch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    for c0 in range(0, body.numel(), le.CHUNK_WORDS):
        part = body[c0:c0 + le.CHUNK_WORDS].view(torch.float32)
        part.uniform_(-0.1, 1.2, generator=gen)
        part[1::1009] = float("nan")
        part[2::1013] = float("inf")
        part[3::1019] = -0.0


@pytest.mark.parametrize("Wn, H, bottom_up, boundaries", [(20000, 18000, 1, [B31, B32]),
                                                          (32768, 32800, 0, [B32, 2 * B32, 3 * B32])])
def test_encode_past_2_32_bytes(Wn, H, bottom_up, boundaries):
    """20 000 x 18 000: the input is past 2^32 bytes (4.32 GB), a 32-bit input offset fails.  32 768 x 32 800: 12.9 GB in, 4.3 GB
    out -- the output rows from 32 752 on lie past 2^32 bytes -- a 32-bit output offset fails."""
    import torch
    lib = capi.load_library()
    in_wpc, in_words = 3 * H, 3 * H * Wn
    pitch = Wn * 4 + GAP
    out_words = H * pitch // 4
    assert in_words * 4 > B32 and (Wn < 32768 or H * pitch > B32)
    need = Guarded.need(in_words) + Guarded.need(out_words) + Guarded.need(le.STRIP_COLUMNS * H) + SLACK
    le.require_device_memory(need)
    cols = le.boundary_columns(boundaries, 4 * in_wpc, Wn)
    params, _ = image_params(channels=4, bottom_up=bottom_up)
    T = image_ref.table("srgb")
    what = f"rt_encode_image_device {Wn}x{H}"
    src = dst = small = None
    try:
        src, dst = Guarded(in_words), Guarded(out_words)
        fill_colours(src.body)
        before = le.checksum(src.body)
        capi.check(lib.rt_encode_image_device(0, C.byref(params), Wn, H, src.ptr, dst.ptr, pitch, None))
        torch.cuda.synchronize()
        assert dst.guards_untouched(), f"{what}: a guard word before or after the output was overwritten"
        rows = dst.body.view(H, pitch // 4)
        assert le.count_equal(rows[:, Wn:], le.SENTINEL) == H * GAP // 4, f"{what}: the bytes after a row's end were written"
        assert dst.sentinels_left() == H * GAP // 4, f"{what}: pixels were never written"
        # (b) every byte against the kernel's own strips
        small = Guarded(le.STRIP_COLUMNS * H)
        for x0 in range(0, Wn, le.STRIP_COLUMNS):
            x1 = min(x0 + le.STRIP_COLUMNS, Wn)
            n = x1 - x0
            small.refill()
            capi.check(lib.rt_encode_image_device(0, C.byref(params), n, H, src.ptr + x0 * in_wpc * 4, small.ptr, n * 4, None))
            torch.cuda.synchronize()
            small.assert_written(f"{what}: strip {x0}:{x1}", n * H)
            assert small.sentinels_left() == small.n - n * H, f"{what}: strip {x0}:{x1} was written past its end"
            got, want = rows[:, x0:x1], small.body[:n * H].view(H, n)
            if not torch.equal(got, want):
                bad = (got != want).nonzero()
                r, c = int(bad[0][0]), int(bad[0][1])
                raise AssertionError(f"{what}: columns {x0}:{x1} against their own strip: {len(bad)} pixels differ, first at row {r}, "
                                     f"column {x0 + c} (byte offset {r * pitch + (x0 + c) * 4} of the output): got "
                                     f"0x{int(got[r, c]) & 0xFFFFFFFF:08x}, want 0x{int(want[r, c]) & 0xFFFFFFFF:08x}")
        # (a) the boundary columns against image_ref
        for x in cols:
            column = src.body[x * in_wpc:(x + 1) * in_wpc].cpu().numpy().view(F).reshape(1, H, 3)
            want = image_ref.encode(column, T, 4, 1.0, bool(bottom_up)).reshape(H, 4)
            got = rows[:, x].cpu().numpy().view(np.uint8).reshape(H, 4)
            assert len(np.unique(want[:, :3])) > 250              # (a column exercises the table)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (f"{what}: column {x} against image_ref: {len(bad)} bytes differ, first at row {bad[0][0]}, "
                                   f"channel {bad[0][1]}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
        assert le.checksum(src.body) == before and src.guards_untouched(), f"{what}: the input changed"
    finally:
        for g in (src, dst, small):
            if g is not None:
                g.free()
        rows = got = want = None
        torch.cuda.empty_cache()
