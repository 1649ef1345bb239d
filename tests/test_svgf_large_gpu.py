"""The variance-steered filter (include/rt_svgf.h) on a frame of 16 400 x 16 400 -- 2^28 + 524 544 pixels, the smallest square at
which a 16-byte scratch plane passes 2^32 bytes -- by test_large_composed_gpu.py's ground rules: everything large stays on the
device, every large output and the scratch lie between sentinel guards, the inputs' checksums are the same before and after, and
two references that do not share the addressing under test: svgf_ref on windows of 96 x 96 around every pixel at which a buffer
crosses a multiple of 2^31 bytes, and the same kernels on strips of 1024 columns and their margin, filtered at offset 0 of small
buffers with a small scratch.  Both rest on the filter being local within m = spatial_radius + 2 (2^iterations - 1) pixels on
both axes, which test_limits_cpu.py proves for svgf_ref.

At this frame the records (48 bytes a pixel, 12.9 GB) pass 2^32 three times and every 16-byte plane once; value and out_value
(12 bytes a pixel with three channels, 3.2 GB) cross 2^31 only.  The 18 944^2 frame that would take them past 2^32 needs 54 GB
with the filter's scratch, more than a test may use, so that crossing stays uncovered: the kernels index value and out_value by
the 64-bit pixel number p * channels + c that also indexes the moments."""
import ctypes as C
import time

import numpy as np
import pytest

import large_extents as le
import svgf_ref
from large_extents import Guarded, hashed
from tilecoderaytracer_amd import HostScene, Renderer, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE, svgf_params

pytestmark = pytest.mark.gpu
F = np.float32
B31, B32, B33 = 1 << 31, 1 << 32, 1 << 33
W = H = 16400
N = W * H
WIN = 96
NAMES = ("value", "variance", "estimate")


def scratch_planes(channels, iterations, sigma_l, sigma_plane, pixels):
    """d_scratch as the header describes it and csrc/rt_svgf.hip lays it out: the packed guide (key and aux, 16 bytes a pixel
    each, and with sigma_plane > 0 pnt), one frame of cells {value, variance} (16 bytes a pixel for three channels, 8 for one)
    or two for more than one iteration, and with sigma_l > 0 and one channel the tolerance plane (4), each rounded up to 256
    bytes -> ([(name, offset, bytes a pixel)], total)"""
    planes, at = [], 0
    cell = 16 if channels == 3 else 8
    wanted = [("key", 16), ("aux", 16)] + ([("pnt", 16)] if sigma_plane > 0 else []) + [("cells0", cell)] + \
        ([("cells1", cell)] if iterations > 1 else []) + ([("invl", 4)] if sigma_l > 0 and channels == 1 else [])
    for name, bpp in wanted:
        planes.append((name, at, bpp))
        at += (pixels * bpp + 255) // 256 * 256
    return planes, at


def windows(buffers):
    """buffers: [(bytes a pixel, offset of the first pixel from the buffer's start)] -> (the WIN x WIN windows (x0, z0): the four
    corners and one around every pixel at which a buffer crosses a multiple of 2^31 bytes, those pixels)"""
    spots = {(0, 0), (W - WIN, 0), (0, H - WIN), (W - WIN, H - WIN)}
    crossing = set()
    for bpp, start in buffers:
        for B in range(B31, start + bpp * N, B31):
            if B > start:
                crossing.add((B - start) // bpp)
    for p in sorted(crossing):
        x, z = divmod(p, H)
        spots.add((min(max(x - WIN // 2, 0), W - WIN), min(max(z - WIN // 2, 0), H - WIN)))
    return sorted(spots), sorted(crossing)


def count_different(a, b):
    """how many words of two int32 device tensors differ, a GiB at a time"""
    a, b = a.reshape(-1), b.reshape(-1)
    return sum(int((a[c0:c0 + le.CHUNK_WORDS] != b[c0:c0 + le.CHUNK_WORDS]).sum()) for c0 in range(0, a.numel(), le.CHUNK_WORDS))


def filter_large(channels, outputs, kw):
    """rt_svgf_filter_device over the records of a depth-0 rt_render_gbuffer_device of the built-in scene and hashed values,
    moments and lengths (1..6: both estimate paths at min_history 4); outputs: which of (value, variance, estimate) are asked
    for.  Checks both references and prints the counted conditions and the wall time."""
    import torch
    lib = capi.load_library()
    params = svgf_params(channels, **kw)
    iterations, radius = kw["iterations"], kw["spatial_radius"]
    m = radius + 2 * (2 ** iterations - 1)
    per = (channels, 1, 1)
    planes, scratch_bytes = scratch_planes(channels, iterations, kw["sigma_l"], kw["sigma_plane"], N)
    assert scratch_bytes == int(lib.rt_svgf_scratch_bytes(C.byref(params), W, H))
    strip_cols = le.STRIP_COLUMNS + 2 * m
    strip_scratch = int(lib.rt_svgf_scratch_bytes(C.byref(params), strip_cols, H))
    # (the render's colours, 12 bytes a pixel, are freed before anything but the records is there: they are not in the peak)
    need = Guarded.need(12 * N) + (4 * channels + 8 + 4) * N + sum(Guarded.need(N * k) for k, o in zip(per, outputs) if o) \
        + Guarded.need(scratch_bytes // 4) + sum(Guarded.need(strip_cols * H * k) for k in per) + Guarded.need(strip_scratch // 4) \
        + (3 << 30)
    le.require_device_memory(need)
    what = f"rt_svgf_filter_device {W}x{H} channels {channels} {kw}"
    t0 = time.time()
    host = HostScene.builtin()
    r = Renderer(host)
    bufs = []
    value = moments = length = None
    try:
        hits, colours = Guarded(12 * N), Guarded(3 * N)
        bufs += [hits, colours]
        r.render_gbuffer_device(W, H, 0, 0, W, colours.ptr, hits.ptr)
        torch.cuda.synchronize()
        hits.assert_written("the frame's records")
        colours.free()
        torch.cuda.empty_cache()
        value, moments, length = hashed(channels * N, 1), hashed(2 * N, 4), hashed(N, 3, 5.0, 1.0)
        short = le.count_equal(length < 4.0, True)
        assert 1000 <= short <= N - 1000                            # both estimate paths
        ins = [value.view(torch.int32), hits.body, moments.view(torch.int32), length.view(torch.int32)]
        before = [le.checksum(t) for t in ins]
        out = [Guarded(N * k) if o else None for k, o in zip(per, outputs)]
        scratch = Guarded(scratch_bytes // 4)
        bufs += [g for g in out if g is not None] + [scratch]

        def call(x0, x1, ptrs, scratch_ptr):
            capi.check(lib.rt_svgf_filter_device(0, C.byref(params), x1 - x0, H, value.data_ptr() + x0 * H * 4 * channels,
                                                 hits.ptr + x0 * H * 48, moments.data_ptr() + x0 * H * 8, length.data_ptr() + x0 * H * 4,
                                                 *ptrs, scratch_ptr, None))

        call(0, W, [g.ptr if g is not None else None for g in out], scratch.ptr)
        torch.cuda.synchronize()
        for g, name in zip(out, NAMES):
            if g is not None:
                g.assert_written(f"{what}, {name}")
        assert scratch.guards_untouched(), f"{what}: a word beside the scratch was written"
        changed = count_different(out[0].body, ins[0])
        assert changed >= N // 10, f"{what}: only {changed} words of the value were filtered"    # not all pass-through
        # (1) windows against svgf_ref
        buffers = [(4 * channels, 0), (48, 0), (8, 0), (4, 0)] + [(bpp, off) for _, off, bpp in planes]
        spots, crossing = windows(buffers)
        assert len(spots) >= 10 and (W - WIN, H - WIN) in spots
        for p in (B32 // 48, B32 // 16):                            # the records' and the key plane's 2^32
            px, pz = divmod(p, H)
            assert p < N and any(x0 <= px < x0 + WIN and z0 <= pz < z0 + WIN for x0, z0 in spots), (px, pz)
        views = [value.view(W, H, channels), hits.body.view(W, H, 12), moments.view(W, H, 2), length.view(W, H)]
        big = [g.body.view(W, H, k) if g is not None else None for g, k in zip(out, per)]
        filtered = spatial = 0
        for x0, z0 in spots:
            cx0, cx1, cz0, cz1 = max(x0 - m, 0), min(x0 + WIN + m, W), max(z0 - m, 0), min(z0 + WIN + m, H)
            c_value, c_hits, c_moments, c_length = (np.ascontiguousarray(v[cx0:cx1, cz0:cz1].cpu().numpy()) for v in views)
            c_hits = c_hits.view(HIT_DTYPE).reshape(cx1 - cx0, cz1 - cz0)
            c_value = c_value if channels == 3 else c_value[..., 0]
            want = svgf_ref.svgf(c_value, c_hits, c_moments, c_length, **kw)
            inner = (slice(x0 - cx0, x0 - cx0 + WIN), slice(z0 - cz0, z0 - cz0 + WIN))
            for g, w, name in zip(big, want, NAMES):
                if g is None:
                    continue
                got = np.ascontiguousarray(g[x0:x0 + WIN, z0:z0 + WIN].cpu().numpy()).view(F).reshape(w[inner].shape)
                assert svgf_ref.same_bits(got, w[inner]), \
                    f"{what}: {name} of the window at ({x0}, {z0}) differs from svgf_ref in " \
                    f"{int((got.view(np.uint32) != np.ascontiguousarray(w[inner]).view(np.uint32)).sum())} words"
            filtered += int((np.ascontiguousarray(want[0][inner]).view(np.uint32) != np.ascontiguousarray(c_value[inner]).view(np.uint32)).sum())
            spatial += int(((c_length[inner] < 4) & ~svgf_ref.dead_records(c_hits[inner])).sum())
        assert filtered >= 1000 and spatial >= 1000, (filtered, spatial)
        # (2) every word against strips with their margin, at offset 0 of small buffers
        small = [Guarded(strip_cols * H * k) for k in per]
        small_scratch = Guarded(strip_scratch // 4)
        bufs += small + [small_scratch]
        for x0 in range(0, W, le.STRIP_COLUMNS):
            x1 = min(x0 + le.STRIP_COLUMNS, W)
            a, b = max(x0 - m, 0), min(x1 + m, W)
            for s in small:
                s.refill()
            call(a, b, [s.ptr if g is not None else None for s, g in zip(small, out)], small_scratch.ptr)
            torch.cuda.synchronize()
            assert small_scratch.guards_untouched(), f"{what}: a word beside the scratch of strip {a}:{b} was written"
            for k, (g, s, name) in enumerate(zip(out, small, NAMES)):
                if g is None:
                    assert s.sentinels_left() == s.n and s.guards_untouched()
                    continue
                words, wpc = (b - a) * H * per[k], H * per[k]
                s.assert_written(f"{what}: {name} of strip {a}:{b}", words)
                assert s.sentinels_left() == s.n - words, f"{what}: {name} of strip {a}:{b} was written past its end"
                text = le.device_difference(g.body[x0 * wpc:x1 * wpc], s.body[(x0 - a) * wpc:(x1 - a) * wpc], wpc,
                                            f"{what}: {name}, columns {x0}:{x1} against their own strip", x0)
                assert text is None, text
        assert [le.checksum(t) for t in ins] == before, f"{what}: an input changed"
        assert all(g.guards_untouched() for g in out if g is not None) and hits.guards_untouched() and scratch.guards_untouched()
        print(f"[large svgf] {what}: scratch {scratch_bytes} bytes, {len(spots)} windows over {len(crossing)} crossings, "
              f"{changed} of {channels * N} value words filtered, {short} of {N} lengths below min_history, {time.time() - t0:.1f} s")
        return planes, scratch_bytes
    finally:
        for g in bufs:
            g.free()
        value = moments = length = ins = views = big = None
        torch.cuda.empty_cache()
        r.close()


def test_three_channels_two_iterations_where_the_second_cells_frame_begins_past_2_33_bytes():
    """Run A: three channels, two iterations (steps 1 and 2), the luminance term with the prefilter made inside the iteration
    kernel, no plane term, spatial_radius 1, out_variance asked for and out_estimate NULL.  The scratch is key, aux and two frames
    of 16-byte cells, 4 x 4.3 GB: every plane passes 2^32 bytes within itself, and the second cells frame BEGINS 12.9 GB -- more
    than 2^33 bytes -- behind d_scratch.  152 bytes a pixel, 41 GB.
    The one-line narrowings this is there for (derived from the code; no narrowed kernel was built or run):
      `(uint32_t)(16 * base)` for `base * 16` in the a-trous row pointers kb, xb_ and cb: every tap row from pixel 2^28 on --
        columns 16 368 to 16 399 -- is read 2^32 bytes too low, inside the planes; the windows at the last corners and around the
        planes' 2^32 differ from svgf_ref, and the last strip, whose own offsets are small, from the frame;
      `3 * p` without its cast in rt_svgf_pack_kernel counts 16-byte words and stays below 2^32 at every size the call accepts;
        a BYTE offset there, `(uint32_t)(48 * p)`, packs the guide of pixel 89 478 486 (column 5456) and every later one from
        records 2^32 bytes too low, and every window and strip from there on differs;
      value and out_value, `p * kC + c`, cross 2^31 bytes only (the window there) and no 2^32 -- see the module's docstring;
      `(uint32_t)s.cells[1]` in enqueue(), 12.9 GB modulo 2^32, puts the second frame of cells over the key plane: iteration 0
        overwrites the guide iteration 1 still reads, and every window differs."""
    kw = dict(iterations=2, sigma_l=2.0, sigma_plane=0.0, min_history=4, spatial_radius=1, normal_squarings=1, match_color=False)
    planes, total = filter_large(3, (True, True, False), kw)
    assert total >= 4 * 16 * N
    assert [name for name, _, _ in planes] == ["key", "aux", "cells0", "cells1"] and planes[3][1] > B33


def test_one_channel_with_the_plane_term_the_prefilter_pass_and_the_estimate():
    """Run B: one channel, one iteration, the luminance term with the prefilter pass of its own and its invl plane, the plane term
    and its pnt plane, spatial_radius 3, all three outputs.  The scratch is key, aux, pnt (16 bytes a pixel, each passing 2^32
    within itself, pnt beginning 8.6 GB behind d_scratch), 8-byte cells and the 4-byte invl plane beginning 15 GB behind it.
    136 bytes a pixel, 37 GB.
    The one-line narrowings this is there for (derived from the code; no narrowed kernel was built or run):
      `(uint32_t)(16 * base)` in the a-trous row pointer pb: the plane term compares with other pixels' points from pixel 2^28 on;
      `(uint32_t)(base * sizeof(Cell))` in cb wraps only at 2^29 pixels of 8-byte cells and is right here;
      `(uint32_t)s.invl` in enqueue(), 15 GB modulo 2^32, puts the tolerances into the pnt plane, which the iteration then reads
        as points: every window differs;
      the prefilter's and the estimate's own indices -- `invl[x64 * (int64_t)H + z64]`, `var[q * kWords]`, `moments[q]`, `key[q]`
        -- count elements and fit 32 bits at every size the call accepts; a byte offset in 32 bits wraps at the key plane's 2^32
        (pixel 2^28) and, with `(int32_t)`, at the moments' 2^31 (the same pixel), where a window lies."""
    kw = dict(iterations=1, sigma_l=2.0, sigma_plane=0.4, min_history=4, spatial_radius=3, normal_squarings=3, match_color=True)
    planes, total = filter_large(1, (True, True, True), kw)
    assert [name for name, _, _ in planes] == ["key", "aux", "pnt", "cells0", "invl"] and planes[4][1] > 3 * B32
