"""Kernel addressing past 2^31 and 2^32 bytes, more than 2^31 pixels in one launch, and the host-side size thresholds, on the GPU.
Every comparison is bit-exact.  Each large output lies between two guards of 1 MiB inside one tensor, all of it filled with a
NaN-payload sentinel (large_extents.Guarded): after the launch the guards still hold it and no output word does.  Two references,
neither sharing the addressing under test:
  (a) the C oracle, query_ref, soft_ref / refract_ref or denoise_ref on the column that straddles each byte boundary, its two
      neighbours, column 0 and the last column (large_extents.boundary_columns, computed from H);
  (b) the same kernel's strips of at most 1024 columns, each rendered at offset 0 of a small buffer and compared on the device
      with the matching slice of the large output -- every word of it.
Everything large stays on the device; only columns and crops come to the host.  Every test computes its device-memory need first
and skips only if less than 1.1 x that is free; none needs more than 48 GB.

Sizes the oracle's ints and the Python side were tried with on the CPU first: W = 2^30 and H = 2^24 + 4096 are plain ints for both
(orc_render indexes its output in size_t), so no case of the issue had to be dropped."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import denoise_ref
import kernel_matrix as km
import large_extents as le
import oracle_lib as oracle
import query_ref
import refract_ref
import soft_ref
from large_extents import Guarded
from ssaa_ref import box_filter
from test_denoise_gpu import soft_renderer
from test_kernel_matrix_gpu import ray_batch, segments, world
from test_query_gpu import assert_hits_same
from test_refract_gpu import glass_builtin, make as make_refractive, ref_scene as glass_ref_scene
from test_texture_gpu import Desc
from tilecoderaytracer_amd import HostScene, Renderer, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

pytestmark = pytest.mark.gpu
F = np.float32
B31, B32, B33, B34 = 1 << 31, 1 << 32, 1 << 33, 1 << 34
SLACK = 3 << 30                          # the comparisons' temporaries: a few GiB-sized chunks at a time


@pytest.fixture(autouse=True)
def measured(request):
    """each test's wall time and peak device memory, printed (pytest -rA shows them)"""
    import torch
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"[large extents] {request.node.name}: {time.time() - t0:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    torch.cuda.empty_cache()


def sync():
    import torch
    torch.cuda.synchronize()


def assert_reference_columns(big, wpc, cols, reference, what):
    """ground rule (a): columns `cols` of the int32 device view `big` (wpc words a column) against reference(x0, x1), a numpy
    array of the run's words (any 4-byte dtype)"""
    for x0, x1 in le.runs(cols):
        got = big[x0 * wpc:x1 * wpc].cpu().numpy()
        want = np.ascontiguousarray(reference(x0, x1)).reshape(-1).view(np.int32)
        d = le.first_difference(got, want)
        assert d is None, (f"{what}: columns {x0}:{x1} against the reference: {d[3]} words differ, first in column "
                           f"{x0 + d[0] // wpc}, word {d[0] % wpc} of it: got 0x{d[1] & 0xFFFFFFFF:08x}, want 0x{d[2] & 0xFFFFFFFF:08x}")


def launched_into(words, launch, what):
    """launch(address) into a guarded buffer of `words` int32 words -> the words on the host, after the guard and sentinel checks"""
    g = Guarded(words)
    try:
        launch(g.ptr)
        sync()
        g.assert_written(what)
        return g.body.cpu().numpy()
    finally:
        g.free()


# ---- 1. colours past 2^32 bytes -------------------------------------------------------------------------------------------------

def test_colours_past_2_32_bytes_device_and_host_paths():
    """rt_render_device, 20 000 x 18 000 (4.32 GB): (b) over every word, (a) on the columns around 2^31 and 2^32 bytes, the first
    and the last.  Then rt_render of the same frame into host memory (the handle's framebuffer, the download's byte count): its
    boundary columns and every 97th column equal the device frame's."""
    import torch
    W, H, depth = 20000, 18000, 2
    wpc, words = 3 * H, 3 * H * W
    assert words * 4 > B32
    need = Guarded.need(words) + Guarded.need(le.STRIP_COLUMNS * wpc) + words * 4 + SLACK     # (rt_render's own framebuffer)
    le.require_device_memory(need)
    cols = le.boundary_columns([B31, B32], 4 * wpc, W)
    r, o, big, host = Renderer(HostScene.builtin()), oracle.OracleScene.builtin(), None, None
    what = f"rt_render_device {W}x{H}"
    try:
        big = Guarded(words)
        r.render_device(W, H, depth, 0, W, big.ptr)
        sync()
        big.assert_written(what)
        le.assert_columns_equal_strips(lambda x0, x1, ptr: r.render_device(W, H, depth, x0, x1, ptr), [(big.body, wpc)], W, what)
        assert_reference_columns(big.body, wpc, cols, lambda x0, x1: o.render(W, H, depth, x0, x1), what)
        host = np.full(words, le.SENTINEL, dtype=np.int32)
        capi.check(capi.load_library().rt_render(r._scene, r._cam, W, H, 0, W, depth, host.ctypes.data))
        assert int(np.count_nonzero(host == le.SENTINEL)) == 0, "rt_render left words of the host image unwritten"
        for x in sorted(set(cols) | set(range(0, W, 97))):
            d = le.first_difference(host[x * wpc:(x + 1) * wpc], big.body[x * wpc:(x + 1) * wpc].cpu().numpy())
            assert d is None, f"rt_render {W}x{H}: column {x} differs from rt_render_device's, first at word {d[0]} of it ({d[3]} words)"
        assert big.guards_untouched()
    finally:
        del host
        if big is not None:
            big.free()
        r.close()
        torch.cuda.empty_cache()


# ---- 2. more than 2^31 pixels in one launch ----------------------------------------------------------------------------------------

def test_more_than_2_31_pixels_in_one_launch():
    """46 400 x 46 400 = 2 152 960 000 pixels, 25.8 GB: (b) over every word; (a) on the columns around 2^31, 2^32, 2^33 and 2^34 bytes,
    around the pixel whose number is 2^31 (byte 12 x 2^31), the first and the last"""
    import torch
    W = H = 46400
    depth = 2
    wpc, words = 3 * H, 3 * H * W
    assert W * H > B31 and words * 4 > B34
    need = Guarded.need(words) + Guarded.need(le.STRIP_COLUMNS * wpc) + SLACK
    le.require_device_memory(need)
    cols = le.boundary_columns([B31, B32, B33, B34, 12 * B31], 4 * wpc, W)
    assert (B31 // H) in cols                                # the column in which the pixel count passes 2^31
    r, o, big = Renderer(HostScene.builtin()), oracle.OracleScene.builtin(), None
    what = f"rt_render_device {W}x{H}"
    try:
        big = Guarded(words)
        r.render_device(W, H, depth, 0, W, big.ptr)
        sync()
        big.assert_written(what)
        le.assert_columns_equal_strips(lambda x0, x1, ptr: r.render_device(W, H, depth, x0, x1, ptr), [(big.body, wpc)], W, what)
        assert_reference_columns(big.body, wpc, cols, lambda x0, x1: o.render(W, H, depth, x0, x1), what)
        assert big.guards_untouched()
    finally:
        if big is not None:
            big.free()
        r.close()
        torch.cuda.empty_cache()


# ---- 3. records past 2^32 bytes ---------------------------------------------------------------------------------------------------

GB_SIDE, GB_DEPTH = 16400, 2


def soft_builtin_references():
    """the built-in scene with both lights one-sample area lights of radius 1.0, seed 1 (test_denoise_gpu.soft_renderer): its
    colours (soft_ref) and records (query_ref) of columns [x0, x1) of a W x H frame"""
    o = oracle.OracleScene.builtin()
    lights = [i for i in range(o.object_count) if o.get_object(i).is_light]
    scene, query, cam = soft_ref.Scene(o, {k: (1, 1.0) for k in lights}, seed=1), query_ref.Scene(o), HostScene.builtin().camera

    def colours(W, H, depth, x0, x1):
        return soft_ref.trace(scene, le.column_rays(cam, W, H, x0, x1), depth, le.column_keys(H, x0, x1))

    def records(W, H, x0, x1):
        return query_ref.intersect(query, le.column_rays(cam, W, H, x0, x1))

    return colours, records


def test_gbuffer_records_past_2_32_bytes():
    """rt_render_gbuffer_device, 16 400 x 16 400: 12.9 GB of records, 3.2 GB of colours.  Both against strips on the device; the
    records against query_ref and the colours against soft_ref on the columns around the RECORDS' 2^31, 2^32 and 2^33 bytes
    (stride 48 H) and around the colours' 2^31 bytes (stride 12 H), the first and the last."""
    import torch
    W = H = GB_SIDE
    depth = GB_DEPTH
    cw, hw = 3 * H, 12 * H
    assert hw * W * 4 > B33 and cw * W * 4 > B31
    need = Guarded.need(cw * W) + Guarded.need(hw * W) + Guarded.need(le.STRIP_COLUMNS * cw) + Guarded.need(le.STRIP_COLUMNS * hw) + SLACK
    le.require_device_memory(need)
    record_cols = le.boundary_columns([B31, B32, B33], 4 * hw, W)
    colour_cols = sorted(set(record_cols) | set(le.boundary_columns([B31], 4 * cw, W)))
    colours, records = soft_builtin_references()
    r, rgb, hits = soft_renderer("builtin"), None, None
    what = f"rt_render_gbuffer_device {W}x{H}"
    try:
        rgb, hits = Guarded(cw * W), Guarded(hw * W)
        r.render_gbuffer_device(W, H, depth, 0, W, rgb.ptr, hits.ptr)
        sync()
        rgb.assert_written(what + " colours")
        hits.assert_written(what + " records")
        le.assert_columns_equal_strips(lambda x0, x1, p_rgb, p_hits: r.render_gbuffer_device(W, H, depth, x0, x1, p_rgb, p_hits),
                                       [(rgb.body, cw), (hits.body, hw)], W, what)
        for x0, x1 in le.runs(record_cols):
            got = hits.body[x0 * hw:x1 * hw].cpu().numpy().view(HIT_DTYPE).reshape(x1 - x0, H)
            assert_hits_same(got, records(W, H, x0, x1), f"{what}: records of columns {x0}:{x1}")
        assert_reference_columns(rgb.body, cw, colour_cols, lambda x0, x1: colours(W, H, depth, x0, x1), what + " colours")
        assert rgb.guards_untouched() and hits.guards_untouched()
    finally:
        for g in (rgb, hits):
            if g is not None:
                g.free()
        r.close()
        torch.cuda.empty_cache()


# ---- 4. ray batches past 2^32 bytes in and out -------------------------------------------------------------------------------------

def tiled(base, n):
    """a device tensor (M, k) repeated along its first axis to n rows: row i is base[i % M]"""
    M = base.shape[0]
    return base.repeat(-(-n // M), 1)[:n]


def coprime_prefix(*arrays):
    """the arrays cut to the largest common length M that is coprime to 64 (odd): tiles of M never align with the wavefront's 64"""
    M = len(arrays[0])
    M -= 1 - (M & 1)
    assert M > 64 and math.gcd(M, 64) == 1
    return [a[:M] for a in arrays]


def trace_tiled(n, row_counts):
    """rt_trace_rays_device of n rays -- test_kernel_matrix_gpu's batch of the built-in scene (M rays, M odd) tiled on the device --
    against soft_ref's colours of the M rays tiled the same way, so every output word is compared; once per row count"""
    import torch
    rays, want, _ = coprime_prefix(*ray_batch("builtin", ""))
    depth = km.DEPTH
    need = n * 24 + Guarded.need(3 * n) + n * 12 + SLACK
    le.require_device_memory(need)
    r, out = world("builtin", "").renderer({}), None
    try:
        d_rays = tiled(torch.from_numpy(rays).cuda(), n)
        expected = tiled(torch.from_numpy(np.ascontiguousarray(want).view(np.int32)).cuda(), n).reshape(-1)
        assert d_rays.is_contiguous() and expected.is_contiguous() and d_rays.shape == (n, 6)
        out = Guarded(3 * n)
        for rows in row_counts:
            what = f"rt_trace_rays_device n={n} rows={rows}"
            out.refill()
            r.trace_rays_device(n, rows, d_rays.data_ptr(), depth, out.ptr)
            sync()
            out.assert_written(what)
            text = le.device_difference(out.body, expected, 3, what + " (a column is a ray)")
            assert text is None, text
    finally:
        if out is not None:
            out.free()
        d_rays = expected = None
        r.close()
        torch.cuda.empty_cache()


def test_trace_rays_past_2_32_bytes_in_and_out_three_row_counts():
    """370 000 037 rays: 8.88 GB in (past 2^33), 4.44 GB of colours out (past 2^32).  rows = n (one column), a power of two, an odd
    number near 1e4.  What crosses 2^32 here is the BYTE offset; the element indices (6 n = 2.2e9 floats in, 3 n = 1.1e9 out) still
    fit 32 bits."""
    n = 370000037
    assert n * 24 > B33 and n * 12 > B32 and n * 6 < B32
    trace_tiled(n, (n, 1 << 15, 9973))


def test_trace_rays_ray_index_times_six_past_2_32():
    """720 000 011 rays, 17.3 GB in, 8.6 GB out: the input's element index `ray * 6` itself passes 2^32 floats (4.3e9), so a 32-bit
    product in batch_ray() or render_tile()'s read would wrap here; the output's byte offset passes 2^33."""
    n = 720000011
    assert n * 6 > B32 and n * 12 > B33
    trace_tiled(n, (1 << 15,))


def test_intersect_rays_records_past_2_32_bytes():
    """100 000 007 rays: 4.8 GB of records, compared as words with query_ref's records of the M rays, tiled"""
    import torch
    rays, _, recs = coprime_prefix(*ray_batch("builtin", ""))
    r = world("builtin", "").renderer({})
    n = 100000007
    assert n * 48 > B32 and n * 24 > B31
    le.require_device_memory(n * 24 + Guarded.need(12 * n) + n * 48 + SLACK)
    out = None
    try:
        assert_hits_same(r.intersect_rays(rays), recs, "the M rays on their own")       # (and so: no NaN to excuse below)
        words = np.ascontiguousarray(recs).view(np.int32).reshape(len(recs), 12)
        assert not np.isnan(words.view(F)[:, 1:11]).any()
        d_rays = tiled(torch.from_numpy(rays).cuda(), n)
        expected = tiled(torch.from_numpy(words).cuda(), n).reshape(-1)
        out = Guarded(12 * n)
        for rows in (n, 4099):
            what = f"rt_intersect_rays_device n={n} rows={rows}"
            out.refill()
            r.intersect_rays_device(n, rows, d_rays.data_ptr(), out.ptr)
            sync()
            out.assert_written(what)
            text = le.device_difference(out.body, expected, 12, what + " (a column is a ray)")
            assert text is None, text
    finally:
        if out is not None:
            out.free()
        d_rays = expected = None
        r.close()
        torch.cuda.empty_cache()


def test_occluded_rays_segments_past_2_32_bytes_in():
    """370 000 037 segments, 8.88 GB in, one byte each out: the verdicts of query_ref.occluded of the M segments, tiled"""
    import torch
    segs, want = coprime_prefix(*segments("builtin", ""))
    n = 370000037
    le.require_device_memory(n * 24 + Guarded.need(n, as_bytes=True) + n + SLACK)
    r, out = world("builtin", "").renderer({}), None
    try:
        assert 0 < want.sum() < len(want)
        d_segs = tiled(torch.from_numpy(segs).cuda(), n)
        expected = tiled(torch.from_numpy(want.astype(np.uint8)[:, None]).cuda(), n).reshape(-1)
        out = Guarded(n, as_bytes=True)
        for rows in (n, 8191):
            what = f"rt_occluded_rays_device n={n} rows={rows}"
            out.refill()
            r.occluded_rays_device(n, rows, d_segs.data_ptr(), out.ptr)
            sync()
            out.assert_written(what)
            if not torch.equal(out.body, expected):
                bad = (out.body != expected).nonzero()
                raise AssertionError(f"{what}: {len(bad)} verdicts differ, first at segment {int(bad[0])}: got {int(out.body[int(bad[0])])}")
    finally:
        if out is not None:
            out.free()
        d_segs = expected = None
        r.close()
        torch.cuda.empty_cache()


def test_trace_rays_clustered_field_past_2_32_bytes_in():
    """the clustered field through rt_render_kernel_clusters_rays: 180 000 017 rays, 4.32 GB in, 2.16 GB out"""
    import torch
    case = [c for c in km.CASES if c.mode == "_clusters" and c.call == "rays" and c.shading == ""][0]
    rays, want, _ = coprime_prefix(*ray_batch(case.scene, case.shading))
    n, depth = 180000017, km.DEPTH
    assert n * 24 > B32 and n * 12 > B31
    le.require_device_memory(n * 24 + Guarded.need(3 * n) + n * 12 + SLACK)
    r, out = world(case.scene, case.shading).renderer(case.options), None
    try:
        d_rays = tiled(torch.from_numpy(rays).cuda(), n)
        expected = tiled(torch.from_numpy(np.ascontiguousarray(want).view(np.int32)).cuda(), n).reshape(-1)
        out = Guarded(3 * n)
        what = f"rt_trace_rays_device (clustered field) n={n}"
        r.trace_rays_device(n, 1 << 14, d_rays.data_ptr(), depth, out.ptr)
        sync()
        assert r.kernel_name() == km.kernel_name(case) and "_clusters" in r.kernel_name(), r.kernel_name()
        out.assert_written(what)
        text = le.device_difference(out.body, expected, 3, what + " (a column is a ray)")
        assert text is None, text
    finally:
        if out is not None:
            out.free()
        d_rays = expected = None
        r.close()
        torch.cuda.empty_cache()


# ---- 5. the PRIMARY threshold and its 16-bit rectangles ----------------------------------------------------------------------------

PRIMARY_FRAMES = [(30000, 64, 0, 30000), (30001, 64, 0, 30001), (64, 30000, 0, 64), (64, 30001, 0, 64),
                  (29999, 29999, 0, 16), (29999, 29999, 14992, 15008), (29999, 29999, 29983, 29999)]


@pytest.mark.parametrize("W, H, x0, x1", PRIMARY_FRAMES)
def test_primary_table_on_both_sides_of_its_threshold(W, H, x0, x1):
    """the built-in scene (the PRIMARY table's scene) where primary_table() clamps its 16-bit rectangles and gives up beyond
    30 000: the whole output against the oracle, and once more with the table off"""
    depth, words = 2, 3 * H * (x1 - x0)
    le.require_device_memory(2 * Guarded.need(words) + SLACK)
    r = Renderer(HostScene.builtin())
    try:
        want = oracle.OracleScene.builtin().render(W, H, depth, x0, x1).reshape(-1).view(np.int32)
        for primary in (1, 0):
            r.set_option("primary", primary)
            what = f"rt_render_device {W}x{H} columns {x0}:{x1}, primary={primary}"
            got = launched_into(words, lambda ptr: r.render_device(W, H, depth, x0, x1, ptr), what)
            d = le.first_difference(got, want)
            assert d is None, f"{what}: {d[3]} words differ from the oracle's, first at column {x0 + d[0] // (3 * H)}, word {d[0] % (3 * H)}"
    finally:
        r.close()


@pytest.mark.parametrize("k, W, H", [(4, 7500, 16), (4, 7501, 16), (2, 16, 15000), (2, 16, 15001)])
def test_primary_threshold_through_supersampling(k, W, H):
    """rt_render_ssaa_device whose VIRTUAL size k W x k H crosses 30 000 (30 000 and 30 004 wide; 30 000 and 30 002 high) against
    the box-filtered oracle frame of that size, and once more with the table off"""
    depth, words = 2, 3 * H * W
    le.require_device_memory(2 * Guarded.need(words) + SLACK)
    r = Renderer(HostScene.builtin())
    try:
        want = box_filter(oracle.OracleScene.builtin().render(k * W, k * H, depth), k).reshape(-1).view(np.int32)
        for primary in (1, 0):
            r.set_option("primary", primary)
            what = f"rt_render_ssaa_device {W}x{H} k={k}, primary={primary}"
            got = launched_into(words, lambda ptr: r.render_ssaa_device(W, H, depth, k, 0, W, ptr), what)
            d = le.first_difference(got, want)
            assert d is None, f"{what}: {d[3]} words differ from the filtered oracle frame, first at column {d[0] // (3 * H)}, word {d[0] % (3 * H)}"
            assert r.kernel_name().endswith("_ssaa"), r.kernel_name()
    finally:
        r.close()


# ---- 6. pixel numbers a float cannot hold -----------------------------------------------------------------------------------------

W24 = (1 << 24) + 4096
FLOAT_FRAMES = [(W24, 64, (1 << 24) - 8, (1 << 24) + 8), (W24, 64, W24 - 16, W24), (64, W24, 31, 33), (1 << 30, 64, (1 << 30) - 8, 1 << 30)]


@pytest.mark.parametrize("W, H, x0, x1", FLOAT_FRAMES)
def test_pixel_numbers_above_2_24_round_as_the_oracles(W, H, x0, x1):
    """(float)x and (float)z are inexact above 2^24: neighbouring pixels share a ray, and the kernel must round as the oracle's
    `((float)x) / W` does"""
    depth, words = 2, 3 * H * (x1 - x0)
    le.require_device_memory(2 * Guarded.need(words) + SLACK)
    r = Renderer(HostScene.builtin())
    try:
        what = f"rt_render_device {W}x{H} columns {x0}:{x1}"
        got = launched_into(words, lambda ptr: r.render_device(W, H, depth, x0, x1, ptr), what)
        want = oracle.OracleScene.builtin().render(W, H, depth, x0, x1).reshape(-1).view(np.int32)
        d = le.first_difference(got, want)
        assert d is None, f"{what}: {d[3]} words differ from the oracle's, first at column {x0 + d[0] // (3 * H)}, word {d[0] % (3 * H)}"
    finally:
        r.close()


# ---- 7. the denoiser past 2^32 bytes a plane ---------------------------------------------------------------------------------------

def denoise_windows(W, H, side, plane_bytes, planes):
    """96 x 96 windows (x0, z0): the four corners (the last pixel is in one), and one around every pixel at which a buffer crosses a
    multiple of 2^31 bytes -- rgb and the output (12 bytes a pixel), the records (48), and the scratch planes (16 a pixel, plane k
    at k x plane_bytes from the scratch's start: the guide's two, then the colour planes)"""
    pixels = W * H
    spots = {(0, 0), (W - side, 0), (0, H - side), (W - side, H - side)}
    crossing = set()
    for bpp, start in [(12, 0), (48, 0)] + [(16, k * plane_bytes) for k in range(planes)]:
        for B in range(B31, start + bpp * pixels, B31):
            if B > start:
                crossing.add((B - start) // bpp)
    for p in sorted(crossing):
        x, z = divmod(p, H)
        spots.add((min(max(x - side // 2, 0), W - side), min(max(z - side // 2, 0), H - side)))
    return sorted(spots), sorted(crossing)


@pytest.mark.parametrize("side, runs, rgb_crosses", [(GB_SIDE, [(3, 1.0, 3), (1, 0.0, 3)], False), (18944, [(1, 0.0, 3)], True)])
def test_denoiser_past_2_32_bytes_a_plane(side, runs, rgb_crosses):
    """rt_denoise_device on a one-sample soft-shadow G-buffer frame of the built-in scene (case 3's frame, rendered here again).
    16 400^2: 2^28 + 524 544 pixels -- every 16-byte scratch plane exceeds 4 GiB, the records are 12.9 GB -- with 3 iterations, sigma
    1.0, 3 squarings, and again with 1 iteration, sigma 0.  rgb and the output (12 bytes a pixel) cross only 2^31 there, so a frame of
    18 944^2 (4.31 GB of colours, 17.2 GB of records) is filtered with 1 iteration, which is what fits 48 GB.  The filter is local
    within m = 2 (2^iterations - 1) pixels on both axes (test_limits_cpu.py proves it for denoise_ref): windows of 96 x 96 at the
    corners and around every pixel at which rgb, the output, the records or a scratch plane crosses a multiple of 2^31 bytes,
    copied to the host with a margin of m clipped at the frame's edges, filtered by denoise_ref and compared on the window.  The
    inputs' checksums are the same before and after."""
    import torch
    lib = capi.load_library()
    W = H = side
    pixels, depth, win = W * H, GB_DEPTH, 96
    assert pixels > (1 << 28)
    params = [capi.RtDenoiseParams(it, sq, sigma) for it, sigma, sq in runs]
    scratch_bytes = max(int(lib.rt_denoise_scratch_bytes(C.byref(p), W, H)) for p in params)
    assert scratch_bytes >= 3 * 16 * pixels
    plane = (pixels * 16 + 255) // 256 * 256
    need = 2 * Guarded.need(3 * pixels) + Guarded.need(12 * pixels) + scratch_bytes + SLACK
    le.require_device_memory(need)
    r, rgb, hits, out, scratch = soft_renderer("builtin"), None, None, None, None
    try:
        rgb, hits, out = Guarded(3 * pixels), Guarded(12 * pixels), Guarded(3 * pixels)
        scratch = torch.empty(((scratch_bytes + 15) // 16 * 4,), dtype=torch.int32, device="cuda")
        r.render_gbuffer_device(W, H, depth, 0, W, rgb.ptr, hits.ptr)
        sync()
        rgb.assert_written("the frame's colours")
        hits.assert_written("the frame's records")
        before = le.checksum(rgb.body), le.checksum(hits.body)
        rgb3, hits12, out3 = rgb.body.view(W, H, 3), hits.body.view(W, H, 12), out.body.view(W, H, 3)
        for p, (iterations, sigma, squarings) in zip(params, runs):
            what = f"rt_denoise_device {W}x{H} it{iterations} sigma{sigma} k{squarings}"
            out.refill()
            scratch.fill_(le.SENTINEL)
            capi.check(lib.rt_denoise_device(0, C.byref(p), W, H, rgb.ptr, hits.ptr, out.ptr, scratch.data_ptr(), None))
            sync()
            out.assert_written(what)
            m = 2 * (2 ** iterations - 1)
            spots, crossing = denoise_windows(W, H, win, plane, 4 if iterations > 1 else 3)
            assert len(spots) >= 6 and (W - win, H - win) in spots
            # a window sits on the very pixel at which each buffer crosses 2^32 bytes: the records and the first scratch plane in
            # both frames, rgb and the output (12 bytes a pixel) in the larger one, which exists for that crossing
            assert (12 * pixels > B32) == rgb_crosses and 48 * pixels > B32 and 16 * pixels > B32
            for bpp in (12, 48, 16) if rgb_crosses else (48, 16):
                px, pz = divmod(B32 // bpp, H)
                assert any(x0 <= px < x0 + win and z0 <= pz < z0 + win for x0, z0 in spots), (bpp, px, pz)
            filtered = 0
            for x0, z0 in spots:
                cx0, cx1, cz0, cz1 = max(x0 - m, 0), min(x0 + win + m, W), max(z0 - m, 0), min(z0 + win + m, H)
                c_rgb = rgb3[cx0:cx1, cz0:cz1].cpu().numpy().view(F)
                c_hits = np.ascontiguousarray(hits12[cx0:cx1, cz0:cz1].cpu().numpy()).view(HIT_DTYPE).reshape(cx1 - cx0, cz1 - cz0)
                want = denoise_ref.denoise(c_rgb, c_hits, iterations, sigma, squarings)[x0 - cx0:x0 - cx0 + win, z0 - cz0:z0 - cz0 + win]
                got = out3[x0:x0 + win, z0:z0 + win].cpu().numpy().view(F)
                assert denoise_ref.same_bits(got, want), \
                    f"{what}: the window at ({x0}, {z0}) differs from denoise_ref in {int((got.view(np.uint32) != want.view(np.uint32)).sum())} words"
                filtered += int((got.view(np.uint32) != c_rgb[x0 - cx0:x0 - cx0 + win, z0 - cz0:z0 - cz0 + win].view(np.uint32)).any())
            assert filtered >= 1                              # (the windows are not all pass-through)
            assert (le.checksum(rgb.body), le.checksum(hits.body)) == before, f"{what}: the inputs changed"
            assert rgb.guards_untouched() and hits.guards_untouched()
    finally:
        for g in (rgb, hits, out):
            if g is not None:
                g.free()
        scratch = rgb3 = hits12 = out3 = None
        r.close()
        torch.cuda.empty_cache()


# ---- 8. the HBM bounce stack past 2^32 bytes ---------------------------------------------------------------------------------------

def stack_bytes(li, depth, quads):
    return li.grid_blocks * li.block_threads * (depth + 1) * 16 * quads


def twomirrors_case():
    o = oracle.OracleScene.named("twomirrors")
    return Renderer(HostScene.named("twomirrors")), 1, lambda W, H, depth, x0, x1: o.render(W, H, depth, x0, x1)


def glass_case():
    host, o = HostScene.builtin(), oracle.OracleScene.builtin()
    refr = glass_builtin(host)
    d = Desc(host)
    rs = glass_ref_scene(o, glass_builtin(o))
    return (make_refractive(d, refractive=refr), 3,
            lambda W, H, depth, x0, x1: refract_ref.trace(rs, le.column_rays(d.cam, W, H, x0, x1), depth))


@pytest.mark.parametrize("case", [twomirrors_case, glass_case], ids=["twomirrors", "glass"])
def test_hbm_bounce_stack_past_2_32_bytes(case):
    """option "stack" = 2, every level in HBM, on a persistent grid of eight times the resident workgroups ("grid_mult" = 8): the
    depth is chosen from a first launch's grid so that the stack -- grid_blocks x block_threads x (depth + 1) x 16 bytes, three
    times that for the *_refract kernels' three-quad entries -- lies between 2^32 + 10 % and the 8e9 bytes the host admits.  The
    frame (4096 x 2048, twice the grid's lanes) against the oracle-side reference on three columns, and every word against the
    same frame at the same depth with "grid_mult" = 1, whose stack is an eighth and below 2^31 bytes."""
    import torch
    r, quads, reference = case()
    W, H = 4096, 2048
    wpc, words = 3 * H, 3 * H * W
    le.require_device_memory(2 * Guarded.need(words) + 8 * 10 ** 9 + SLACK)
    big = small = None
    try:
        r.set_option("stack", 2)
        r.set_option("grid_mult", 8)
        launched_into(words, lambda ptr: r.render_device(W, H, 2, 0, W, ptr), "the first launch")
        li = r.launch_info()
        per_level = li.grid_blocks * li.block_threads * 16 * quads
        depth = math.ceil(1.12 * B32 / per_level)             # (depth + 1 levels: just above 2^32 + 10 %)
        assert 1.1 * B32 <= per_level * (depth + 1) <= 8e9, (li.grid_blocks, li.block_threads, depth)
        big, small = Guarded(words), Guarded(words)
        what = f"{r.kernel_name() or 'render'} {W}x{H} depth {depth}, stack in HBM"
        r.render_device(W, H, depth, 0, W, big.ptr)
        sync()
        li = r.launch_info()
        assert 1.1 * B32 <= stack_bytes(li, depth, quads) <= 8e9, (li.grid_blocks, li.block_threads, depth)
        assert li.grid_blocks * li.block_threads * 2 <= W * H           # the frame fills the grid
        big.assert_written(what)
        r.set_option("grid_mult", 1)
        r.render_device(W, H, depth, 0, W, small.ptr)
        sync()
        assert stack_bytes(r.launch_info(), depth, quads) < B31
        small.assert_written(what + ", grid_mult 1")
        text = le.device_difference(big.body, small.body, wpc, what + " against the same frame with a stack below 2^31 bytes")
        assert text is None, text
        assert_reference_columns(big.body, wpc, [0, W // 2 - 1, W - 1], lambda x0, x1: reference(W, H, depth, x0, x1), what)
    finally:
        for g in (big, small):
            if g is not None:
                g.free()
        r.close()
        torch.cuda.empty_cache()
