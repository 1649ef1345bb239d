"""The composed calls -- rt_render_adaptive, rt_render_lens, rt_indirect_diffuse -- at the sizes test_large_extents_gpu.py holds the
render kernels to: outputs past 2^32 bytes, records past 2^34, a list of more than 2^28 pixels (the scan's second step), and
chunks whose own scratch passes 4 GiB.  The ground rules are that file's, unchanged.  Every comparison is bit-exact.  Each large
output lies between two guards inside one sentinel-filled tensor (large_extents.Guarded): after the launch the guards still hold
the sentinel and no output word does.  Two references, neither sharing the addressing under test:
  (a) on the column that straddles each byte boundary, its two neighbours, column 0 and the last column
      (large_extents.boundary_columns): the call's definition restated -- adaptive_ref / lens_ref / indirect_ref over the handle's
      own G-buffer, supersampled and ray-batch calls of those few columns, each pinned by its own tests at these sizes;
  (b) the same call's strips of at most 1024 columns, each rendered at offset 0 of small guarded buffers and compared on the
      device with the matching slice of the large output -- every word of it.
Everything large stays on the device.  Every test computes its device-memory need first and skips only if less than 1.1 x that
is free; none needs more than 48 GB."""
import time

import numpy as np
import pytest

import adaptive_ref
import cameras
import indirect_ref
import large_extents as le
import lens_ref
import oracle_lib as oracle
from large_extents import Guarded
from tilecoderaytracer_amd import HostScene, Renderer
from tilecoderaytracer_amd.renderer import HIT_DTYPE

pytestmark = pytest.mark.gpu
F = np.float32
B28, B31, B32, B33, B34 = 1 << 28, 1 << 31, 1 << 32, 1 << 33, 1 << 34
SLACK = 3 << 30                          # the comparisons' temporaries: a few GiB-sized chunks at a time
CHUNK_SCRATCH = 256 << 20                # the three units' default chunk: its scratch within 256 MiB
MID_W, MID_H = 8200, 8185                # section 4's frame: 2^26 + 8136 pixels
MID_RECORDS = (1 << 26) + 4099


@pytest.fixture(autouse=True)
def measured(request):
    """each test's wall time and peak device memory, printed (pytest -rA shows them)"""
    import torch
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"[large composed] {request.node.name}: {time.time() - t0:.1f} s, peak device memory "
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


def gbuffer_columns(r, W, H, depth, x0, x1):
    """rt_render_gbuffer_device of columns [x0, x1) into small guarded buffers -> (rgb float32 (x1 - x0, H, 3), hits HIT_DTYPE
    (x1 - x0, H)) on the host"""
    n = (x1 - x0) * H
    rgb, hits = Guarded(3 * n), Guarded(12 * n)
    try:
        r.render_gbuffer_device(W, H, depth, x0, x1, rgb.ptr, hits.ptr)
        sync()
        rgb.assert_written(f"the G-buffer's colours of columns {x0}:{x1}")
        hits.assert_written(f"the G-buffer's records of columns {x0}:{x1}")
        return (rgb.body.cpu().numpy().view(F).reshape(x1 - x0, H, 3),
                hits.body.cpu().numpy().view(HIT_DTYPE).reshape(x1 - x0, H))
    finally:
        rgb.free()
        hits.free()


def free_all(*guarded):
    import torch
    for g in guarded:
        if g is not None:
            g.free()
    torch.cuda.empty_cache()


# ---- 1. adaptive supersampling past 2^28 pixels and past 2^32 bytes ---------------------------------------------------------------

# (W, H, x1, the colours' byte boundaries, the records' byte boundaries, color_threshold)
ADAPTIVE_CASES = [
    pytest.param(18945, 18944, 18944, [B31, B32], [B31, B32, B33, B34], 1 / 32, id="18945x18944-halo"),
    pytest.param(16400, 16400, 16400, [B31], [B31, B32, B33], 1e-5, id="16400x16400-direct"),
]


@pytest.mark.parametrize("W, H, x1, rgb_boundaries, hit_boundaries, threshold", ADAPTIVE_CASES)
def test_adaptive_list_past_2_28_pixels(W, H, x1, rgb_boundaries, hit_boundaries, threshold):
    """rt_render_adaptive_device, built-in scene, depth 2, k = 2, columns [0, x1).
    18 945 x 18 944, columns [0, 18 944): the halo path -- the first pass goes into scratch and the flag kernel copies the
    colours; 358 875 136 pixels, 1 401 856 workgroups, 1369 groups of counts, so rt_adaptive_scan_kernel takes a second step;
    the colours pass 2^32 bytes and the first pass's records 2^34.  16 400 x 16 400, the whole frame: the direct path, 268 960 000
    pixels, 1027 groups, the records past 2^33 bytes.
    In this order: (1) colours and flag bytes against the same call's strips of 1024 columns, each but a frame's last with its
    halo column; (2) on the boundary columns of the colours' and the records' strides the frame equals
    adaptive_ref.expected_frame(flags, rt_render_ssaa_device, rt_render_gbuffer_device) with adaptive_ref.frame_flags of that
    G-buffer's columns and their halo, and the flag bytes equal those flags; (3) rt_adaptive_info's `flagged` is the device-side
    count of flag bytes equal to 1 and rays = 4 x flagged.
    Condition (asserted): among the pixels numbered >= 2^28 -- the columns from 2^28 // H on, whose list offsets the scan's second
    step decides -- at least 1000 are flagged and at least 1000 are not, counted on the flag bytes once they have been held to the
    strips'.  Measured at the default thresholds (1 / 32, 0.9): 80 382 flagged and 90 359 298 unflagged of the first frame's
    90 439 680 such pixels; 427 flagged and 524 117 unflagged of the second frame's 524 544 (its last 32 columns) -- too few, so
    that case lowers color_threshold to 1e-5, where neighbouring pixels of a shaded surface already differ at this resolution
    while a flat background does not."""
    import torch
    depth, k, x0 = 2, 2, 0
    Wn, x1h = x1 - x0, min(x1 + 1, W)
    n, nh = Wn * H, (x1h - x0) * H
    cw = 3 * H
    assert n > B28 and H % 4 == 0
    blocks = -(-n // 256)
    assert -(-blocks // 1024) > 1024                     # the groups' sums need a second step of the scan
    assert (12 * n > B32) == (B32 in rgb_boundaries) and 48 * nh > hit_boundaries[-1]
    scratch = (12 * nh if x1h > x1 else 0) + 48 * nh + n + 4 * n + 16 * blocks + CHUNK_SCRATCH
    need = (Guarded.need(3 * n) + Guarded.need(n, as_bytes=True) + scratch + Guarded.need(le.STRIP_COLUMNS * cw)
            + Guarded.need(le.STRIP_COLUMNS * H // 4) + SLACK)
    le.require_device_memory(need)
    cols = sorted(set(le.boundary_columns(rgb_boundaries, 4 * cw, Wn)) | set(le.boundary_columns(hit_boundaries, 48 * H, Wn)))
    assert (B28 // H) < Wn - 1
    r, rgb, flags = Renderer(HostScene.builtin()), None, None
    what = f"rt_render_adaptive_device {W}x{H} columns {x0}:{x1} k={k}"
    kw = dict(samples=k, color_threshold=threshold)
    try:
        rgb, flags = Guarded(3 * n), Guarded(n, as_bytes=True)
        r.render_adaptive_device(W, H, depth, x0, x1, rgb.ptr, flags.ptr, **kw)
        sync()
        info = r.adaptive_info()
        flagged, rays, chunks = int(info.flagged), int(info.rays), int(info.chunks)
        rgb.assert_written(what + " colours")
        flags.assert_written(what + " flags")
        # (1) a strip's flag bytes are compared as the H / 4 words a column they are: a byte is 0 or 1, so no written word is
        # the sentinel
        le.assert_columns_equal_strips(lambda s0, s1, p_rgb, p_flags: r.render_adaptive_device(W, H, depth, s0, s1, p_rgb, p_flags, **kw),
                                       [(rgb.body, cw), (flags.body.view(torch.int32), H // 4)], Wn, what)
        tail = flags.body[B28:]
        tail_flagged = le.count_equal(tail, 1)
        tail_unflagged = le.count_equal(tail, 0)
        assert tail_flagged + tail_unflagged == n - B28
        print(f"[large composed] {what}: of the {n - B28} pixels numbered >= 2^28, {tail_flagged} are flagged and {tail_unflagged} "
              f"are not; {flagged} of {n} flagged in all, {chunks} chunks")
        # (2)
        for c0, c1 in le.runs(cols):
            c1h = min(c1 + 1, W)
            plain, hits = gbuffer_columns(r, W, H, depth, c0, c1h)
            ssaa = launched_into(3 * (c1 - c0) * H, lambda p: r.render_ssaa_device(W, H, depth, k, c0, c1, p),
                                 f"rt_render_ssaa_device columns {c0}:{c1}").view(F).reshape(c1 - c0, H, 3)
            want_flags = adaptive_ref.frame_flags(plain, hits, 0, c1 - c0, color_threshold=threshold)
            want = adaptive_ref.expected_frame(want_flags, ssaa, plain[:c1 - c0])
            got_flags = flags.body[c0 * H:c1 * H].cpu().numpy().reshape(c1 - c0, H)
            assert np.array_equal(got_flags, want_flags.astype(np.uint8)), \
                f"{what}: the flags of columns {c0}:{c1} differ from adaptive_ref's in {int((got_flags != want_flags).sum())} pixels"
            assert_reference_columns(rgb.body, cw, range(c0, c1), lambda a, b: want[a - c0:b - c0], what)
        # (3)
        ones = le.count_equal(flags.body, 1)
        assert flagged == ones, f"{what}: rt_adaptive_info says {flagged} flagged pixels, the flag bytes {ones}"
        assert rays == 4 * flagged and chunks == -(-flagged // (CHUNK_SCRATCH // (36 * k * k)))
        assert tail_flagged >= 1000 and tail_unflagged >= 1000, \
            f"{what}: the scan's second step decides too little: {tail_flagged} flagged, {tail_unflagged} unflagged pixels >= 2^28"
        assert rgb.guards_untouched() and flags.guards_untouched()
    finally:
        free_all(rgb, flags)
        r.close()


# ---- 2. the lens camera past 2^32 bytes of output ----------------------------------------------------------------------------------

LENS_W, LENS_H, LENS_DEPTH = 20000, 18000, 2


def test_lens_pinhole_past_2_32_bytes_is_rt_render():
    """rt_render_lens_device, 20 000 x 18 000 (4.32 GB), n = 1, aperture 0, focus 1, in 49 default chunks: every word equals
    rt_render_device's frame of the same size, which test_colours_past_2_32_bytes_device_and_host_paths pins to the oracle"""
    W, H, depth = LENS_W, LENS_H, LENS_DEPTH
    wpc, words = 3 * H, 3 * H * W
    assert words * 4 > B32
    le.require_device_memory(2 * Guarded.need(words) + CHUNK_SCRATCH + SLACK)
    r, lens, plain = Renderer(HostScene.builtin()), None, None
    what = f"rt_render_lens_device {W}x{H} n=1, a pinhole"
    try:
        lens, plain = Guarded(words), Guarded(words)
        r.render_lens_device(W, H, depth, 0, W, lens.ptr, samples=1, aperture=0.0, focus=1.0, seed=7)
        sync()
        info = r.lens_info()
        assert -(-W // (CHUNK_SCRATCH // 36 // H)) == 49
        assert (info.pixels, info.rays, info.chunks) == (W * H, W * H, 49)
        lens.assert_written(what)
        r.render_device(W, H, depth, 0, W, plain.ptr)
        sync()
        plain.assert_written(f"rt_render_device {W}x{H}")
        text = le.device_difference(lens.body, plain.body, wpc, what + " against rt_render_device")
        assert text is None, text
        assert lens.guards_untouched() and plain.guards_untouched()
    finally:
        free_all(lens, plain)
        r.close()


def test_lens_open_past_2_32_bytes():
    """rt_render_lens_device, 20 000 x 18 000, n = 2, lens_ref.lens_of("builtin")'s aperture and focus, seed 0xC0FFEE: 1.44e9 rays
    in 194 default chunks.  (b) over every word; (a) on the columns around 2^31 and 2^32 bytes, the first and the last, against
    lens_ref.resolve of the handle's own rt_trace_rays of lens_ref.rays (test_lens_gpu.own_reference's pattern)."""
    W, H, depth, n, seed = LENS_W, LENS_H, LENS_DEPTH, 2, 0xC0FFEE
    wpc, words = 3 * H, 3 * H * W
    assert words * 4 > B32
    le.require_device_memory(Guarded.need(words) + Guarded.need(le.STRIP_COLUMNS * wpc) + CHUNK_SCRATCH + SLACK)
    cols = le.boundary_columns([B31, B32], 4 * wpc, W)
    aperture, focus = lens_ref.lens_of("builtin", cameras.ANCHORS["builtin"]["focus"])
    assert aperture > 0
    host = HostScene.builtin()
    cam = lens_ref.camera_copy(host)
    r, big = Renderer(host), None
    kw = dict(samples=n, aperture=aperture, focus=focus, seed=seed)
    what = f"rt_render_lens_device {W}x{H} n={n}, lens open"

    def reference(x0, x1):
        rays = lens_ref.rays(cam, W, H, x0, x1, n, seed, aperture, focus)
        colours = r.trace_rays(np.ascontiguousarray(rays.reshape(x1 - x0, H * n * n, 6)), depth)
        return lens_ref.resolve(colours.reshape(x1 - x0, H, n * n, 3), n)

    try:
        big = Guarded(words)
        r.render_lens_device(W, H, depth, 0, W, big.ptr, **kw)
        sync()
        info = r.lens_info()
        assert (info.pixels, info.rays) == (W * H, W * H * n * n) and info.chunks > 1
        big.assert_written(what)
        le.assert_columns_equal_strips(lambda x0, x1, ptr: r.render_lens_device(W, H, depth, x0, x1, ptr, **kw), [(big.body, wpc)], W, what)
        assert_reference_columns(big.body, wpc, cols, reference, what)
        assert big.guards_untouched()
    finally:
        free_all(big)
        r.close()


# ---- 3. the indirect term past 2^32 bytes of output --------------------------------------------------------------------------------

def test_indirect_term_past_2_32_bytes():
    """rt_indirect_diffuse_device on the records of rt_render_gbuffer_device at 18 944^2: 358 875 136 records (above 357 913 941:
    the output passes 4 GiB, the records 2^34 bytes), depth 2, n = 1, gather_depth 1, gain 0.75, seed 0xBEEF, 1 000 003 records a
    chunk (see below).  Three calls: emitters 1
    onto a base (the frame's colours), emitters 0 onto the base, emitters 0 in place (out == base).  Each: (b) every word against the
    same call, out of place, on slices of 1024 columns with key0 = (x0 H) mod 2^32; (a) on the columns around the output's 2^31 and
    2^32 bytes and the records' 2^31 .. 2^34, the first and the last, against indirect_ref.resolve of the handle's own
    rt_trace_rays and rt_intersect_rays of indirect_ref.rays.  Condition: on those columns the term is non-zero on at least 5 % of
    the live records, and at least one gather ray's first hit is a light (so emitters 0 masks something)."""
    W = H = 18944
    depth, n, gather_depth, gain, seed = 2, 1, 1, 0.75, 0xBEEF
    N = W * H
    # The default chunks (7 456 540 and 3 195 660 records: 2^28 / 36 and 2^28 / 84 bytes' worth) both have a chunk start at record
    # 357 913 920, 21 records short of 2^32 bytes of output, and none after it: the host loop's offsets of a chunk -- 48 i0 into the
    # records, 12 i0 into the base and the output -- would never pass 2^32 there.  With 1 000 003 records a chunk the last of the
    # 359 chunks starts at record 358 001 074, past it.
    chunk = 1000003
    assert 12 * (N // chunk * chunk) > B32 and N % chunk != 0
    cw, hw = 3 * H, 12 * H
    assert N > 357913941 and 12 * N > B32 and 48 * N > B34
    need = (2 * Guarded.need(3 * N) + Guarded.need(12 * N) + Guarded.need(le.STRIP_COLUMNS * cw) + CHUNK_SCRATCH + SLACK)
    le.require_device_memory(need)
    cols = sorted(set(le.boundary_columns([B31, B32], 4 * cw, W)) | set(le.boundary_columns([B31, B32, B33, B34], 4 * hw, W)))
    kd = indirect_ref.object_diffuse(oracle.OracleScene.builtin())
    r, base, hits, out = Renderer(HostScene.builtin()), None, None, None
    try:
        base, hits, out = Guarded(3 * N), Guarded(12 * N), Guarded(3 * N)
        r.render_gbuffer_device(W, H, depth, 0, W, base.ptr, hits.ptr)
        sync()
        base.assert_written("the frame's colours")
        hits.assert_written("the frame's records")
        before = le.checksum(base.body)

        # the references of the boundary columns, once: [emitters] -> {(x0, x1): words}
        wanted, shares, lights = {False: {}, True: {}}, [], 0
        for x0, x1 in le.runs(cols):
            h = hits.body[x0 * hw:x1 * hw].cpu().numpy().view(HIT_DTYPE).reshape(x1 - x0, H)
            b = base.body[x0 * cw:x1 * cw].cpu().numpy().view(F).reshape(x1 - x0, H, 3)
            rays, _ = indirect_ref.rays(h, n, seed, (x0 * H) & 0xFFFFFFFF)
            flat = np.ascontiguousarray(rays.reshape(-1, 6))
            colours = r.trace_rays(flat, gather_depth).reshape(h.shape + (n * n, 3))
            light = ((r.intersect_rays(flat)["flags"] & indirect_ref.HIT_LIGHT) != 0).reshape(h.shape + (n * n,))
            for emitters in (False, True):
                wanted[emitters][(x0, x1)] = indirect_ref.resolve(colours, light, kd, h, gain, b, emitters)
            shares.append((indirect_ref.nonzero_share(indirect_ref.resolve(colours, light, kd, h, gain, None, False), h), h.size))
            lights += int(light[indirect_ref.ao_ref.live_records(h).reshape(h.shape)].sum())
        share = sum(s * k for s, k in shares) / sum(k for _, k in shares)
        print(f"[large composed] the indirect term on the boundary columns {cols}: non-zero on {share:.3f} of the live records, "
              f"{lights} gather rays meet a light first")

        def strip(emitters):
            return lambda x0, x1, ptr: r.indirect_diffuse_device(
                (x1 - x0) * H, hits.ptr + x0 * H * 48, base.ptr + x0 * H * 12, ptr, samples=n, gather_depth=gather_depth, gain=gain,
                seed=seed, key0=(x0 * H) & 0xFFFFFFFF, emitters=emitters)

        for emitters, in_place in ((True, False), (False, False), (False, True)):
            what = f"rt_indirect_diffuse_device {N} records, emitters {int(emitters)}" + (", in place" if in_place else "")
            if in_place:
                out.body.copy_(base.body)
            else:
                out.refill()
            r.indirect_diffuse_device(N, hits.ptr, out.ptr if in_place else base.ptr, out.ptr, samples=n, gather_depth=gather_depth,
                                      gain=gain, seed=seed, key0=0, emitters=emitters, chunk_records=chunk)
            sync()
            info = r.indirect_info()
            assert (info.records, info.rays, info.chunks) == (N, N * n * n, -(-N // chunk))
            out.assert_written(what)
            le.assert_columns_equal_strips(strip(emitters), [(out.body, cw)], W, what)
            assert_reference_columns(out.body, cw, cols, lambda x0, x1: wanted[emitters][(x0, x1)], what)
            assert out.guards_untouched() and hits.guards_untouched() and base.guards_untouched()
        assert le.checksum(base.body) == before, "the base changed"
        assert share >= 0.05 and lights >= 1, (share, lights)
    finally:
        free_all(base, hits, out)
        r.close()


# ---- 4. a chunk whose own scratch passes 4 GiB -------------------------------------------------------------------------------------

def test_indirect_chunk_scratch_past_4_gib():
    """2^26 + 4099 records (an 8200 x 8185 G-buffer cut to that many), n = 2, chunk_records = 2^26: one chunk of 2^28 rays -- 6.4 GB
    of rays, 3.2 GB of sample colours and, with emitters 0, 12.9 GB of gather records -- and a tail of 4099 records.  Every word
    equals the same call's with the default chunk (its scratch within 256 MiB), onto a base, for both `emitters` settings."""
    import torch
    W, H, depth, n, N, chunk = MID_W, MID_H, 2, 2, MID_RECORDS, 1 << 26
    S = n * n
    assert W * H >= N and chunk * S * 24 > B32 and chunk * S * 12 > B31 and chunk * S * 48 > B33
    need = W * H * 60 + 2 * Guarded.need(3 * N) + chunk * S * 84 + SLACK
    le.require_device_memory(need)
    r, a, b = Renderer(HostScene.builtin()), None, None
    try:
        base = torch.empty(3 * W * H, dtype=torch.int32, device="cuda")
        hits = torch.empty(12 * W * H, dtype=torch.int32, device="cuda")
        r.render_gbuffer_device(W, H, depth, 0, W, base.data_ptr(), hits.data_ptr())
        sync()
        a, b = Guarded(3 * N), Guarded(3 * N)
        for emitters in (True, False):
            kw = dict(samples=n, gather_depth=1, gain=0.75, seed=3, key0=0xFFFFF000, emitters=emitters)
            what = f"rt_indirect_diffuse_device {N} records n={n} emitters {int(emitters)}"
            a.refill()
            b.refill()
            r.indirect_diffuse_device(N, hits.data_ptr(), base.data_ptr(), a.ptr, **kw)
            sync()
            assert r.indirect_info().chunks == -(-N // (CHUNK_SCRATCH // (S * (36 if emitters else 84)))) > 2
            r.indirect_diffuse_device(N, hits.data_ptr(), base.data_ptr(), b.ptr, chunk_records=chunk, **kw)
            sync()
            info = r.indirect_info()
            assert (info.records, info.rays, info.chunks) == (N, N * S, 2)
            a.assert_written(what + ", default chunk")
            b.assert_written(what + f", chunk_records {chunk}")
            text = le.device_difference(b.body, a.body, 3, what + f": chunk_records {chunk} against the default chunk (a column is a record)")
            assert text is None, text
            assert not torch.equal(a.body, base[:3 * N])              # (the term is not empty)
    finally:
        base = hits = None
        free_all(a, b)
        r.close()


def test_lens_chunk_scratch_past_4_gib():
    """8204 x 8185, n = 2, lens open, chunk_columns = 8200: a chunk of 2^26 + 8136 pixels -- 6.4 GB of rays, 3.2 GB of sample
    colours -- and a tail of 4 columns.  Every word equals the same call's with the default chunk."""
    W, H, depth, n, chunk = MID_W + 4, MID_H, 2, 2, MID_W
    words = 3 * W * H
    assert chunk * H >= 1 << 26 and chunk * H * n * n * 24 > B32
    le.require_device_memory(2 * Guarded.need(words) + chunk * H * n * n * 36 + SLACK)
    aperture, focus = lens_ref.lens_of("builtin", cameras.ANCHORS["builtin"]["focus"])
    r, a, b = Renderer(HostScene.builtin()), None, None
    kw = dict(samples=n, aperture=aperture, focus=focus, seed=5)
    what = f"rt_render_lens_device {W}x{H} n={n}"
    try:
        a, b = Guarded(words), Guarded(words)
        r.render_lens_device(W, H, depth, 0, W, a.ptr, **kw)
        sync()
        assert r.lens_info().chunks > 2
        r.render_lens_device(W, H, depth, 0, W, b.ptr, chunk_columns=chunk, **kw)
        sync()
        info = r.lens_info()
        assert (info.pixels, info.rays, info.chunks) == (W * H, W * H * n * n, 2)
        a.assert_written(what + ", default chunk")
        b.assert_written(what + f", chunk_columns {chunk}")
        text = le.device_difference(b.body, a.body, 3 * H, what + f": chunk_columns {chunk} against the default chunk")
        assert text is None, text
    finally:
        free_all(a, b)
        r.close()


def test_adaptive_chunk_scratch_past_4_gib():
    """8200 x 8185, flag_all, k = 2, chunk_pixels = 2^26: a chunk of 2^28 rays -- 6.4 GB of rays, 3.2 GB of sample colours -- and a
    tail of 8136 pixels.  Every word equals the same call's with the default chunk, and rt_render_ssaa_device's frame."""
    W, H, depth, k, chunk = MID_W, MID_H, 2, 2, 1 << 26
    n = W * H
    assert n >= MID_RECORDS and chunk * k * k * 24 > B32
    le.require_device_memory(3 * Guarded.need(3 * n) + n * (48 + 1 + 4) + chunk * k * k * 36 + SLACK)
    r, a, b, c = Renderer(HostScene.builtin()), None, None, None
    kw = dict(samples=k, flag_all=True)
    what = f"rt_render_adaptive_device {W}x{H} flag_all k={k}"
    try:
        a, b, c = Guarded(3 * n), Guarded(3 * n), Guarded(3 * n)
        r.render_adaptive_device(W, H, depth, 0, W, a.ptr, **kw)
        sync()
        info = r.adaptive_info()
        assert (info.flagged, info.rays) == (n, n * k * k) and info.chunks > 2
        r.render_adaptive_device(W, H, depth, 0, W, b.ptr, chunk_pixels=chunk, **kw)
        sync()
        info = r.adaptive_info()
        assert (info.pixels, info.flagged, info.rays, info.chunks) == (n, n, n * k * k, 2)
        r.render_ssaa_device(W, H, depth, k, 0, W, c.ptr)
        sync()
        a.assert_written(what + ", default chunk")
        b.assert_written(what + f", chunk_pixels {chunk}")
        c.assert_written(f"rt_render_ssaa_device {W}x{H} k={k}")
        for other, name in ((a, "the default chunk"), (c, "rt_render_ssaa_device")):
            text = le.device_difference(b.body, other.body, 3 * H, what + f": chunk_pixels {chunk} against {name}")
            assert text is None, text
    finally:
        free_all(a, b, c)
        r.close()
