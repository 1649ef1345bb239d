"""Device launches into sentinel-filled outputs: a cell that a launch never wrote shows, which a comparison of the handle's own
framebuffer -- never cleared, and still holding the previous launch's correct pixels -- cannot see.

One function per DEVICE entry point (rt_render_device, rt_render_ssaa_device, rt_render_gbuffer_device, rt_trace_rays_device,
rt_intersect_rays_device, rt_occluded_rays_device, rt_ambient_occlusion_device).  Each one
  1. allocates every output as a large_extents.Guarded body SLACK cells longer than the call needs, all of it -- and a MiB before
     and after -- filled with the sentinel (a NaN payload no kernel produces; 0xA5 for the verdicts, which are 0 or 1),
  2. launches on the current torch stream and synchronises,
  3. asserts that the guards are untouched, 4. that no word of the needed part still holds the sentinel, 5. that every slack
     word still does (a write past the end shows inside the body as well as in the guard),
  6. returns the outputs as numpy arrays in the wrappers' shapes.
Before the launch the reference the caller will compare with (`want`) is checked to hold no word equal to the sentinel: otherwise
a legitimate output word could never read as "unwritten".  The comparison itself stays with the caller.

The checking half, check_output(), works on numpy arrays alone (tests/test_poisoned_cpu.py); importing this module needs
neither torch nor a device."""
from collections import namedtuple

import numpy as np

from large_extents import SENTINEL, SENTINEL_BYTE, Guarded

SLACK_CELLS = 67                          # cells beyond the needed ones: more than a tile's 64, and odd
HIT_WORDS = 12                            # an rt_hit is 48 bytes
HIT_FIELDS = ("object", "distance", "point.x", "point.y", "point.z", "normal.x", "normal.y", "normal.z",
              "color.r", "color.g", "color.b", "flags")

# How an output's words map to the launch's cells and tiles: cell = word // words_per_cell, column x0 + cell // rows, row
# cell % rows (a frame's pixels[x][z], a batch's ray x * rows + z).  tile_x, tile_z: rt_launch_info's, in cells of the image the
# launch takes its decisions on -- for a k x k supersampled frame the virtual one, k times the output's (scale = k).
Layout = namedtuple("Layout", "words_per_cell rows x0 tile_x tile_z scale channels")


def layout(words_per_cell, rows, x0=0, tile_x=0, tile_z=0, scale=1, channels=None):
    return Layout(int(words_per_cell), int(rows), int(x0), int(tile_x), int(tile_z), int(scale),
                  tuple(channels) if channels else tuple(str(c) for c in range(words_per_cell)))


def locate(word, lay):
    """word number of an output -> (x, z, channel name, tile column, tile row); the tile is None without a tile shape"""
    cell, c = divmod(int(word), lay.words_per_cell)
    col, z = divmod(cell, lay.rows)
    tile = None
    if lay.tile_x > 0 and lay.tile_z > 0:
        tile = (col * lay.scale // lay.tile_x, z * lay.scale // lay.tile_z)
    return lay.x0 + col, z, lay.channels[c], tile


def describe_unwritten(words, lay, needed):
    """the text for the unwritten word numbers `words` (sorted, not empty) of an output of `needed` words: the first as pixel,
    channel and tile, and whether the unwritten words are whole tiles"""
    x, z, channel, tile = locate(words[0], lay)
    text = f"{len(words)} of {needed} output words were never written, first at pixel (x={x}, z={z}) channel {channel}"
    if tile is None:
        return text
    cells = np.unique(np.asarray(words, dtype=np.int64) // lay.words_per_cell)
    cols, zs = cells // lay.rows, cells % lay.rows
    tiles = np.unique(np.stack([cols * lay.scale // lay.tile_x, zs * lay.scale // lay.tile_z], axis=1), axis=0)
    # the cells of the first tile that lie inside the output (a batch's last column may be short), and how many of them have
    # every word unwritten
    n_cells = needed // lay.words_per_cell
    tx, tz, k = lay.tile_x, lay.tile_z, lay.scale
    c = np.arange(-(-tile[0] * tx // k), -(-(tile[0] + 1) * tx // k), dtype=np.int64)
    zz = np.arange(-(-tile[1] * tz // k), min(-(-(tile[1] + 1) * tz // k), lay.rows), dtype=np.int64)
    of_tile = int(((c[:, None] * lay.rows + zz[None, :]) < n_cells).sum())
    mine = (cols * k // tx == tile[0]) & (zs * k // tz == tile[1])
    per_cell = np.bincount(np.searchsorted(cells, np.asarray(words, dtype=np.int64) // lay.words_per_cell), minlength=len(cells))
    whole_cells = int((mine & (per_cell == lay.words_per_cell)).sum())
    text += (f", in tile column {tile[0]}, tile row {tile[1]} (tiles of {tx} x {tz}); the unwritten words lie in {len(tiles)} "
             f"tile{'s' if len(tiles) != 1 else ''}")
    text += f": tile ({tile[0]}, {tile[1]}) was dropped whole ({of_tile} cells)" if whole_cells == of_tile else \
            f": {int(mine.sum())} of the {of_tile} cells of tile ({tile[0]}, {tile[1]})"
    return text


def _unsigned(a):
    """a flat view of a's words (4-byte items) or bytes as unsigned integers"""
    a = np.ascontiguousarray(a).reshape(-1)
    assert a.dtype.itemsize in (1, 4), a.dtype
    return a.view(np.uint8 if a.dtype.itemsize == 1 else np.uint32)


def check_output(head, body, tail, needed, lay, what, fill=SENTINEL):
    """The checking half, on numpy arrays: head and tail are the guards before and after body, whose first `needed` words the
    launch had to write and whose other words are slack.  Raises AssertionError naming `what`; returns body[:needed]."""
    head, body, tail = (_unsigned(a) for a in (head, body, tail))
    assert head.dtype == body.dtype == tail.dtype and 0 <= fill <= np.iinfo(body.dtype).max, (what, body.dtype, fill)
    for name, guard in (("before", head), ("after", tail)):
        bad = np.flatnonzero(guard != fill)
        assert len(bad) == 0, (f"{what}: {len(bad)} words of the guard {name} the output were overwritten, the "
                               f"{'last' if name == 'before' else 'first'} at {int(bad[-1]) - len(guard) if name == 'before' else int(bad[0])} "
                               f"words {'before its start' if name == 'before' else 'past its end'}")
    assert 0 <= needed <= len(body), (what, needed, len(body))
    left = np.flatnonzero(body[:needed] == fill)
    assert len(left) == 0, f"{what}: {describe_unwritten(left, lay, needed)}"
    spoilt = np.flatnonzero(body[needed:] != fill)
    assert len(spoilt) == 0, (f"{what}: {len(spoilt)} slack words past the output's end were written, the first {int(spoilt[0])} "
                              f"words past it (the output has {needed} words)")
    return body[:needed]


def assert_reference_has_no_sentinel(want, what, fill=SENTINEL):
    """the reference a launch will be compared with holds no word (byte: fill = SENTINEL_BYTE) equal to the sentinel"""
    for k, a in enumerate(want if isinstance(want, (tuple, list)) else (want,)):
        a = np.ascontiguousarray(a)
        assert a.dtype.itemsize in (1, 4) or a.dtype.itemsize % 4 == 0, (what, a.dtype)
        words = a.reshape(-1).view(np.uint8 if a.dtype.itemsize == 1 else np.uint32)
        one = np.uint8(SENTINEL_BYTE) if a.dtype.itemsize == 1 else np.uint32(fill)
        n = int((words == one).sum())
        assert n == 0, (f"{what}: reference {k} holds {n} words equal to the sentinel 0x{int(one):x}, first at word "
                        f"{int(np.flatnonzero(words == one)[0])}: such an output word could never read as written")


# ---- the launching half ---------------------------------------------------------------------------------------------------------

class _Outputs:
    """the guarded outputs of one launch: (needed words, words per cell, channel names, bytes?) each"""

    def __init__(self, specs):
        self.specs = specs
        self.bufs = [Guarded(needed + SLACK_CELLS * wpc, as_bytes=as_bytes) for needed, wpc, _, as_bytes in specs]

    def ptrs(self):
        return [g.ptr for g in self.bufs]

    def checked(self, r, rows, x0, scale, what):
        """synchronise, run check_output() on every output -> the needed words of each, on the host"""
        import torch
        torch.cuda.synchronize()
        li = r.launch_info()
        out = []
        try:
            for k, (g, (needed, wpc, channels, as_bytes)) in enumerate(zip(self.bufs, self.specs)):
                lay = layout(wpc, rows, x0, li.tile_x, li.tile_z, scale, channels)
                name = what if len(self.specs) == 1 else f"{what}, output {k}"
                host = g.all.cpu().numpy()
                out.append(check_output(host[:g.guard], host[g.guard:g.guard + g.n], host[g.guard + g.n:], needed, lay, name,
                                        SENTINEL_BYTE if as_bytes else SENTINEL).copy())
        finally:
            for g in self.bufs:
                g.free()
        return out


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _on_device(array):
    import torch
    t = torch.from_numpy(np.array(array, copy=True, order="C").reshape(-1).view(np.int32)).cuda()      # (a copy: the caller's may be read-only)
    assert t.data_ptr() % 16 == 0
    return t


RGB = ("r", "g", "b")


def rt_render_device(r, W, H, depth, x0, x1, want):
    """rt_render_device of columns [x0, x1) -> float32 (x1 - x0, H, 3)"""
    what = f"rt_render_device {W}x{H} columns {x0}:{x1} depth {depth}"
    assert_reference_has_no_sentinel(want, what)
    o = _Outputs([((x1 - x0) * H * 3, 3, RGB, False)])
    r.render_device(W, H, depth, x0, x1, o.ptrs()[0], _stream())
    rgb, = o.checked(r, H, x0, 1, what)
    return rgb.view(np.float32).reshape(x1 - x0, H, 3)


def rt_render_ssaa_device(r, W, H, depth, samples, x0, x1, want):
    """rt_render_ssaa_device of output columns [x0, x1) -> float32 (x1 - x0, H, 3); a failure's tile is the virtual image's"""
    what = f"rt_render_ssaa_device {W}x{H} k={samples} columns {x0}:{x1} depth {depth}"
    assert_reference_has_no_sentinel(want, what)
    o = _Outputs([((x1 - x0) * H * 3, 3, RGB, False)])
    r.render_ssaa_device(W, H, depth, samples, x0, x1, o.ptrs()[0], _stream())
    rgb, = o.checked(r, H, x0, samples, what)
    return rgb.view(np.float32).reshape(x1 - x0, H, 3)


def rt_render_gbuffer_device(r, W, H, depth, x0, x1, want):
    """rt_render_gbuffer_device -> (float32 (x1 - x0, H, 3), HIT_DTYPE (x1 - x0, H)); want: (colours, records)"""
    from tilecoderaytracer_amd.renderer import HIT_DTYPE
    what = f"rt_render_gbuffer_device {W}x{H} columns {x0}:{x1} depth {depth}"
    assert_reference_has_no_sentinel(want, what)
    cells = (x1 - x0) * H
    o = _Outputs([(cells * 3, 3, RGB, False), (cells * HIT_WORDS, HIT_WORDS, HIT_FIELDS, False)])
    r.render_gbuffer_device(W, H, depth, x0, x1, *o.ptrs(), _stream())
    rgb, hits = o.checked(r, H, x0, 1, what)
    return rgb.view(np.float32).reshape(x1 - x0, H, 3), hits.view(HIT_DTYPE).reshape(x1 - x0, H)


def _batch(rays):
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    assert rays.ndim in (2, 3) and rays.shape[-1] == 6, rays.shape
    return rays, rays.size // 6, rays.shape[:-1]


def rt_trace_rays_device(r, rays, rows, depth, want):
    """rt_trace_rays_device of rays (n, 6) or (X, Z, 6) laid out in `rows` rows -> float32 of rays' shape with 3 for the 6"""
    rays, n, shape = _batch(rays)
    what = f"rt_trace_rays_device n={n} rows={rows} depth {depth}"
    assert_reference_has_no_sentinel(want, what)
    d_rays = _on_device(rays)
    o = _Outputs([(n * 3, 3, RGB, False)])
    r.trace_rays_device(n, rows, d_rays.data_ptr(), depth, o.ptrs()[0], _stream())
    rgb, = o.checked(r, min(rows, max(n, 1)), 0, 1, what)
    return rgb.view(np.float32).reshape(shape + (3,))


def rt_intersect_rays_device(r, rays, rows, want):
    """rt_intersect_rays_device -> HIT_DTYPE of rays' shape without the 6"""
    from tilecoderaytracer_amd.renderer import HIT_DTYPE
    rays, n, shape = _batch(rays)
    what = f"rt_intersect_rays_device n={n} rows={rows}"
    assert_reference_has_no_sentinel(want, what)
    d_rays = _on_device(rays)
    o = _Outputs([(n * HIT_WORDS, HIT_WORDS, HIT_FIELDS, False)])
    r.intersect_rays_device(n, rows, d_rays.data_ptr(), o.ptrs()[0], _stream())
    hits, = o.checked(r, min(rows, max(n, 1)), 0, 1, what)
    return hits.view(HIT_DTYPE).reshape(shape)


def rt_occluded_rays_device(r, segs, rows, want):
    """rt_occluded_rays_device -> bool of segs' shape without the 6 (the byte sentinel: a verdict is 0 or 1)"""
    segs, n, shape = _batch(segs)
    what = f"rt_occluded_rays_device n={n} rows={rows}"
    assert_reference_has_no_sentinel(np.ascontiguousarray(want).view(np.uint8), what)
    d_segs = _on_device(segs)
    o = _Outputs([(n, 1, ("verdict",), True)])
    r.occluded_rays_device(n, rows, d_segs.data_ptr(), o.ptrs()[0], _stream())
    verdicts, = o.checked(r, min(rows, max(n, 1)), 0, 1, what)
    assert ((verdicts == 0) | (verdicts == 1)).all(), f"{what}: a verdict is neither 0 nor 1"
    return verdicts.view(np.bool_).reshape(shape)


def rt_ambient_occlusion_device(r, hits, rows, want, samples=4, radius=1.0, seed=0, key0=0, channels=1):
    """rt_ambient_occlusion_device of records (n,) or (X, Z) -> float32 of hits' shape, with channels = 3 of that shape + (3,)"""
    from tilecoderaytracer_amd.renderer import HIT_DTYPE
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    n, shape = hits.size, hits.shape
    assert channels in (1, 3), channels
    what = f"rt_ambient_occlusion_device n={n} rows={rows} samples {samples} channels {channels}"
    assert_reference_has_no_sentinel(want, what)
    d_hits = _on_device(hits.view(np.int32))
    o = _Outputs([(n * channels, channels, RGB[:channels] if channels == 3 else ("ao",), False)])
    r.ambient_occlusion_device(n, rows, d_hits.data_ptr(), o.ptrs()[0], samples=samples, radius=radius, seed=seed, key0=key0,
                               channels=channels, stream=_stream())
    ao, = o.checked(r, min(rows, max(n, 1)), 0, 1, what)
    return ao.view(np.float32).reshape(shape + ((3,) if channels == 3 else ()))
