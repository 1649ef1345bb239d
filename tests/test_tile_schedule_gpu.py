"""The tile scheduler with work to hand out: frames with more queue entries than the persistent grid has wavefronts, under every
way the tile loop is compiled and every schedule setting, launched into sentinel-filled outputs (poisoned.py) and compared bit
for bit with the references.

Why: the host entry points render into the handle's framebuffer, which is never cleared, so a tile that a launch drops still
holds the previous launch's correct pixels there; and at the small frames of the option tests every wavefront renders the one
tile it was handed by arithmetic and leaves -- the queue heads, the steal walk, the wrap-around of the start row, the twin
entries and the ragged top macro row never decide anything.  A scheduler fault is a MISSING tile, which only an output that was
poisoned before the launch can show.

Kernels (KERNELS): one per way render_body()'s loop is compiled -- rt_render_kernel (twin entries, one look at all heads),
_items (single tiles, asks ahead, one look), _large on the built-in scene and on the clustered field (++steal; both ask ahead:
ask_ahead is false for the kClusters and counting kernels only, and _large is compiled without kClusters), _clusters and
_clusters_wide (++steal, ask afterwards; HELP off, HELP from two leaves with 256 threads, a HEAVY band -- with HELP on, without
which heavy_band() does nothing -- and the automatic choice on a strip of a third of the width), _ssaa with k = 2 (the virtual
image's tiles), _gbuffer (two outputs), _rays, _hits, _occluded, rt_ao_kernel and rt_ao_kernel_clusters over grids with rows > 1
whose last column is five cells short.  Settings (SETTINGS), each on its own: first_row 0, 500, 999 (-1 is the default case),
grid_mult 1 (the default), 2, 0, block_threads 64, 256 and, for the clustered kernels, 512, tile_z 1, 64 (and the default),
tile_prio 1, a learned order, a strip with x0 > 0.

The size condition (size_condition()): every launch with a persistent grid reads rt_get_launch_info and asserts
entries >= 2 x wavefronts (grid_mult 2: entries > wavefronts), entries = tiles_x x tiles_z, for rt_render_kernel tiles_x x
ceil(tiles_z / 2).  A case that does not meet it fails: it would have passed without one queue pop.  With grid_mult 0 the same
frames hand every entry out by arithmetic.

Sizes, the smallest (width between 1.25 and 1.4 heights) that meet the condition for the whole frame and for the strip, with --
under each of the tile shapes 4 x 16 (the default), 64 x 1 and 1 x 64 -- a number of tile rows that is no multiple of 4 (odd for
the twin kernel), a number of macro tiles that is no multiple of 8 and neither side a multiple of the tile's.  The grid is
occupancy x 256 CUs; the occupancy below is what the kernels' register counts admit (`make asm`: 96 VGPRs -> 5 wavefronts per
SIMD, 80 -> 6, 70-72 -> 7, 63 and fewer -> 8, the hardware's limit: no grid of 256-thread workgroups exceeds 2048), which LDS
can only lower; the grid_blocks below are the ones read on an MI355X, and they are these (every test 0.75 s or less there):
  SINGLE  1089 x  833  built-in: _items, _rays, the counting build   7 per SIMD: 1792 x 4 = 7168; 273 x 53 = 14 469 entries, 2.02
  EIGHT   1157 x  897  built-in: _large, _hits, _occluded, rt_ao_kernel   8 per SIMD: 2048 x 4 = 8192; 290 x 57 = 16 530, 2.02
                       (_gbuffer, 7 per SIMD, as well: it shares the records);  the field, one frame for its five kernels:
                       _large 8192, _clusters and rt_ao_kernel_clusters 6 x 1024 = 6144 (2.69), _clusters_wide 5120 (3.23)
  TWIN    1281 x 1025  rt_render_kernel   5 per SIMD: 1280 x 4 = 5120; 321 x 33 = 10 593 twins of 65 tile rows, 2.07
  SSAA     547 x  417  k = 2, virtual 1094 x 834   7 per SIMD: 7168; 274 x 53 = 14 522 entries, 2.03
  THIRD   columns 1159:2316 of 3471 x 897, the clustered kernels' strip of a third of the width (290 x 57 tiles again)
The strips [7, W) (k = 2: [6, W)) keep the ratio at 2.00 or above.  Every case prints what it read ("[tile schedule] ...",
pytest -rA).

References, computed once per scene and size (functools.lru_cache) and never changed: the C oracle's frame at depth 2 (built-in)
or 1 (field), in column blocks on the host's cores; query_ref's records and verdicts; ao_ref; the oracle's 2W x 2H frame through
ssaa_ref.box_filter (the kernel's order)."""
import functools
import os
import time
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import ao_ref
import poisoned
import query_ref
from rays_ref import camera_rays
from ssaa_ref import box_filter
from test_kernel_matrix_gpu import build, world
from test_query_gpu import assert_hits_same, assert_verdicts_same
from test_texture_gpu import assert_same_bits

pytestmark = pytest.mark.gpu
F = np.float32

DEPTH = {"builtin": 2, "field": 1}
SINGLE, EIGHT, TWIN, SSAA = (1089, 833), (1157, 897), (1281, 1025), (547, 417)
STRIP_X0 = {1: 7, 2: 6}                   # the strip [x0, W); by k: k (W - x0) is no multiple of the tile's 4 either
THIRD = (3471, 1159, 2316)                # the clustered kernels' automatic choice: W, x0, x1 of a strip of a third of the width
SHORT = 5                                 # the batches' last column is this many cells short
AO_SAMPLES, AO_RADIUS, AO_SEED = 1, 2.0, 1

Kernel = namedtuple("Kernel", "id scene options call name size clustered")
KERNELS = [
    Kernel("fast", "builtin", {}, "render", "rt_render_kernel", TWIN, False),
    Kernel("items", "builtin", {"fast": 0}, "render", "rt_render_kernel_items", SINGLE, False),
    Kernel("large_builtin", "builtin", {"tables": 2}, "render", "rt_render_kernel_large", EIGHT, False),
    Kernel("large_field", "field", {"tables": 2}, "render", "rt_render_kernel_large", EIGHT, False),
    Kernel("clusters", "field", {"wide": 0, "help": 0}, "render", "rt_render_kernel_clusters", EIGHT, True),
    Kernel("clusters_wide", "field", {"wide": 1, "help": 0}, "render", "rt_render_kernel_clusters_wide", EIGHT, True),
    Kernel("ssaa", "builtin", {}, "ssaa", "rt_render_kernel_ssaa", SSAA, False),
    Kernel("gbuffer", "builtin", {}, "gbuffer", "rt_render_kernel_gbuffer", EIGHT, False),
    Kernel("rays", "builtin", {}, "rays", "rt_render_kernel_rays", SINGLE, False),
    Kernel("hits", "builtin", {}, "hits", "rt_render_kernel_hits", EIGHT, False),
    Kernel("occluded", "builtin", {}, "occluded", "rt_render_kernel_occluded", EIGHT, False),
    Kernel("ao", "builtin", {}, "ao", "rt_ao_kernel", EIGHT, False),
    Kernel("ao_clusters", "field", {"wide": 0}, "ao", "rt_ao_kernel_clusters", EIGHT, True),
]

# id -> (options, what else: "learn" = rt_learn_tile_order first, "strip" = columns [x0, W), "third" = THIRD)
SETTINGS = {
    "default": ({}, None),                # first_row -1, grid_mult 1, the default tile shape
    "first_row_0": ({"first_row": 0}, None),
    "first_row_500": ({"first_row": 500}, None),
    "first_row_999": ({"first_row": 999}, None),
    "grid_mult_2": ({"grid_mult": 2}, None),
    "grid_mult_0": ({"grid_mult": 0}, None),
    "block_64": ({"block_threads": 64}, None),
    "block_256": ({"block_threads": 256}, None),
    "block_512": ({"block_threads": 512}, None),
    "tile_z_1": ({"tile_z": 1}, None),
    "tile_z_64": ({"tile_z": 64}, None),
    "tile_prio_1": ({"tile_prio": 1}, None),
    "learned": ({}, "learn"),
    "strip": ({}, "strip"),
    # the clustered render kernels alone (their own "help": 0 is the HELP-off case)
    "help_2": ({"help": 2, "block_threads": 256}, None),
    "heavy_2": ({"help": 1, "heavy": 2}, None),
    "automatic_third": ({"help": -1, "heavy": -1, "tile_prio": -1}, "third"),
}


def applies(kernel, setting):
    if setting in ("help_2", "heavy_2", "automatic_third"):
        return kernel.clustered and kernel.call == "render"
    if setting == "block_512":
        return kernel.clustered
    if setting == "learned":              # frames of the camera; the counting build it learns with keeps its tables in LDS
        return kernel.call in ("render", "gbuffer") and kernel.options.get("tables") != 2
    if setting == "strip":
        return kernel.call in ("render", "ssaa", "gbuffer")
    return True


CASES = [(k, s) for k in KERNELS for s in SETTINGS if applies(k, s)]


# ---- the references ---------------------------------------------------------------------------------------------------------------

def workers():
    return max(1, min(16, len(os.sched_getaffinity(0))))


def in_chunks(fn, n, chunk):
    """fn(i0, i1) over [0, n) in chunks on the host's cores (the C oracle and numpy release the GIL) -> the parts, in order"""
    bounds = [(i, min(i + chunk, n)) for i in range(0, n, chunk)]
    with ThreadPoolExecutor(max_workers=workers()) as pool:
        return list(pool.map(lambda b: fn(*b), bounds))


@functools.lru_cache(maxsize=None)
def _oracle_columns(scene, W, H, x0, x1):
    out = np.concatenate(in_chunks(lambda a, b: build(scene, "", False)[0].render(W, H, DEPTH[scene], x0 + a, x0 + b), x1 - x0, 24))
    out.setflags(write=False)
    return out


def oracle_frame(scene, W, H, x0=0, x1=None):
    """columns [x0, x1) of the C oracle's W x H frame at the scene's depth, one oracle scene per block of columns: a slice of the
    whole frame, rendered once, or -- less than half of the width -- those columns alone"""
    x1 = W if x1 is None else x1
    if 2 * (x1 - x0) < W:
        return _oracle_columns(scene, W, H, x0, x1)
    return _oracle_columns(scene, W, H, 0, W)[x0:x1]


@functools.lru_cache(maxsize=None)
def rays_of(scene, W, H):
    rays = np.ascontiguousarray(camera_rays(world(scene, "").desc.cam, W, H).reshape(-1, 6))
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def records_of(scene, W, H):
    """query_ref's records of the frame's camera rays, (W * H,)"""
    rays, q = rays_of(scene, W, H), world(scene, "").query
    out = np.concatenate(in_chunks(lambda a, b: query_ref.intersect(q, rays[a:b]), len(rays), 1 << 15))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def segments_of(scene, W, H):
    """from every camera ray's hit point (a miss: the eye) to the first light's centre, then the second's, alternating, with
    query_ref's verdicts"""
    w, hits = world(scene, ""), records_of(scene, W, H)
    L = np.array([w.orc.get_object(k).origin.tuple() for k in (0, 1)], dtype=F)
    P = np.where((hits["object"] >= 0)[:, None], hits["point"], rays_of(scene, W, H)[:, :3]).astype(F)
    segs = np.ascontiguousarray(np.concatenate([P, L[np.arange(len(P)) & 1]], axis=1), dtype=F)
    verdicts = np.concatenate(in_chunks(lambda a, b: query_ref.occluded(w.query, segs[a:b]), len(segs), 1 << 15))
    assert 0.05 < verdicts.mean() < 0.95
    segs.setflags(write=False)
    verdicts.setflags(write=False)
    return segs, verdicts


@functools.lru_cache(maxsize=None)
def ao_records(scene, W, H, n):
    """n records for the AO kernels.  The built-in scene: the frame's.  The field, where query_ref takes ten seconds for a frame
    of this size and ao_ref five: the records of the frame an eighth as wide and high, repeated (their number M is odd, so a
    tile never holds the same ones twice), three in four of them -- by a hash of their number -- turned into misses, which the
    kernel answers with 1.0 without a scan and ao_ref without a query; a tile's lanes are then live and dead in turn"""
    if scene == "builtin":
        return records_of(scene, W, H)[:n]
    base = records_of(scene, W // 8, H // 8)
    M = len(base) - 1 + (len(base) & 1)
    i = np.arange(n, dtype=np.uint64)
    out = base[:M][i % np.uint64(M)].copy()
    out["object"][((i * np.uint64(2654435761)) >> np.uint64(28)) & np.uint64(3) != 0] = -1
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ao_of(scene, W, H, n):
    """ao_ref of ao_records() (record i samples with key i)"""
    q, hits = world(scene, "").query, ao_records(scene, W, H, n)
    out = np.concatenate(in_chunks(lambda a, b: ao_ref.ambient_occlusion(q, hits[a:b], AO_SAMPLES, AO_RADIUS, seed=AO_SEED, key0=a),
                                   n, 1 << 15))
    assert 0 < (out < 1).mean() < 1                              # (not a flat field)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ssaa_frame(scene, W, H, x0, x1):
    out = box_filter(oracle_frame(scene, 2 * W, 2 * H, 2 * x0, 2 * x1), 2)
    out.setflags(write=False)
    return out


# ---- the conditions ---------------------------------------------------------------------------------------------------------------

def ceil_div(a, b):
    return -(-a // b)


def queue_entries(li, cols, rows, twin):
    tiles_x, tiles_z = ceil_div(cols, li.tile_x), ceil_div(rows, li.tile_z)
    return tiles_x * (ceil_div(tiles_z, 2) if twin else tiles_z), tiles_x, tiles_z


def size_condition(r, what, cols, rows, twin, grid_mult):
    """the launch's queue entries against its wavefronts, printed and asserted; cols x rows: the image the launch took its
    decisions on (a strip's columns, the virtual image of a supersampled frame, a batch's grid)"""
    li = r.launch_info()
    entries, tiles_x, tiles_z = queue_entries(li, cols, rows, twin)
    waves = li.grid_blocks * (li.block_threads // 64)
    print(f"[tile schedule] {what}: {cols} x {rows} cells, tiles {li.tile_x} x {li.tile_z}, {tiles_x} x {tiles_z} tiles, "
          f"grid_blocks {li.grid_blocks} x {li.block_threads} threads = {waves} wavefronts, {entries} entries, ratio {entries / waves:.2f}")
    if grid_mult == 0:
        assert waves >= entries and (li.grid_blocks - 1) * (li.block_threads // 64) < entries, (what, waves, entries)
    elif grid_mult == 2:
        assert entries > waves, f"{what}: {entries} entries for {waves} wavefronts: no wavefront needs a second one"
    else:
        assert entries >= 2 * waves, f"{what}: {entries} entries for {waves} wavefronts: fewer than two each, the queues hand out next to nothing"
    return li, tiles_x, tiles_z


def shape_condition(li, what, cols, rows, twin, scale=1):
    """a ragged top macro row (an odd number of tile rows for the twins), macro tiles that do not fill the eight queues evenly,
    neither side a multiple of the tile (a side of `scale` cells -- one pixel -- cannot but divide)"""
    _, tiles_x, tiles_z = queue_entries(li, cols, rows, twin)
    assert tiles_z % 4 != 0 and (not twin or tiles_z % 2 == 1), (what, tiles_z)
    assert (ceil_div(tiles_z, 4) * tiles_x) % 8 != 0, (what, tiles_x, tiles_z)
    assert li.tile_x == scale or cols % li.tile_x != 0, (what, cols, li.tile_x)
    assert li.tile_z == scale or rows % li.tile_z != 0, (what, rows, li.tile_z)


# ---- the cases --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel, setting", CASES, ids=[f"{k.id}-{s}" for k, s in CASES])
def test_every_tile_is_rendered(kernel, setting):
    t_start = time.time()
    options, extra = SETTINGS[setting]
    what = f"{kernel.id} {setting}"
    scene, depth = kernel.scene, DEPTH[kernel.scene]
    W, H = kernel.size
    k = 2 if kernel.call == "ssaa" else 1
    x0, x1 = (STRIP_X0[k], W) if extra == "strip" else (0, W)
    if extra == "third":
        W, x0, x1 = THIRD
        assert (x1 - x0) * 3 <= W
    n = W * H - SHORT                                            # (the batches)
    r = world(scene, "").renderer({**kernel.options, **options})
    try:
        if extra == "learn":
            r.learn_tile_order(W, H, depth)
        if kernel.call == "render":
            want = oracle_frame(scene, W, H, x0, x1)
            got = poisoned.rt_render_device(r, W, H, depth, x0, x1, want)
        elif kernel.call == "ssaa":
            want = ssaa_frame(scene, W, H, x0, x1)
            got = poisoned.rt_render_ssaa_device(r, W, H, depth, 2, x0, x1, want)
        elif kernel.call == "gbuffer":
            want = oracle_frame(scene, W, H, x0, x1)
            want_hits = records_of(scene, W, H).reshape(W, H)[x0:x1]
            got, got_hits = poisoned.rt_render_gbuffer_device(r, W, H, depth, x0, x1, (want, want_hits))
        elif kernel.call == "rays":
            want = oracle_frame(scene, W, H).reshape(-1, 3)[:n]
            got = poisoned.rt_trace_rays_device(r, rays_of(scene, W, H)[:n], H, depth, want)
        elif kernel.call == "hits":
            want_hits = records_of(scene, W, H)[:n]
            got_hits = poisoned.rt_intersect_rays_device(r, rays_of(scene, W, H)[:n], H, want_hits)
        elif kernel.call == "occluded":
            segs, verdicts = segments_of(scene, W, H)
            got_verdicts = poisoned.rt_occluded_rays_device(r, segs[:n], H, verdicts[:n])
        else:
            want = ao_of(scene, W, H, n)
            got = poisoned.rt_ambient_occlusion_device(r, ao_records(scene, W, H, n), H, want, AO_SAMPLES, AO_RADIUS, AO_SEED)
        assert r.kernel_name() == kernel.name, (what, r.kernel_name())
        twin = kernel.name == "rt_render_kernel"
        li, _, _ = size_condition(r, what, k * (x1 - x0), k * H, twin, options.get("grid_mult", 1))
        assert li.block_threads == options.get("block_threads", li.block_threads), (what, li.block_threads)
        # (a supersampled frame's tile holds whole pixels: both sides at least k)
        assert "tile_z" not in options or li.tile_z == min(max(options["tile_z"], k), 64 // k), (what, li.tile_z)
        if extra != "strip":
            shape_condition(li, what, k * (x1 - x0), k * H, twin, k)
        if kernel.call in ("render", "ssaa", "gbuffer", "rays", "ao"):
            assert_same_bits(got, want, what)
        if kernel.call in ("gbuffer", "hits"):
            assert_hits_same(got_hits, want_hits, f"{what}: records")
        if kernel.call == "occluded":
            assert_verdicts_same(got_verdicts, np.asarray(verdicts[:n]), what)
    finally:
        r.close()
    print(f"[tile schedule] {what}: {time.time() - t_start:.2f} s")


def test_the_shapes_are_what_the_docstring_says():
    """the tile arithmetic of the chosen sizes, without a launch: every shape condition under the three tile shapes"""
    Li = namedtuple("Li", "tile_x tile_z")
    for (W, H), twin, k in ((SINGLE, False, 1), (EIGHT, False, 1), (TWIN, True, 1), (SSAA, False, 2)):
        for tile_x, tile_z in ((4, 16), (64 // k, k), (k, 64 // k)):
            shape_condition(Li(tile_x, tile_z), (W, H, tile_x), k * W, k * H, twin, k)
        assert (k * (W - STRIP_X0[k])) % 4 != 0


# ---- the counting build ---------------------------------------------------------------------------------------------------------------

def test_counting_build_over_a_spoilt_framebuffer():
    """rt_render_stats has no device entry point: the handle's framebuffer is first filled with the background colour by a host
    batch of W x H rays aimed away from the scene, so a tile the counting kernel drops holds that colour, which fewer than half
    of the frame's pixels have"""
    scene, (W, H) = "builtin", SINGLE
    depth = DEPTH[scene]
    w = world(scene, "")
    want = oracle_frame(scene, W, H)
    background = np.array(w.desc.null, dtype=F)
    assert (want == background).all(axis=2).mean() < 0.5
    away = np.array([3e4, -5e4, 7e4, 3e4 + 1, -5e4 - 2, 7e4 + 3], dtype=F)
    assert query_ref.intersect(w.query, away[None, :])["object"][0] == -1
    r = w.renderer({})
    try:
        stale = r.trace_rays(np.ascontiguousarray(np.broadcast_to(away, (W * H, 6))), depth, rows=H)
        assert (stale == background).all()
        got, stats = r.render_stats(W, H, depth)
        assert "_stats" in r.kernel_name(), r.kernel_name()
        size_condition(r, "the counting build", W, H, False, 1)
        assert_same_bits(got, want, "rt_render_stats over a framebuffer full of the background colour")
        assert stats["nearest_rays"] >= W * H
    finally:
        r.close()
