"""Compact glass records (include/rt_glass_compact.h) past 2^32 bytes, on the GPU, bit-exact: test_mirror_large_gpu.py's runs
(b), (d), (e) and test_glass_large_gpu.py for the call that walks glass chains over the live rays alone, shaped like them and
built from their helpers.  A tile of M rays (M odd: a tile never aligns with a wavefront or a workgroup) is tiled on the device
to n = 100 000 007 rays and walked by rt_glass_records_compact_device on a side stream with max_bounces 8, min_reflective 0.5 and
min_transmissive 0.5; the reference is glass_ref's outputs of the M rays, tiled the same way and compared as 32-bit words, every
word of every output, a slice of 2^24 rays at a time.  Every output lies between two guards of 1 MiB inside one sentinel-filled
tensor (large_extents.Guarded): after a run the guards still hold the sentinel and no output word does; the rays' checksum is
unchanged.  The info struct must equal what the tiled path words imply for the chunking (mirror_large.tiled_expected_info):
rays, rays_queried, chunks, queries, syncs and all 65 alive[] entries.  The hit queries are the `*_image` hits kernel.

The sizes.  n x 48 = 4.8 GB: the terminal and the guide records each pass 2^32 bytes; n x 24 = 2.4 GB of rays pass 2^31.  What
crosses 2^32 is the BYTE offset: the element indices (12 n words of records, 6 n floats of rays) stay below 2^32.

NOT covered: out_weight past 2^32 bytes (n > 357.9 million rays); out_path past 2^32 bytes (n > 2^30 rays); the 32-bit element
index `6 * ray` past 2^32 (n > 715 827 882 rays); a list of more than 2^28 entries through the call (the scan alone is held to
that size, tests/test_mirror_compact_gpu.py); and the host variant rt_glass_records_compact, whose staging is rt_host.h's and
which would need the batch and its outputs a second time in host memory.

The runs, each with a handle of its own, closed before the next (the scratch lives in the handle and only grows):
  (a) the default chunk, all four outputs, the standard tile (glass_scenes.large_tile, M = 7679): 1 237 029 rays a chunk, 81
      chunks -- the outputs' i0 * 48 passes 2^32 in the chunk loop;
  (b) chunk_rays 90 000 001, all four outputs, the standard tile: 19.5 GB of scratch; the state planes (56 x chunk) and the
      chunk's records (48 x chunk) pass 2^32 bytes; the list of bounce 1 has 62 340 474 entries (69.3 % of the chunk), whose
      243 518 workgroups' counts fill 238 groups of the scan's first level, and a ray's index in the chunk, read back from the
      list, addresses output bytes past 2^32; the tail of 10 000 006 rays runs in the grown buffers, its outputs begin past 2^32;
  (c) as (b) with hits and path only: the GUIDE = false kernels and a state of 4 planes;
  (d) chunk_rays 90 000 001, all four outputs, the tile in which every ray is alive after bounce 0
      (glass_compact_batches.all_alive_tile, M = 5319): the first chunk's list of bounce 1 has 90 000 001 entries, so the LIST's
      records (48 x entries) pass 2^32 bytes and its rays (24 x entries) 2^31 -- the count kernel's rt_glass_decide and the
      FIRST = false step read records[3 i] and rays_k[6 i] of a list past those marks, which no run of a standard tile reaches
      (a list is that long only if more than 89 478 485 of a chunk's rays are alive).  The tile has glass steps, mirror steps
      and ended chains at every query from 1 on, 47 chains cut at the limit, and 15 chains that END on a candidate without a
      child (the bubble's rim, no mirror in the glass room) at query 1 or later: the count must say of each what the step says.
      The standard tile's other 70 such rays end at query 0, are not in this tile, and rest on (b).
      glass_compact_batches.ALL_ALIVE_FIGURES pins the counts; test_glass_compact_cpu.py holds them on the CPU.

Each run prints its wall time, its peak device memory and the info's query_ms and step_ms; no time is asserted."""
import math
import time

import numpy as np
import pytest

import glass_compact_batches as batches
import glass_scenes
import large_extents as le
import mirror_large
from large_extents import Guarded
from mirror_large import WORDS
from test_glass_gpu import renderer_of
from test_large_extents_gpu import SLACK, coprime_prefix, tiled

pytestmark = pytest.mark.gpu
B31, B32 = 1 << 31, 1 << 32
N, ROWS = 100000007, mirror_large.ROOM_H
BOUNCES, FLOOR, LOOK = (glass_scenes.LARGE[name] for name in ("bounces", "floor", "look"))
BIG_CHUNK = 90000001
SLICE_RAYS = 1 << 24
RAY_BYTES = 217                                              # scratch a ray of a chunk: the header's figure
RAY_BYTES_NO_GUIDE = 217 - 2 * 40                            # (a state of 16 bytes for 56 in each of the two lists)
SCAN_BLOCK, BLOCK = 1024, 256                                # csrc/rt_scan.h: counts a group of the scan's first level, entries a count
ALL = ("hits", "guide", "weight", "path")
#       tile, chunk_rays, outputs asked for
RUNS = {"a_default_chunk": ("standard", 0, ALL),
        "b_one_large_chunk": ("standard", BIG_CHUNK, ALL),
        "c_one_large_chunk_hits_and_path_only": ("standard", BIG_CHUNK, ("hits", "path")),
        "d_one_large_chunk_every_ray_alive_after_bounce_0": ("all_alive", BIG_CHUNK, ALL)}


@pytest.fixture(autouse=True)
def measured(request):
    """each run's wall time and peak device memory, printed (pytest -rA shows them)"""
    import torch
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"[glass compact large] {request.node.name}: {time.time() - t0:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tiles():
    """both tiles -- the M rays and their reference as words -- and the preconditions that keep the runs from passing
    vacuously (test_glass_cpu.py and test_glass_compact_cpu.py hold the same on the CPU)"""
    assert (BOUNCES, FLOOR, LOOK) == (8, 0.5, 0.5) == (batches.BOUNCES, batches.FLOOR, batches.LOOK)
    rays, words, details = glass_scenes.large_tile()
    M = len(rays)
    assert M == 7679 and coprime_prefix(rays)[0].shape == rays.shape and math.gcd(M, 256) == 1
    for name, w in words.items():
        assert not (w.view(np.uint32) == np.uint32(le.SENTINEL)).any(), name
    figures = glass_scenes.large_tile_figures(words, details)
    assert figures == glass_scenes.LARGE_FIGURES
    assert figures["childless"] == 85 and min(figures["glass_steps"]) > 0 and figures["cut"] == 47
    assert 0.69 < figures["alive"][1] / M < 0.70 and min(figures["alive"]) > 0
    made = {"standard": (rays, words)}

    rays, words, details = batches.all_alive_tile()
    M = len(rays)
    assert M == 5319 and M % 2 == 1 and math.gcd(M, 256) == 1 and coprime_prefix(rays)[0].shape == rays.shape
    for name, w in words.items():
        assert not (w.view(np.uint32) == np.uint32(le.SENTINEL)).any(), name
    figures = batches.all_alive_tile_figures(words, details)
    assert figures == batches.ALL_ALIVE_FIGURES
    assert figures["alive"][0] == figures["alive"][1] == M and min(figures["alive"]) > 0
    # glass steps, mirror steps and ended chains at every query past 0, so they meet in the workgroups; chains that end on a
    # candidate without a child; chains cut at the limit
    assert min(figures["glass_steps"]) > 0 and min(figures["mirror_steps"]) > 0 and min(figures["ended"][1:]) > 0
    assert figures["childless"] > 0 and figures["ended_childless"] > 0 and figures["cut"] > 0
    made["all_alive"] = (rays, words)
    return made


def run_sizes(tile_words, chunk_rays, asked):
    """-> (chunk, chunks, the scratch's bytes, the expected info), every size the run claims asserted"""
    n = N
    assert n * 48 > B32 and n * 24 > B31 and 12 * n < B32 and 6 * n < B32
    default = (256 << 20) // RAY_BYTES
    assert default == 1237029
    chunk = min(chunk_rays or default, n)
    chunks = -(-n // chunk)
    if chunk_rays:
        assert chunk * 48 > B32 and chunk * 56 > B32 and chunks == 2 and n - chunk == 10000006
    else:
        assert chunks == 81 and (chunks - 1) * chunk * 48 > B32
    scratch = chunk * (RAY_BYTES if "guide" in asked else RAY_BYTES_NO_GUIDE)
    assert not (chunk_rays and "guide" in asked) or 19.5e9 < scratch < 19.6e9
    path = tile_words["path"].view(np.uint32).reshape(-1)
    return chunk, chunks, scratch, mirror_large.tiled_expected_info(path, n, BOUNCES, chunk)


def first_chunk_lists(tile_words, chunk):
    """the first chunk's list sizes per bounce: alive[] of the chunk alone"""
    return mirror_large.tiled_expected_info(tile_words["path"].view(np.uint32).reshape(-1), chunk, BOUNCES)[5]


@pytest.mark.parametrize("run", list(RUNS))
def test_glass_records_compact_past_2_32_bytes(tiles, run):
    import torch
    which, chunk_rays, asked = RUNS[run]
    rays, words = tiles[which]
    M, n = len(rays), N
    chunk, chunks, scratch, want_info = run_sizes(words, chunk_rays, asked)
    if chunk_rays:
        listed = first_chunk_lists(words, chunk)
        assert listed[0] == chunk
        if which == "standard":                              # 62.3 million entries, 238 groups of the scan's first level
            assert listed[1] == 62340474 and 62.3e6 < listed[1] < 62.4e6
            assert 237 * SCAN_BLOCK < -(-listed[1] // BLOCK) <= 238 * SCAN_BLOCK
        else:                                                # the list's own records and rays pass 2^32 and 2^31 bytes
            assert listed[1] == chunk == 90000001 and 48 * listed[1] > B32 and 24 * listed[1] > B31
            assert listed[2] > 0 and min(listed[:BOUNCES + 1]) > 0
    if which == "all_alive":
        assert want_info[5][0] == want_info[5][1] == n
    need = -(-n // M) * M * 24 + sum(Guarded.need(WORDS[name] * n) for name in asked) + scratch + SLACK
    assert need <= 48e9
    le.require_device_memory(need)
    what = f"rt_glass_records_compact_device n={n} tile {which} chunk_rays={chunk_rays} outputs {'+'.join(asked)}"
    r, outs = renderer_of("glass"), {}
    try:
        d_rays = tiled(torch.from_numpy(rays).cuda(), n)
        assert d_rays.is_contiguous() and d_rays.shape == (n, 6)
        ray_words = d_rays.view(torch.int32)
        before = le.checksum(ray_words)
        base = {name: torch.from_numpy(words[name]).cuda() for name in asked}
        outs = {name: Guarded(WORDS[name] * n) for name in asked}
        ptr = lambda name: outs[name].ptr if name in outs else 0
        stream = torch.cuda.Stream()
        assert stream.cuda_stream != 0
        stream.wait_stream(torch.cuda.current_stream())
        r.glass_records_device(n, ROWS, d_rays.data_ptr(), ptr("hits"), ptr("guide"), ptr("weight"), ptr("path"),
                               stream=stream.cuda_stream, max_bounces=BOUNCES, min_reflective=FLOOR, min_transmissive=LOOK,
                               chunk_rays=chunk_rays, compact=True)
        stream.synchronize()
        print(f"[glass compact large] {run}: the hit queries ran {r.kernel_name()}")
        for name in asked:
            outs[name].assert_written(f"{what}: {name}")
        for name in asked:
            w = WORDS[name]
            for c0 in range(0, n, SLICE_RAYS):
                c1 = min(c0 + SLICE_RAYS, n)
                want = mirror_large.tiled_slice(base[name], c0, c1)
                text = le.device_difference(outs[name].body[c0 * w:c1 * w], want, w, f"{what}: {name} (a column is a ray)", c0)
                assert text is None, text
                del want
        assert le.checksum(ray_words) == before, f"{what}: the rays changed"
        i = r.glass_compact_info()
        got = (i.rays, i.rays_queried, i.chunks, i.queries, i.syncs, list(i.alive))
        assert got == want_info, what
        assert got[2] == chunks and len(got[5]) == 65
        assert i.reserved == 0 and i.query_ms > 0 and i.step_ms > 0
        print(f"[glass compact large] {run}: query {i.query_ms:.1f} ms, step {i.step_ms:.1f} ms, rays queried {i.rays_queried}, "
              f"queries {i.queries}, syncs {i.syncs}")
        assert "image" in r.kernel_name() and "hits" in r.kernel_name()
    finally:
        for g in outs.values():
            g.free()
        d_rays = ray_words = base = None
        r.close()
        torch.cuda.empty_cache()
