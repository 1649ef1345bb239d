"""Mirror records (include/rt_mirror.h, include/rt_mirror_compact.h) past 2^32 bytes, on the GPU, bit-exact.  The batch is
the room's 96 x 80 pixel rays, flat, cut to M = 7679 (odd: a tile never aligns with a wavefront or a workgroup) and tiled on the
device to n = 100 000 007 rays, walked with max_bounces 8 and min_reflective 0.5; the reference is mirror_ref's outputs of those M
rays, tiled the same way and compared as 32-bit words, every word of every output, a slice of 2^24 rays at a time -- no second
tensor of an output's size is ever built.  Every output lies between two guards of 1 MiB inside one sentinel-filled tensor
(large_extents.Guarded): after a run the guards still hold the sentinel and no output word does.

The sizes.  n x 48 = 4.8 GB: the terminal and the guide records each pass 2^32 bytes; n x 24 = 2.4 GB of rays pass 2^31.  What
crosses 2^32 is the BYTE offset: the element indices (12 n words of records, 6 n floats of rays) stay below 2^32, as in
test_trace_rays_past_2_32_bytes_in_and_out_three_row_counts.  NOT covered: the 32-bit element index `6 * ray` wraps only for
n > 715 827 882 rays, which together with their records does not fit a test's 48 GB; the weights and the path words pass
2^32 bytes only for n > 357.9 million and n > 2^30.

The runs, each with a handle of its own, closed before the next (the scratch lives in the handle and only grows):
  (a) in place, the default chunk: 2 097 152 rays a chunk, 48 chunks -- the outputs' i0 * 48 passes 2^32 in the chunk loop;
  (b) compact, the default chunk: 1 237 029 rays a chunk, 81 chunks;
  (c) in place, chunk_rays 90 000 001: one chunk whose records (48 x chunk) and whose guide state planes (56 x chunk) pass 2^32
      bytes, then a tail of 10 000 006 rays whose outputs begin past 2^32 bytes;
  (d) compact, chunk_rays 90 000 001: 19.5 GB of scratch -- the lists, the index plane and both lists' buffers at that size; the
      list of bounce 1 has about 43.9 million entries (171 000 workgroups' counts, 168 groups of the scan's first level), and a
      ray's index in the chunk, read back from the list, addresses output bytes past 2^32; the tail reuses the grown buffers;
  (e) as (d) without guide and weight: the GUIDE = false kernels and the state's stride of 4 planes."""
import math
import time

import numpy as np
import pytest

import large_extents as le
import mirror_large
import mirror_scenes
from large_extents import Guarded
from mirror_large import WORDS
from test_large_extents_gpu import SLACK, coprime_prefix, tiled
from tilecoderaytracer_amd import Renderer

pytestmark = pytest.mark.gpu
B31, B32 = 1 << 31, 1 << 32
N, BOUNCES, FLOOR, ROWS = 100000007, 8, 0.5, mirror_large.ROOM_H
BIG_CHUNK = 90000001
SLICE_RAYS = 1 << 24
IN_PLACE_RAY_BYTES, COMPACT_RAY_BYTES = 128, 217             # scratch a ray of a chunk: the headers' figures
COMPACT_RAY_BYTES_NO_GUIDE = 217 - 2 * 40                    # (a state of 16 bytes for 56 in each of the two lists)
#       compact, chunk_rays, outputs asked for
RUNS = {"a_in_place_default_chunk": (False, 0, ("hits", "guide", "weight", "path")),
        "b_compact_default_chunk": (True, 0, ("hits", "guide", "weight", "path")),
        "c_in_place_one_large_chunk": (False, BIG_CHUNK, ("hits", "guide", "weight", "path")),
        "d_compact_one_large_chunk": (True, BIG_CHUNK, ("hits", "guide", "weight", "path")),
        "e_compact_one_large_chunk_no_guide_no_weight": (True, BIG_CHUNK, ("hits", "path"))}


@pytest.fixture(autouse=True)
def measured(request):
    """each run's wall time and peak device memory, printed (pytest -rA shows them)"""
    import torch
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"[mirror large] {request.node.name}: {time.time() - t0:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tile():
    """the M rays, their reference as words, and the preconditions that keep the runs from passing vacuously"""
    rays, words = mirror_large.room_tile(BOUNCES, FLOOR)
    M = len(rays)
    assert M == 7679 and coprime_prefix(rays)[0].shape == rays.shape and math.gcd(M, 256) == 1
    alive, cut = mirror_large.tile_preconditions(words, le.SENTINEL)
    assert alive == [7679, 3742, 1421, 475, 228, 104, 68, 36, 28] and cut == 15
    # so 48.7 % of a chunk is alive at bounce 1, every bounce up to the limit has live rays, and since a workgroup's 256 rays are
    # a thirtieth of a tile, chains that end and chains that go on meet in the workgroups
    assert 0.48 < alive[1] / M < 0.49 and min(alive) > 0
    return rays, words


def chunk_of(compact, chunk_rays):
    default = (256 << 20) // (COMPACT_RAY_BYTES if compact else IN_PLACE_RAY_BYTES)
    assert default == (1237029 if compact else 2097152)
    return min(chunk_rays or default, N)


@pytest.mark.parametrize("run", list(RUNS))
def test_mirror_records_past_2_32_bytes(tile, run):
    import torch
    compact, chunk_rays, asked = RUNS[run]
    rays, words = tile
    M, n = len(rays), N
    assert n * 48 > B32 and n * 24 > B31 and 12 * n < B32 and 6 * n < B32
    chunk = chunk_of(compact, chunk_rays)
    chunks = -(-n // chunk)
    if chunk_rays:
        assert chunk * 48 > B32 and chunk * 56 > B32 and chunks == 2 and n - chunk == 10000006
    else:
        assert chunks == (81 if compact else 48) and (chunks - 1) * chunk * 48 > B32
    per_ray = (COMPACT_RAY_BYTES if "guide" in asked else COMPACT_RAY_BYTES_NO_GUIDE) if compact else IN_PLACE_RAY_BYTES
    scratch = chunk * per_ray
    assert not (compact and chunk_rays and "guide" in asked) or 19.5e9 < scratch < 19.6e9
    if compact and chunk_rays:                               # the first chunk's list of bounce 1, and its workgroups' counts
        listed = mirror_large.tiled_expected_info(words["path"].view(np.uint32).reshape(-1), chunk, BOUNCES)[5][1]
        assert 43.8e6 < listed < 43.9e6 and 167 * 1024 < -(-listed // 256) <= 168 * 1024
    need = -(-n // M) * M * 24 + sum(Guarded.need(WORDS[name] * n) for name in asked) + scratch + SLACK
    le.require_device_memory(need)
    what = f"rt_mirror_records{'_compact' if compact else ''}_device n={n} chunk_rays={chunk_rays} outputs {'+'.join(asked)}"
    r, outs = Renderer(mirror_scenes.host_scene("room")), {}
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
        r.mirror_records_device(n, ROWS, d_rays.data_ptr(), ptr("hits"), ptr("guide"), ptr("weight"), ptr("path"),
                                stream=stream.cuda_stream, max_bounces=BOUNCES, min_reflective=FLOOR, chunk_rays=chunk_rays,
                                compact=compact)
        stream.synchronize()
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
        if compact:
            i = r.mirror_compact_info()
            got = (i.rays, i.rays_queried, i.chunks, i.queries, i.syncs, list(i.alive))
            assert got == mirror_large.tiled_expected_info(words["path"].view(np.uint32).reshape(-1), n, BOUNCES, chunk), what
            assert i.reserved == 0 and i.query_ms > 0 and i.step_ms > 0
        else:
            i = r.mirror_info()
            assert (i.rays, i.chunks, i.queries) == (n, chunks, chunks * (BOUNCES + 1)), what
            assert i.query_ms > 0 and i.step_ms > 0
        print(f"[mirror large] {run}: query {i.query_ms:.1f} ms, step {i.step_ms:.1f} ms")
    finally:
        for g in outs.values():
            g.free()
        d_rays = ray_words = base = None
        r.close()
        torch.cuda.empty_cache()
