"""Glass records (include/rt_glass.h) past 2^32 bytes, on the GPU, bit-exact: test_mirror_large_gpu.py's test for the call
that looks through glass, shaped like it and built from its helpers.  The batch is the glass room's 96 x 80 pixel rays, flat, cut
to M = 7679 (odd: a tile never aligns with a wavefront or a workgroup) and tiled on the device to n = 100 000 007 rays, walked
with max_bounces 8, min_reflective 0.5 and min_transmissive 0.5; the reference is glass_ref's outputs of those M rays
(glass_scenes.large_tile, whose chains test_glass_cpu.py pins), tiled the same way and compared as 32-bit words, every word of
every output, a slice of 2^24 rays at a time.  Every output lies between two guards of 1 MiB inside one sentinel-filled tensor
(large_extents.Guarded): after a run the guards still hold the sentinel and no output word does.  The scene is refractive and
therefore packed as an image scene, so the hit queries of these runs are the `*_image` hits kernel (each run prints its name),
not the kernel test_mirror_large_gpu.py's non-refractive room runs.

The sizes.  n x 48 = 4.8 GB: the terminal and the guide records each pass 2^32 bytes; n x 24 = 2.4 GB of rays pass 2^31.  What
crosses 2^32 is the BYTE offset: the element indices (12 n words of records, 6 n floats of rays) stay below 2^32.

NOT covered: the weights and the path words past 2^32 bytes (n > 357.9 million and n > 2^30 rays); the 32-bit element index
`6 * ray`, which wraps only for n > 715 827 882 rays; and the host variant rt_glass_records, whose staging is rt_host.h's and
which would need the batch and its outputs a second time in host memory.

The runs, each with a handle of its own, closed before the next (the scratch lives in the handle and only grows):
  (a) the default chunk, all four outputs: 2 097 152 rays a chunk, 48 chunks -- the outputs' i0 * 48 passes 2^32 in the chunk
      loop;
  (b) chunk_rays 90 000 001, all four outputs: one chunk whose records (48 x chunk) and whose guide state planes (56 x chunk)
      pass 2^32 bytes -- 11.5 GB of scratch -- then a tail of 10 000 006 rays whose outputs begin past 2^32 bytes;
  (c) as (b) with hits and path only: the GUIDE = false instantiations of the step and the state's stride of 4 planes."""
import math
import time

import numpy as np
import pytest

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
RAY_BYTES, RAY_BYTES_NO_GUIDE = 128, 88                      # scratch a ray of a chunk: record, next ray, 14 or 4 state planes
#       chunk_rays, outputs asked for
RUNS = {"a_default_chunk": (0, ("hits", "guide", "weight", "path")),
        "b_one_large_chunk": (BIG_CHUNK, ("hits", "guide", "weight", "path")),
        "c_one_large_chunk_hits_and_path_only": (BIG_CHUNK, ("hits", "path"))}


@pytest.fixture(autouse=True)
def measured(request):
    """each run's wall time and peak device memory, printed (pytest -rA shows them)"""
    import torch
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"[glass large] {request.node.name}: {time.time() - t0:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 1e9:.2f} GB")
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def tile():
    """the M rays, their reference as words, and the preconditions that keep the runs from passing vacuously"""
    rays, words, details = glass_scenes.large_tile()
    M = len(rays)
    assert M == 7679 and coprime_prefix(rays)[0].shape == rays.shape and math.gcd(M, 256) == 1
    assert (BOUNCES, FLOOR, LOOK) == (8, 0.5, 0.5)
    for name, w in words.items():
        assert not (w.view(np.uint32) == np.uint32(le.SENTINEL)).any(), name
    figures = glass_scenes.large_tile_figures(words, details)
    assert figures == glass_scenes.LARGE_FIGURES
    # so 69.3 % of a chunk is alive at bounce 1, every bounce up to the limit has live rays and glass steps, and since a
    # workgroup's 256 rays are a thirtieth of a tile, glass steps, mirror steps and ended chains meet in the workgroups
    assert 0.69 < figures["alive"][1] / M < 0.70 and min(figures["alive"]) > 0 and min(figures["glass_steps"]) > 0
    return rays, words


@pytest.mark.parametrize("run", list(RUNS))
def test_glass_records_past_2_32_bytes(tile, run):
    import torch
    chunk_rays, asked = RUNS[run]
    rays, words = tile
    M, n = len(rays), N
    assert n * 48 > B32 and n * 24 > B31 and 12 * n < B32 and 6 * n < B32
    default = (256 << 20) // RAY_BYTES
    assert default == 2097152
    chunk = min(chunk_rays or default, n)
    chunks = -(-n // chunk)
    if chunk_rays:
        assert chunk * 48 > B32 and chunk * 56 > B32 and chunks == 2 and n - chunk == 10000006
    else:
        assert chunks == 48 and (chunks - 1) * chunk * 48 > B32
    scratch = chunk * (RAY_BYTES if "guide" in asked else RAY_BYTES_NO_GUIDE)
    assert not (chunk_rays and "guide" in asked) or 11.5e9 < scratch < 11.6e9
    need = -(-n // M) * M * 24 + sum(Guarded.need(WORDS[name] * n) for name in asked) + scratch + SLACK
    le.require_device_memory(need)
    what = f"rt_glass_records_device n={n} chunk_rays={chunk_rays} outputs {'+'.join(asked)}"
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
                               chunk_rays=chunk_rays)
        stream.synchronize()
        print(f"[glass large] {run}: the hit queries ran {r.kernel_name()}")
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
        i = r.glass_info()
        assert (i.rays, i.chunks, i.queries) == (n, chunks, chunks * (BOUNCES + 1)), what
        assert i.query_ms > 0 and i.step_ms > 0
        print(f"[glass large] {run}: query {i.query_ms:.1f} ms, step {i.step_ms:.1f} ms")
        assert "image" in r.kernel_name() and "hits" in r.kernel_name()
    finally:
        for g in outs.values():
            g.free()
        d_rays = ray_words = base = None
        r.close()
        torch.cuda.empty_cache()
