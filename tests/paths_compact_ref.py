"""What include/rt_paths_compact.h says a call launches and counts, for the tests: the header's COUNTS rule applied to a
paths_ref.Walk's per-path alive masks chunk by chunk, and the batches the tests of tests/test_paths_compact_gpu.py are built from --
each built here once, so that tests/test_paths_compact_cpu.py can hold on the CPU oracle the conditions the GPU comparisons rest
on.  The output words have no reference of their own: they are rt_indirect_paths' (paths_ref)."""
import numpy as np

import adaptive_frames
import indirect_ref
import paths_ref
from tilecoderaytracer_amd.renderer import HIT_DTYPE

F = np.float32
PATH_BYTES = 141                                   # the header's SCRATCH: a path's 140 bytes and the counts, reckoned as one more
CHUNK_BYTES = 256 << 20
MAX_BATCH_RAYS = 0x7FFFFFFF - 64
LIST_SIZES = (1, 63, 64, 65, 255, 256, 257)        # a wavefront's and a workgroup's edges
LIST_KW = dict(n=1, gather_depth=1, gain=1.0, seed=5)      # the list-size construction's walk
SKY_KW = dict(n=3, gather_depth=1, gain=1.0, seed=2)       # tests/test_paths_gpu.py's, for the sky-facing records
SCAN_GROUP = 262144                                # entries one group of the scan covers: 1024 counts of 256


def chunk_of(chunk_records, N, S):
    """the records of a chunk: the caller's, or the header's default"""
    c = chunk_records if chunk_records > 0 else max(1, CHUNK_BYTES // (PATH_BYTES * S))
    return min(c, MAX_BATCH_RAYS // S, N)


def paths_compact_expect(walk, chunk_records, B, emitters):
    """the header's COUNTS of rt_indirect_paths_compact over walk's batch -> dict(records, rays, chunks, traces, queries, syncs,
    alive, runs): per chunk the bounces run are 1 + |{b in 1..B-1: the chunk's alive[b] > 0}|; traces their sum; queries the same
    minus one for every chunk that ran bounce B-1 with emitters; syncs the bounces run minus 1 if the chunk ran all B; rays the
    records * S plus the sum of alive[b >= 1].  runs: the bounces run of every chunk, in order."""
    walk.extend(B)
    N, S = int(np.asarray(walk.hits).size), walk.S
    chunk = chunk_of(int(chunk_records), N, S)
    out = dict(records=N, rays=0, chunks=0, traces=0, queries=0, syncs=0, alive=[int(a.sum()) for a in walk.alive[:B]], runs=[])
    for i0 in range(0, N, chunk):
        paths = slice(i0 * S, min(i0 + chunk, N) * S)
        counts = [int(walk.alive[b][paths].sum()) for b in range(B)]
        assert all(counts[b] >= counts[b + 1] for b in range(B - 1)), counts          # (a path never comes back)
        run = 1 + sum(1 for b in range(1, B) if counts[b] > 0)
        out["runs"].append(run)
        out["chunks"] += 1
        out["traces"] += run
        out["queries"] += run - (1 if run == B and emitters else 0)
        out["syncs"] += run - (1 if run == B else 0)
        out["rays"] += (paths.stop - paths.start) + sum(counts[1:run])
    return out


def info_of(info, B):
    """an RtPathsCompactInfo's counts in paths_compact_expect's names"""
    return dict(records=int(info.records), rays=int(info.rays), chunks=int(info.chunks), traces=int(info.traces),
                queries=int(info.queries), syncs=int(info.syncs), alive=[int(v) for v in info.alive[:B]])


def builtin_records():
    """the built-in 61 x 37 frame's records, flat, writable"""
    frame = {f[0]: f for f in indirect_ref.FRAMES}["builtin"]
    return np.array(indirect_ref.oracle_gather(*frame)[1], dtype=HIT_DTYPE, order="C").reshape(-1)


def going_on(walk_of):
    """the built-in records flat, walked ONCE by walk_of(records) -> a paths_ref.Walk of LIST_KW: the records (n = 1: the paths)
    whose path goes on after bounce 0, ascending"""
    on = np.flatnonzero(walk_of(builtin_records()).extend(2).alive[1])
    assert len(on) > max(LIST_SIZES), len(on)
    return on


def list_of_size(c, on):
    """the list-size construction from on = going_on(...): the first c records whose path goes on after bounce 0 are kept, the
    OTHER going-on records are marked dead (object = -1: a dead record changes no other path's key) and the records whose path
    ends at bounce 0 are left -> the records, of which exactly c have a path alive at bounce 1"""
    out = builtin_records()
    out["object"][on[c:]] = -1
    return out


def sky_records(count=300):
    """tests/test_paths_gpu.py's records high above the built-in scene that look away from it: every gather ray misses"""
    rng = np.random.RandomState(8)
    hits = np.zeros(count, dtype=HIT_DTYPE)
    hits["object"] = 4
    hits["point"] = (np.array([0.0, 0.0, 1000.0]) + rng.uniform(-5, 5, (count, 3))).astype(F)
    hits["normal"] = (0.0, 0.0, 1.0)
    hits["color"] = rng.uniform(0.2, 1, (count, 3)).astype(F)
    hits["distance"] = F(1.0)
    return hits


def two_chunk_batch():
    """300 sky-facing records, whose paths all end at their first ray, then 300 built-in records: with chunk_records = 300 one
    chunk that runs one bounce and one that runs them all"""
    return np.concatenate([sky_records(300), builtin_records()[600:900]])


def oracle_walk_of(hits, n, gather_depth=1, gain=1.0, seed=0, key0=0):
    """the Walk of a batch of records over the built-in scene on the CPU oracle"""
    orc = adaptive_frames.oracle_scene("builtin")
    w = paths_ref.Walk(paths_ref.oracle_tracer(orc, gather_depth), hits, n, indirect_ref.object_diffuse(orc), gain, seed, key0)
    w.orc = orc
    return w
