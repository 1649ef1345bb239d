"""The batches of test_glass_compact_gpu.py that are cut from the glass room's rays (include/rt_glass_compact.h), here so that
test_glass_compact_cpu.py can hold them to what the GPU test needs of them: batches whose dense list at query 1 or 2 has exactly
c entries, for c at the edges of a wavefront and of a workgroup, the survivors all glass steps or all mirror steps, interleaved
with chains that end one query sooner; and the batch in which every ray is alive after bounce 0.  A ray's result depends on that
ray alone (include/rt_glass.h), so a batch's reference is the frame's reference at the batch's indices."""
import functools

import numpy as np

import glass_ref
import glass_scenes

W96, H80 = glass_scenes.SIZES[1]
BOUNCES, FLOOR, LOOK = 8, 0.5, 0.5
LIST_SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
ENDING = 300                                   # the chains that end one query sooner, among which the c are spread
KINDS = ("glass", "mirror")


def handmade_rays():
    """test_glass_gpu.py's: misses, an E == T ray, starts inside the glass sphere, the bubble's rim"""
    from test_glass_gpu import handmade_rays as made
    return made()


def interleave(few, many):
    """the indices `few` spread evenly among the indices `many`, both kept in their order (test_mirror_compact_gpu.py's)"""
    out = list(many)
    for j, i in enumerate(few):
        out.insert((j * (len(many) + 1)) // max(len(few), 1) + j, i)
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def chains():
    """the glass room's 96 x 80 rays at floor 0.5 and look 0.5, flat -> dict(rays (n, 6), want: the four outputs flat, k (n,),
    glass (n, 8): step s of the chain was a glass step)"""
    n = W96 * H80
    ref = glass_scenes.reference("glass", W96, H80, BOUNCES, FLOOR, LOOK)
    want = [np.asarray(a).reshape((n,) + np.asarray(a).shape[2:]) for a in ref[:4]]
    k = glass_ref.unpack(want[3])[0]
    rays = np.array(glass_scenes.pixel_rays("glass", W96, H80), dtype=np.float32, order="C").reshape(-1, 6)
    return dict(rays=rays, want=want, k=k, glass=ref[4]["glass"].reshape(n, -1))


def list_size_batch(bounce, c, kind):
    """-> the indices of ENDING rays whose chain ends at query bounce - 1 with, spread among them, c rays whose chain reaches
    query `bounce` by a step of `kind` ("glass" or "mirror") at query bounce - 1"""
    ch = chains()
    k, glass = ch["k"], ch["glass"]
    go_on = np.flatnonzero((k >= bounce) & (glass[:, bounce - 1] == (kind == "glass")))
    end = np.flatnonzero(k == bounce - 1)
    assert len(go_on) >= max(LIST_SIZES) and len(end) >= ENDING, (bounce, kind, len(go_on), len(end))
    pick = interleave(go_on[:: len(go_on) // max(LIST_SIZES)][:c], end[:: len(end) // ENDING][:ENDING])
    assert len(pick) == ENDING + c and len(set(pick.tolist())) == ENDING + c
    return pick


def all_alive_batch():
    """-> the indices of every ray that follows something, in ray order"""
    return np.flatnonzero(chains()["k"] >= 1)


# ---- the tile of test_glass_compact_large_gpu.py's run (d) and the chunks of "open" ---------------------------------------------

# all_alive_tile_figures() of all_alive_tile(): test_glass_compact_cpu.py holds the reference to them, the large test asserts them
# again.  childless: rays that met a candidate without a child; ended_childless: chains that END on one (the bubble's rim, which
# is no mirror in the glass room) without being cut -- here the same 15 rays, all past query 0; the standard tile's other 70
# childless rays end at query 0 and are not in this tile
ALL_ALIVE_FIGURES = dict(alive=[5319, 5319, 2632, 1039, 577, 288, 148, 111, 64], cut=47, g=3495,
                         glass_steps=[3007, 288, 367, 177, 76, 55, 24, 23], mirror_steps=[2312, 2344, 672, 400, 212, 93, 87, 41],
                         ended=[0, 2687, 1593, 462, 289, 140, 37, 47, 64], childless=15, ended_childless=15)


def all_alive_tile():
    """run (d)'s tile: the 5319 rays of all_alive_batch(), flat and in ray order -> (rays float32 (M, 6), {output: its reference
    as int32 words (M, words a ray)} -- mirror_large.room_tile's format, the frame's reference at the batch's indices -- and the
    reference's details of those rays)"""
    from mirror_large import WORDS
    ch, pick = chains(), all_alive_batch()
    M = len(pick)
    rays = np.ascontiguousarray(ch["rays"][pick])
    words = {name: np.ascontiguousarray(a[pick]).view(np.int32).reshape(M, w) for (name, w), a in zip(WORDS.items(), ch["want"])}
    ref = glass_scenes.reference("glass", W96, H80, BOUNCES, FLOOR, LOOK)
    details = {name: a.reshape((W96 * H80,) + a.shape[2:])[pick] for name, a in ref[4].items()}
    return rays, words, details


def all_alive_tile_figures(words, details):
    """what run (d) needs of all_alive_tile()'s reference, so that it cannot pass vacuously: mirror_large.tile_preconditions (no
    sentinel word, no NaN in a float field; the chains of length >= b, the chains cut at the limit), the glass steps and the
    mirror steps per bounce, the chains that end at each query, the rays that met a candidate without a child, and those whose
    chain ended on one"""
    import mirror_large
    alive, cut = mirror_large.tile_preconditions(words)
    k = glass_ref.unpack(words["path"].view(np.uint32).reshape(-1))[0]
    glass = details["glass"]
    taken = np.arange(glass.shape[1])[None, :] < k[:, None]                  # step s of the chain was taken at all
    hits = words["hits"]
    scene = glass_scenes.ref_scene("glass")
    tf = glass_ref.transmissive(scene)[0]
    o, flags = hits[:, 0], hits[:, 11]
    at_end = (o >= 0) & (flags & 2 == 0) & (tf[np.clip(o, 0, None)] > 0) & (tf[np.clip(o, 0, None)] >= np.float32(LOOK))
    return dict(alive=alive, cut=cut, g=int(details["g"].sum()), glass_steps=[int(c) for c in (glass & taken).sum(0)],
                mirror_steps=[int(c) for c in (~glass & taken).sum(0)],
                ended=[int((k == b).sum()) for b in range(BOUNCES + 1)], childless=int((details["childless"] > 0).sum()),
                ended_childless=int((at_end & ~details["cut"]).sum()))


OPEN_CHUNKS = (7, 64, 300, 600, 1000)           # chunk_rays of the tests on "open" at 61 x 37
OPEN_CHUNKS_NO_LATER_CHUNK_GOES_FURTHER = (1000,)
W61, H37 = glass_scenes.SIZES[0]


def queries_per_chunk(path, bounces, chunk):
    """from a batch's path words in ray order: the hit queries each chunk of `chunk` rays runs -- the number of b <= bounces
    for which the chunk has a ray whose chain reached query b (include/rt_glass_compact.h, EARLY END)"""
    k = glass_ref.unpack(np.asarray(path))[0].reshape(-1)
    return [sum(1 for b in range(bounces + 1) if (k[i0:i0 + chunk] >= b).any()) for i0 in range(0, len(k), chunk)]


def assert_chunks_end_at_different_bounces(path, bounces, chunk):
    """what the chunk tests on "open" need of the path words: the chunks do not all run the same number of queries, some chunk
    ends early -- a bounce at which it has no live ray -- and a LATER chunk runs more queries than it, so the call must start
    that chunk at bounce 0 with both lists' roles and the count as they were at the call's start -> the queries per chunk.
    In chunks of 1000 the 2257 rays run 4, 4 and 3 queries: no later chunk goes further than an earlier one, so of that size
    only the first is asked, and at max_bounces 8 (where 4 queries are an early end) that an early end has a chunk after it;
    600 (3, 4, 3, 4 queries) stands beside it as the large chunk of which everything holds."""
    q = queries_per_chunk(path, bounces, chunk)
    assert len(set(q)) > 1, (chunk, q)
    if chunk in OPEN_CHUNKS_NO_LATER_CHUNK_GOES_FURTHER:
        assert q == [4, 4, 3] and (bounces < 4 or q[0] <= bounces), (chunk, q)
        return q
    assert any(a <= bounces and max(q[j + 1:], default=0) > a for j, a in enumerate(q)), (chunk, q)
    assert {a % 2 for a in q[:-1]} == {0, 1}, (chunk, q)     # chunks that stop on either list are followed by another
    return q
