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
