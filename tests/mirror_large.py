"""Shared by the mirror-record tests (include/rt_mirror.h, include/rt_mirror_compact.h): what rt_mirror_compact_info must say of
a call, from the path words of its batch -- of the batch itself (expected_info), and of a batch that is M path words tiled to n
rays, without ever building the n words (tiled_expected_info: test_mirror_compact_cpu.py proves the two equal) -- and the batch
of test_mirror_large_gpu.py: the room's rays and their reference as words, and the slices of either tiled on the device."""
import numpy as np

import mirror_ref
import mirror_scenes

F = np.float32
MAX_BOUNCES = mirror_ref.MAX_BOUNCES


def expected_info(path, bounces, chunk=0):
    """from the path words of a batch, in ray order: what rt_mirror_compact_info must say of a call that walks it in chunks of
    `chunk` rays (0: one chunk) -> (rays, rays_queried, chunks, queries, syncs, alive[0 .. 64])"""
    k = mirror_ref.unpack(np.asarray(path))[0].reshape(-1)
    n = len(k)
    chunk = chunk or n
    alive, queries, syncs, chunks = [0] * 65, 0, 0, 0
    for i0 in range(0, n, chunk):
        mine = [int((k[i0:i0 + chunk] >= b).sum()) for b in range(bounces + 1)]
        q = sum(1 for a in mine if a > 0)
        queries, syncs, chunks = queries + q, syncs + q - (1 if q == bounces + 1 else 0), chunks + 1
        alive = [a + m for a, m in zip(alive, mine + [0] * 65)]
    return n, sum(alive), chunks, queries, syncs, alive


def tiled_expected_info(path, n, bounces, chunk=0):
    """expected_info(tile, bounces, chunk) of the n words tile[i] = path[i % M], M = len(path), in closed form: the rays of
    [0, x) whose chain reaches query b number (x // M) T_b + P_b[x % M], where P_b[t] counts them among path[:t] and T_b = P_b[M];
    a chunk [i0, i1) has the difference of the two.  O(bounces x (M + chunks)) work, and nothing of n words is built."""
    k = mirror_ref.unpack(np.asarray(path))[0].reshape(-1)
    M, n = len(k), int(n)
    assert M > 0 and n > 0 and 0 <= bounces <= MAX_BOUNCES
    chunk = int(chunk) or n
    prefix = np.zeros((bounces + 1, M + 1), dtype=np.int64)
    for b in range(bounces + 1):
        prefix[b, 1:] = np.cumsum(k >= b)
    starts = np.arange(0, n, chunk, dtype=np.int64)
    ends = np.minimum(starts + chunk, n)
    before = lambda x: (x // M)[None, :] * prefix[:, -1:] + prefix[:, x % M]          # (bounces + 1, chunks)
    mine = before(ends) - before(starts)
    q = (mine > 0).sum(axis=0)                               # (a chunk's live rays never grow with b: its first q bounces)
    alive = [int(a) for a in mine.sum(axis=1)] + [0] * (MAX_BOUNCES - bounces)
    return n, sum(alive), len(starts), int(q.sum()), int((q - (q == bounces + 1)).sum()), alive


# ---- the batch of test_mirror_large_gpu.py ------------------------------------------------------------------------------------

ROOM_W, ROOM_H = mirror_scenes.SIZES[1]
TILE_RAYS = ROOM_W * ROOM_H - 1                              # 7679: odd, so a tile never aligns with a wavefront or a workgroup
WORDS = dict(hits=12, guide=12, weight=3, path=1)            # 32-bit words a ray of each output


def room_tile(bounces, floor, reference=None):
    """the room's 96 x 80 pixel rays, flat, cut to TILE_RAYS -> (rays float32 (M, 6), {output: its reference as int32 words
    (M, words a ray)}), of mirror_scenes.reference -- a ray's result depends on that ray alone (include/rt_mirror.h).
    reference: another call's, as (the (ROOM_W, ROOM_H, 6) pixel rays, its four outputs of them) -- test_glass_large_gpu.py's
    is glass_scenes'; its path words keep k and cut where rt_mirror.h has them, which is all tile_preconditions reads of them"""
    M = TILE_RAYS
    frame, want = reference or (mirror_scenes.pixel_rays("room", ROOM_W, ROOM_H),
                                mirror_scenes.reference("room", ROOM_W, ROOM_H, bounces, floor))
    rays = np.array(frame, dtype=F, order="C").reshape(-1, 6)[:M]
    assert np.shape(frame) == (ROOM_W, ROOM_H, 6)
    words = {name: np.ascontiguousarray(a).reshape(ROOM_W * ROOM_H, -1)[:M].copy().view(np.int32).reshape(M, w)   # (a copy: the
             for (name, w), a in zip(WORDS.items(), want[:4])}                                # reference itself is read-only)
    return rays, words


def tile_preconditions(words, sentinel=0x7FC5A5A5):
    """what the large test needs of room_tile()'s reference, so that it cannot pass vacuously: no output holds the sentinel word
    (large_extents.SENTINEL) or a NaN, whose bits a kernel need not reproduce -> (the chains of length >= b for b = 0 .. 8, the
    chains cut at the limit).  The words may be rt_glass.h's as well: k and cut lie where rt_mirror.h's do."""
    for name, w in words.items():
        assert not (w.view(np.uint32) == np.uint32(sentinel)).any(), f"the reference's {name} holds the sentinel"
    for name in ("hits", "guide"):
        assert not np.isnan(words[name].view(F)[:, 1:11]).any(), f"the reference's {name} holds a NaN"
    assert not np.isnan(words["weight"].view(F)).any()
    k, cut, _ = mirror_ref.unpack(words["path"].view(np.uint32).reshape(-1))
    return [int((k >= b).sum()) for b in range(9)], int(cut.sum())


def tiled_slice(base, c0, c1):
    """rows [c0, c1) of the device tensor (M, k) tiled along its first axis -- row i is base[i % M] -- flat"""
    import torch
    at = torch.arange(c0, c1, dtype=torch.int64, device=base.device) % base.shape[0]
    return base[at].reshape(-1)
