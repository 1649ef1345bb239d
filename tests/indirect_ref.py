"""The reference of include/rt_capi_indirect.h, for the tests: the header's definition restated in numpy fp32, one rounding per
operation, the sums in the order written.  The directions are ao_ref's (the header refers to rt_capi_ao.h's formulae; they are
not derived a second time), the gather rays' colours rays_ref.oracle_trace's, their first hits query_ref.intersect's -- and the
frames the GPU tests compare with the CPU oracle, each computed once."""
import functools

import numpy as np

import adaptive_frames
import ao_ref
import query_ref
import rays_ref

F = np.float32
HIT_LIGHT = ao_ref.HIT_LIGHT
NULL_COLOR = F(0.75)                    # the reference's colour of a miss


def rays(hits, n, seed=0, key0=0):
    """the header's gather rays of the records hits (HIT_DTYPE, any shape) -> (float32 hits.shape + (S, 6), ray [..., s] =
    {P, add(P, D)}, a dead record's all +0.0; the mask of the live records, hits.shape)"""
    P = ao_ref.frames(hits)[0]
    D = ao_ref.directions(hits, n, seed, key0)
    with np.errstate(all="ignore"):
        T = P[:, None, :] + D
    live = ao_ref.live_records(hits)
    out = np.concatenate([np.broadcast_to(P[:, None, :], T.shape), T], axis=2).astype(F)
    out[~live] = F(0)
    shape = np.shape(hits)
    return np.ascontiguousarray(out).reshape(shape + (n * n, 6)), live.reshape(shape)


def resolve(colours, light_first, kd, hits, gain, base=None, emitters=False):
    """the header's out_rgb: colours float32 hits.shape + (S, 3) of the gather rays; light_first bool hits.shape + (S,), whether
    a ray's first hit is a light (read with emitters False only; None allowed otherwise); kd float32 per Scene object; base None
    or float32 hits.shape + (3,) -> float32 hits.shape + (3,)"""
    shape = np.shape(hits)
    flat = np.ascontiguousarray(hits).reshape(-1)
    S = colours.shape[-2]
    c = np.array(colours, dtype=F, copy=True).reshape(len(flat), S, 3)
    if not emitters:
        c[np.asarray(light_first, dtype=bool).reshape(len(flat), S)] = F(0)
    with np.errstate(all="ignore"):
        acc = c[:, 0, :].copy()
        for s in range(1, S):
            acc = acc + c[:, s, :]
        mean = acc / F(S)
        obj = flat["object"]
        kd = np.asarray(kd, dtype=F)
        k = np.zeros(len(flat), dtype=F)                    # 0.0f for an object the scene does not have
        known = (obj >= 0) & (obj < len(kd))
        k[known] = kd[obj[known]]
        w = (flat["color"].astype(F) * k[:, None]) * F(gain)
        term = np.where(ao_ref.live_records(hits)[:, None], w * mean, F(0)).astype(F)
        out = term if base is None else np.asarray(base, dtype=F).reshape(len(flat), 3) + term
    return np.ascontiguousarray(out, dtype=F).reshape(shape + (3,))


def object_diffuse(orc):
    """the `diffuse` of every object of an oracle scene, float32"""
    return np.array([orc.get_object(i).diffuse for i in range(orc.object_count)], dtype=F)


def gather(orc, hits, n, seed, key0, gather_depth):
    """-> (colours hits.shape + (S, 3), light_first hits.shape + (S,)) of the gather rays, from the CPU oracle; a dead
    record's rays are not traced (their colours count for nothing): zeros and False"""
    r, live = rays(hits, n, seed, key0)
    colours = np.zeros(r.shape[:-1] + (3,), dtype=F)
    light = np.zeros(r.shape[:-1], dtype=bool)
    colours[live] = rays_ref.oracle_trace(orc, r[live], gather_depth)
    light[live] = (query_ref.intersect(query_ref.Scene(orc), r[live])["flags"] & HIT_LIGHT) != 0
    return colours, light


def indirect(orc, hits, n, gather_depth=1, gain=1.0, seed=0, key0=0, emitters=False, base=None, kd=None):
    """rt_indirect_diffuse of the records hits on the oracle scene orc -> float32 hits.shape + (3,); kd: the objects' diffuse
    in place of the scene's own (the issue's table was made with all ones)"""
    colours, light = gather(orc, hits, n, seed, key0, gather_depth)
    return resolve(colours, light, object_diffuse(orc) if kd is None else kd, hits, gain, base, emitters)


# ---- the frames compared with the CPU oracle: (key, W, H, depth, n, seed, gather_depth) ----------------------------------------
FRAMES = [
    ("builtin", 61, 37, 4, 3, 0, 2),
    ("grid16", 48, 44, 4, 2, 7, 2),
    ("random2", 36, 28, 4, 2, 0x9E3779B9, 1),
    ("twomirrors", 40, 36, 4, 2, 1, 2),
    ("random3", 36, 28, 4, 2, 1, 2),
]
# The conditions (a test must not pass on an empty term): at least 0.5 of the live records with a nonzero term and at least 200
# distinct colours, with the objects' diffuse applied.  Measured on the CPU oracle:
#     builtin 0.834 / 1880    grid16 0.737 / 1521    random2 0.949 / 225    twomirrors 0.463 / 272    random3 0.941 / 950
# twomirrors misses the first bar whatever the seed (seeds 1 and 2, n 2 and 3: 0.463 each): more than half of what its camera
# sees are the mirrors themselves, whose diffuse is 0, so that their term is exactly 0.  It stays among the frames compared bit
# for bit; random3 was added for the conditions in its place.
CONDITION_FRAMES = [f for f in FRAMES if f[0] != "twomirrors"]
# The frame of the `emitters` flag.  The built-in scene is the only one where gather rays meet a light first; on its 61 x 37
# frame they are 38 of 20 286 rays on 29 records, 27 of which get another term (two lie on mirrors) -- fewer than the 100
# differing records asked for whatever the code does.  The same scene, depth, n, seed and gather depth at 131 x 79: 152 rays on
# 120 records, 115 of which differ.
EMITTER_FRAME = ("builtin", 131, 79, 4, 3, 0, 2)


@functools.lru_cache(maxsize=None)
def oracle_gather(key, W, H, depth, n, seed, gather_depth):
    """-> (rgb, hits, colours, light_first, kd) of a frame of FRAMES, read-only: the oracle's frame and records
    (adaptive_frames.first_pass) and its gather rays' colours and first-hit flags"""
    orc = adaptive_frames.oracle_scene(key)
    rgb, hits = adaptive_frames.first_pass(key, W, H, depth)
    colours, light = gather(orc, hits, n, seed, 0, gather_depth)
    kd = object_diffuse(orc)
    for a in (colours, light, kd):
        a.setflags(write=False)
    return rgb, hits, colours, light, kd


def oracle_term(frame, emitters, with_base, gain=1.0):
    key, W, H, depth, n, seed, gather_depth = frame
    rgb, hits, colours, light, kd = oracle_gather(*frame)
    return resolve(colours, light, kd, hits, gain, rgb if with_base else None, emitters)


def check_conditions(frame):
    """a frame's term, emitters 0 and no base, is not empty: at least half of the live records nonzero, 200 distinct colours"""
    hits = oracle_gather(*frame)[1]
    term = oracle_term(frame, False, False)
    assert np.isfinite(term).all()
    assert nonzero_share(term, hits) >= 0.5, (frame, nonzero_share(term, hits))
    assert distinct_colours(term) >= 200, (frame, distinct_colours(term))


def check_emitter_frame():
    """the two `emitters` results of EMITTER_FRAME differ on at least 100 records, and those of the 61 x 37 frame on some"""
    for frame, least in ((EMITTER_FRAME, 100), (FRAMES[0], 1)):
        off, on = oracle_term(frame, False, False), oracle_term(frame, True, False)
        differ = int((off.view(np.uint32) != on.view(np.uint32)).any(axis=-1).sum())
        assert differ >= least, (frame, differ)


def distinct_colours(frame):
    return len(np.unique(np.ascontiguousarray(frame).view(np.uint32).reshape(-1, 3), axis=0))


def nonzero_share(term, hits):
    """the share of the live records whose term has a nonzero channel"""
    live = ao_ref.live_records(hits).reshape(np.shape(hits))
    return float((term[live] != 0).any(axis=-1).mean())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def handmade_records(count=130):
    """a batch of made-up records: misses, a light, an inside hit, |N.x| on both sides of 0.5 (both choices of the tangent
    frame's axis), an object the scene does not have -- unit normals, finite points"""
    rng = np.random.RandomState(41)
    hits = np.zeros(count, dtype=query_ref.HIT_DTYPE)
    N = rng.normal(size=(count, 3)).astype(np.float64)
    N /= np.linalg.norm(N, axis=1)[:, None]
    N[3] = (0.49999997, 0.0, np.sqrt(1 - 0.49999997 ** 2))           # either side of the 0.5 that picks the axis
    N[4] = (0.5, 0.0, np.sqrt(0.75))
    N[5] = (-0.50000006, np.sqrt(1 - 0.50000006 ** 2), 0.0)
    N[6], N[7], N[8] = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0)
    hits["object"] = rng.randint(0, 12, count)
    hits["distance"] = rng.uniform(1, 30, count).astype(F)
    hits["point"] = rng.uniform(-6, 12, (count, 3)).astype(F)
    hits["normal"] = N.astype(F)
    hits["color"] = rng.uniform(0, 1, (count, 3)).astype(F)
    hits["object"][[0, 17, 64, 129]] = -1                            # misses, the first and the last record among them
    hits["flags"][9] = HIT_LIGHT
    hits["flags"][10] = ao_ref.HIT_INSIDE
    hits["flags"][11] = ao_ref.HIT_INSIDE | HIT_LIGHT
    hits["object"][12] = 1 << 20                                     # no such object: kd is 0
    assert (np.abs(hits["normal"][:, 0]) < F(0.5)).sum() > 20 and (np.abs(hits["normal"][:, 0]) >= F(0.5)).sum() > 20
    return hits
