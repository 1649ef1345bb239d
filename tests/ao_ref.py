"""The reference of include/rt_capi_ao.h, for the tests: the header's definition restated in fp32 numpy -- one rounding per
operation, the hash in uint32 arithmetic (soft_ref.H), every sample's verdict query_ref's occlusion of its segment."""
import numpy as np

import query_ref
from soft_ref import GOLDEN, H

F = np.float32
U32 = np.uint32
HIT_INSIDE, HIT_LIGHT = 1, 2


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def live_records(hits):
    """the records that sample at all: neither a miss nor a light"""
    flat = np.ascontiguousarray(hits).reshape(-1)
    return (flat["object"] >= 0) & ((flat["flags"] & HIT_LIGHT) == 0)


def frames(hits):
    """(P, N, U, V) of every record, float32 (n, 3) each: the point, the normal (negated for an inside hit) and the header's
    tangent frame"""
    flat = np.ascontiguousarray(hits).reshape(-1)
    P = flat["point"].astype(F)
    N = flat["normal"].astype(F)
    N = np.where(((flat["flags"] & HIT_INSIDE) != 0)[:, None], -N, N)
    with np.errstate(all="ignore"):
        A = np.where((np.abs(N[:, 0]) < F(0.5))[:, None], np.array([1, 0, 0], dtype=F), np.array([0, 1, 0], dtype=F))
        U = query_ref._normalize(_cross(A, N))[0]
        V = _cross(N, U)
    return P, N, U, V


def disc_points(n_records, samples, seed, key0):
    """the header's (a, b, dx, dy, dz) of every record and sample: float32 (n_records, samples^2) each, sample s = i * samples + j"""
    n = int(samples)
    key = ((np.arange(n_records, dtype=np.uint64) + np.uint64(int(key0) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)).astype(U32)
    g = H(H(U32(int(seed) & 0xFFFFFFFF) ^ GOLDEN) ^ key)
    step = F(2.0) / F(n)
    out = [np.empty((n_records, n * n), dtype=F) for _ in range(5)]
    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(n):
                s = i * n + j
                hs = H(g ^ U32(s))
                xi1 = (hs >> U32(8)).astype(F) * F(2.0 ** -24)
                xi2 = (H(hs ^ GOLDEN) >> U32(8)).astype(F) * F(2.0 ** -24)
                a = (F(i) + xi1) * step - F(1.0)
                b = (F(j) + xi2) * step - F(1.0)
                dx = a * np.sqrt(F(1.0) - (b * b) * F(0.5))
                dy = b * np.sqrt(F(1.0) - (a * a) * F(0.5))
                w = (F(1.0) - dx * dx) - dy * dy
                dz = np.where(w > F(0), np.sqrt(np.where(w > F(0), w, F(0))), F(0)).astype(F)
                for o, v in zip(out, (a, b, dx, dy, dz)):
                    o[:, s] = v
    return out


def directions(hits, samples, seed=0, key0=0):
    """D of every record and sample: float32 (n_records, samples^2, 3)"""
    _, N, U, V = frames(hits)
    _, _, dx, dy, dz = disc_points(len(N), samples, seed, key0)
    with np.errstate(all="ignore"):
        return (U[:, None, :] * dx[:, :, None] + V[:, None, :] * dy[:, :, None]) + N[:, None, :] * dz[:, :, None]


def segments(hits, samples, radius, seed=0, key0=0):
    """the segments {P, Q} of every record and sample: float32 (n_records, samples^2, 6), sample s = i * samples + j, and the
    mask of the live records (the others' segments are {0, 0}: they are never asked)"""
    P = frames(hits)[0]
    D = directions(hits, samples, seed, key0)
    with np.errstate(all="ignore"):
        Q = P[:, None, :] + D * F(radius)
    live = live_records(hits)
    segs = np.concatenate([np.broadcast_to(P[:, None, :], Q.shape), Q], axis=2).astype(F)
    segs[~live] = F(0)
    return np.ascontiguousarray(segs), live


def from_verdicts(blocked, live, samples):
    """ao of every record from its segments' verdicts blocked (n_records, samples^2): open / samples^2, 1 where not live"""
    n = int(samples)
    open_ = (~np.asarray(blocked, dtype=bool)).sum(axis=1)
    return np.where(live, open_.astype(F) / F(n * n), F(1.0)).astype(F)


def ambient_occlusion(scene, hits, samples, radius, seed=0, key0=0, channels=1):
    """rt_ambient_occlusion of the records hits (any shape) on scene (a query_ref.Scene) -> float32 of hits' shape, or with
    channels = 3 of that shape + (3,)"""
    segs, live = segments(hits, samples, radius, seed, key0)
    blocked = np.zeros(segs.shape[:2], dtype=bool)
    blocked[live] = query_ref.occluded(scene, segs[live])
    ao = from_verdicts(blocked, live, samples).reshape(np.shape(hits))
    return np.repeat(ao[..., None], 3, axis=-1) if channels == 3 else ao


__all__ = ["segments", "ambient_occlusion", "directions", "disc_points", "frames", "live_records", "from_verdicts"]
