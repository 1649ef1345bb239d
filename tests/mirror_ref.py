"""The reference of include/rt_mirror.h, for the tests: the header's definition restated in numpy float32 on top of
query_ref.intersect / directions, vectorised over the rays still alive and looped over the bounces; one rounding per operation
(numpy's float32 ufuncs do not contract), in the header's order."""
import contextlib

import numpy as np

import query_ref
from query_ref import HIT_DTYPE

F = np.float32
RT_HIT_LIGHT = 2
MAX_BOUNCES = 64


def lowbias32(x):
    """rt_capi_ao.h's hash, on uint32 arrays"""
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def reflective(scene):
    """rf[o] of a query_ref.Scene"""
    return np.array([o.reflective for o in scene.objects], dtype=F)


@contextlib.contextmanager
def _directions_given(table):
    """query_ref.intersect with the directions table["d"] (one row per ray of its next call; None: its own) in place of
    normalize(T - E): for the measurement of the header's stated deviation only"""
    own = query_ref.directions
    query_ref.directions = lambda rays: table["d"] if table["d"] is not None and len(table["d"]) == len(rays) else own(rays)
    try:
        yield
    finally:
        query_ref.directions = own


def records(scene, rays, max_bounces, min_reflective=1.0, details=False, follow_r=False):
    """rt_mirror_records of float32 rays (..., 6) -> (hits, guide HIT_DTYPE (...), weight float32 (..., 3), path uint32 (...));
    with details also a dict: "chain", int (..., max_bounces), the objects followed in order (-1 beyond k), "k", "cut", "tag",
    "L".  follow_r: NOT the header -- ray k + 1 is traced along normalize(r), as calculatePixel's Ray(P, r) is, and not along
    normalize((P + r) - P): what the header's deviation is measured against."""
    assert 0 <= max_bounces <= MAX_BOUNCES
    flat = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    n = flat.shape[0]
    rf = reflective(scene)
    cur = flat.copy()
    with np.errstate(all="ignore"):
        d0 = query_ref.directions(flat)
    d = d0.copy()
    w = np.ones((n, 3), dtype=F)
    L = np.zeros(n, dtype=F)
    A = np.tile(np.eye(3, dtype=F), (n, 1, 1))
    tag = np.zeros(n, dtype=np.uint32)
    k = np.zeros(n, dtype=np.uint32)
    cut = np.zeros(n, dtype=bool)
    alive = np.ones(n, dtype=bool)
    term = np.zeros(n, dtype=HIT_DTYPE)
    chain = np.full((n, max_bounces), -1, dtype=np.int32)
    given = dict(d=None)
    with np.errstate(all="ignore"), _directions_given(given):
        for s in range(max_bounces + 1):
            idx = np.nonzero(alive)[0]
            if not idx.size:
                break
            assert not follow_r or idx.size <= query_ref.CHUNK      # (intersect asks for the directions once per chunk)
            h = query_ref.intersect(scene, cur[idx])
            found = h["object"] >= 0
            L[idx] = np.where(found, L[idx] + h["distance"], L[idx])
            obj = np.clip(h["object"], 0, None)
            mirror = found & ((h["flags"] & RT_HIT_LIGHT) == 0) & (rf[obj] >= F(min_reflective)) if len(rf) else found & False
            stop = ~mirror | (s == max_bounces)
            term[idx[stop]] = h[stop]
            cut[idx[stop]] = mirror[stop]
            alive[idx[stop]] = False
            gi, hg = idx[~stop], h[~stop]
            if not gi.size:
                continue
            nrm, P, dd = hg["normal"], hg["point"], d[gi]
            c = _dot(nrm, dd)
            r = ((F(-2.0) * nrm) * c[:, None]) + dd
            cur[gi, :3] = P
            cur[gi, 3:] = P + r
            if follow_r:
                d[gi] = query_ref._normalize(r)[0]
                given["d"] = d[gi]
            else:
                d[gi] = query_ref.directions(cur[gi])
            w[gi] = w[gi] * (rf[hg["object"]][:, None] * hg["color"])
            Ag = A[gi]
            an = (Ag[:, :, 0] * nrm[:, None, 0] + Ag[:, :, 1] * nrm[:, None, 1]) + Ag[:, :, 2] * nrm[:, None, 2]
            A[gi] = Ag - (F(2.0) * an)[:, :, None] * nrm[:, None, :]
            tag[gi] = np.uint32(1) + lowbias32((tag[gi] << np.uint32(12)) | hg["object"].astype(np.uint32)) % np.uint32(0x7fffe)
            chain[gi, s] = hg["object"]
            k[gi] += np.uint32(1)
        assert not alive.any()
        guide = term.copy()
        m = (term["object"] >= 0) & (k > 0)
        guide["object"][m] = ((tag[m] << np.uint32(12)) | term["object"][m].astype(np.uint32)).view(np.int32)
        guide["distance"][m] = L[m]
        guide["point"][m] = flat[m, :3] + d0[m] * L[m, None]
        tn = term["normal"][m]
        Am = A[m]
        guide["normal"][m] = (Am[:, :, 0] * tn[:, None, 0] + Am[:, :, 1] * tn[:, None, 1]) + Am[:, :, 2] * tn[:, None, 2]
    path = k | (cut.astype(np.uint32) << np.uint32(8)) | (tag << np.uint32(12))
    shape = np.shape(rays)[:-1]
    out = (term.reshape(shape), guide.reshape(shape), w.reshape(shape + (3,)), path.reshape(shape))
    if details:
        out += (dict(chain=chain.reshape(shape + (max_bounces,)), k=k.reshape(shape).astype(np.int64), cut=cut.reshape(shape),
                     tag=tag.reshape(shape), L=L.reshape(shape)),)
    return out


def unpack(path):
    """out_path -> (k, cut, tag)"""
    path = np.asarray(path, dtype=np.uint32)
    return (path & np.uint32(0xff)).astype(np.int64), ((path >> np.uint32(8)) & np.uint32(1)).astype(bool), path >> np.uint32(12)


__all__ = ["records", "unpack", "reflective", "lowbias32", "HIT_DTYPE", "MAX_BOUNCES"]
