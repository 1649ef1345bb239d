"""The reference of include/rt_glass.h, for the tests: the header's definition restated in numpy float32.  It is
mirror_ref.records with the header's one more way to go on: the transmitted child of a candidate is refract_ref.transmitted's
(the restatement of rt_capi_refract.h the render kernels are held to), given N = normalize(P - centre) for a sphere -- the
record's own normal has been normalised a second time.  One rounding per operation (numpy's float32 ufuncs do not contract), in
the header's order.  A scene is a refract_ref.Scene: query_ref's objects and refractive = {index: (tf, ior)}."""
import numpy as np

import query_ref
import refract_ref
from mirror_ref import MAX_BOUNCES, RT_HIT_LIGHT, _directions_given, _dot, lowbias32, reflective
from query_ref import HIT_DTYPE

F = np.float32
INF = float("inf")


def transmissive(scene):
    """(tf[o], ior[o]) of a refract_ref.Scene (tf 0 where the object has no rt_refraction_desc)"""
    tf = np.zeros(len(scene.objects), dtype=F)
    ior = np.ones(len(scene.objects), dtype=F)
    for o, (t, i) in getattr(scene, "refractive", {}).items():
        tf[o], ior[o] = t, i
    return tf, ior


def child(scene, h, E, d, ior):
    """the header's step 5 for the records h of rays (E, d), all candidates -> (exists, O, D, s); s is 0 for a pane"""
    n = len(h)
    exists = np.zeros(n, dtype=bool)
    O, D, s = np.zeros((n, 3), dtype=F), np.zeros((n, 3), dtype=F), np.zeros(n, dtype=F)
    with np.errstate(all="ignore"):
        for o in np.unique(h["object"]):
            sel = np.nonzero(h["object"] == o)[0]
            ob = scene.objects[o]
            P, t = h["point"][sel], h["distance"][sel]
            N = None
            if ob.kind == query_ref.SPHERE:
                Q = P - query_ref._v(ob.origin)[None, :]
                N = query_ref._normalize(Q)[0]
            ok, co, cd = refract_ref.transmitted(ob, E[sel], d[sel], t, P, N, ior[o])
            exists[sel], O[sel], D[sel] = ok, co, cd
            if ob.kind == query_ref.SPHERE:                                   # the chord, as transmitted() computes it
                eta = F(1.0) / F(ior[o])
                c1 = -_dot(N, d[sel])
                k1 = F(1) - (eta * eta) * (F(1) - c1 * c1)
                T1 = query_ref._normalize(d[sel] * eta + N * (eta * c1 - np.sqrt(k1))[:, None])[0]
                s[sel] = F(-2.0) * _dot(T1, Q)
    return exists, O, D, s


def records(scene, rays, max_bounces, min_reflective=1.0, min_transmissive=0.5, details=False, follow_d=False):
    """rt_glass_records of float32 rays (..., 6) -> (hits, guide HIT_DTYPE (...), weight float32 (..., 3), path uint32 (...));
    with details also a dict: "chain", int (..., max_bounces), the objects followed in order (-1 beyond k), "glass", bool of the
    same shape: followed as glass, "k", "cut", "g", "tag", "L", "first" (the origin of the first transmitted child of a ray's
    first candidate, NaN where it has none) and "childless" (candidates met whose child did not exist).  follow_d: NOT the
    header -- a transmitted child is traced along D itself, as calculatePixel's Ray(O, D) is, and not along
    normalize((O + D) - O): what the header's deviation is measured against."""
    assert 0 <= max_bounces <= MAX_BOUNCES
    flat = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    n = flat.shape[0]
    rf = reflective(scene)
    tf, ior = transmissive(scene)
    cur = flat.copy()
    with np.errstate(all="ignore"):
        d0 = query_ref.directions(flat)
    d = d0.copy()
    w = np.ones((n, 3), dtype=F)
    L = np.zeros(n, dtype=F)
    A = np.tile(np.eye(3, dtype=F), (n, 1, 1))
    tag = np.zeros(n, dtype=np.uint32)
    k = np.zeros(n, dtype=np.uint32)
    g = np.zeros(n, dtype=bool)
    cut = np.zeros(n, dtype=bool)
    alive = np.ones(n, dtype=bool)
    term = np.zeros(n, dtype=HIT_DTYPE)
    chain = np.full((n, max_bounces), -1, dtype=np.int32)
    glass = np.zeros((n, max_bounces), dtype=bool)
    first = np.full((n, 3), np.nan, dtype=F)
    seen_candidate = np.zeros(n, dtype=bool)
    childless = np.zeros(n, dtype=np.int32)
    given = dict(d=None)
    with np.errstate(all="ignore"), _directions_given(given):
        for s in range(max_bounces + 1):
            idx = np.nonzero(alive)[0]
            if not idx.size:
                break
            assert not follow_d or idx.size <= query_ref.CHUNK        # (intersect asks for the directions once per chunk)
            h = query_ref.intersect(scene, cur[idx])
            found = h["object"] >= 0
            L[idx] = np.where(found, L[idx] + h["distance"], L[idx])
            obj = np.clip(h["object"], 0, None)
            eligible = found & ((h["flags"] & RT_HIT_LIGHT) == 0)
            if not len(rf):
                eligible = eligible & False
                obj = np.zeros_like(obj)
            otf = tf[obj] if len(tf) else np.zeros(len(obj), dtype=F)
            candidate = eligible & (otf > F(0)) & (otf >= F(min_transmissive))
            through = np.zeros(len(idx), dtype=bool)
            O, D, chord = np.zeros((len(idx), 3), dtype=F), np.zeros((len(idx), 3), dtype=F), np.zeros(len(idx), dtype=F)
            c = np.nonzero(candidate)[0]
            if c.size:
                exists, O[c], D[c], chord[c] = child(scene, h[c], cur[idx[c], :3], d[idx[c]], ior)
                through[c] = exists
                fresh = c[~seen_candidate[idx[c]] & exists]
                first[idx[fresh]] = O[fresh]
                seen_candidate[idx[c]] = True
                childless[idx[c[~exists]]] += 1
            mirror = eligible & (rf[obj] >= F(min_reflective)) if len(rf) else eligible
            follow = through | mirror
            stop = ~follow | (s == max_bounces)
            term[idx[stop]] = h[stop]
            cut[idx[stop]] = follow[stop]
            alive[idx[stop]] = False
            # step 10: through glass
            sel = ~stop & through
            gi, hg = idx[sel], h[sel]
            if gi.size:
                cur[gi, :3] = O[sel]
                cur[gi, 3:] = O[sel] + D[sel]
                d[gi] = D[sel] if follow_d else query_ref.directions(cur[gi])
                w[gi] = w[gi] * (tf[hg["object"]][:, None] * hg["color"])
                kinds = np.array([scene.objects[o].kind for o in hg["object"]])
                L[gi] = np.where(kinds == query_ref.SPHERE, L[gi] + chord[sel], L[gi])
                tag[gi] = np.uint32(1) + lowbias32((tag[gi] << np.uint32(12)) | hg["object"].astype(np.uint32)
                                                   | np.uint32(0x80000000)) % np.uint32(0x7fffe)
                chain[gi, s] = hg["object"]
                glass[gi, s] = True
                g[gi] = True
                k[gi] += np.uint32(1)
            # step 11: rt_mirror.h's mirror step (mirror_ref.records')
            sel = ~stop & ~through
            gi, hg = idx[sel], h[sel]
            if gi.size:
                nrm, P, dd = hg["normal"], hg["point"], d[gi]
                cc = _dot(nrm, dd)
                r = ((F(-2.0) * nrm) * cc[:, None]) + dd
                cur[gi, :3] = P
                cur[gi, 3:] = P + r
                d[gi] = query_ref.directions(cur[gi])
                w[gi] = w[gi] * (rf[hg["object"]][:, None] * hg["color"])
                Ag = A[gi]
                an = (Ag[:, :, 0] * nrm[:, None, 0] + Ag[:, :, 1] * nrm[:, None, 1]) + Ag[:, :, 2] * nrm[:, None, 2]
                A[gi] = Ag - (F(2.0) * an)[:, :, None] * nrm[:, None, :]
                tag[gi] = np.uint32(1) + lowbias32((tag[gi] << np.uint32(12)) | hg["object"].astype(np.uint32)) % np.uint32(0x7fffe)
                chain[gi, s] = hg["object"]
                k[gi] += np.uint32(1)
            if follow_d:
                given["d"] = d[np.nonzero(alive)[0]]
        assert not alive.any()
        guide = term.copy()
        m = (term["object"] >= 0) & (k > 0)
        guide["object"][m] = ((tag[m] << np.uint32(12)) | term["object"][m].astype(np.uint32)).view(np.int32)
        guide["distance"][m] = L[m]
        guide["point"][m] = flat[m, :3] + d0[m] * L[m, None]
        tn = term["normal"][m]
        Am = A[m]
        guide["normal"][m] = (Am[:, :, 0] * tn[:, None, 0] + Am[:, :, 1] * tn[:, None, 1]) + Am[:, :, 2] * tn[:, None, 2]
    path = k | (cut.astype(np.uint32) << np.uint32(8)) | (g.astype(np.uint32) << np.uint32(10)) | (tag << np.uint32(12))
    shape = np.shape(rays)[:-1]
    out = (term.reshape(shape), guide.reshape(shape), w.reshape(shape + (3,)), path.reshape(shape))
    if details:
        out += (dict(chain=chain.reshape(shape + (max_bounces,)), glass=glass.reshape(shape + (max_bounces,)),
                     k=k.reshape(shape).astype(np.int64), cut=cut.reshape(shape), g=g.reshape(shape), tag=tag.reshape(shape),
                     L=L.reshape(shape), first=first.reshape(shape + (3,)), childless=childless.reshape(shape)),)
    return out


def unpack(path):
    """out_path -> (k, cut, g, tag)"""
    path = np.asarray(path, dtype=np.uint32)
    return ((path & np.uint32(0xff)).astype(np.int64), ((path >> np.uint32(8)) & np.uint32(1)).astype(bool),
            ((path >> np.uint32(10)) & np.uint32(1)).astype(bool), path >> np.uint32(12))


__all__ = ["records", "unpack", "transmissive", "child", "HIT_DTYPE", "MAX_BOUNCES", "INF"]
