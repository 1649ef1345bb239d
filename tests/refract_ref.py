"""The reference of include/rt_capi_refract.h, for the tests: an fp32 numpy restatement of calculatePixel (oracle/rt_oracle.c,
calculate_pixel) with the header's transmission term, as a tree over ray batches -- every level's rays of one batch traced
together, the reflected and the transmitted children of a batch as two batches of the next level.  The nearest hit and the
shadow verdicts are query_ref's (pinned to the oracle); with no refractive object, render() is the oracle's frame bit for bit
(test_refract_cpu.py), which ties the shading here to the oracle as well.

A scene is Scene(oracle scene, refractive={index: (tf, ior)}, images={plane index: texture_ref image}); cam is an
RtCameraDesc or an OrcCamera."""
import numpy as np

import query_ref
import texture_ref
from rays_ref import camera_rays

F = np.float32
SPHERE = query_ref.SPHERE
NULL = F(0.75)                                   # NULL_COLOR, src/RayTracer.h:52


class Scene:
    def __init__(self, oscene, refractive=None, images=None):
        q = query_ref.Scene(oscene)
        self.objects = q.objects
        self.shadow_range = q.shadow_range
        self.refractive = dict(refractive or {})
        self.images = dict(images or {})


_v, _dot = query_ref._v, query_ref._dot


def _normalize(v):
    return query_ref._normalize(v)[0]


def _nearest(scene, E, d):
    """get_collision over rays (E, d): Scene index (-1: miss), distance, point, raw normal (before the CollisionObject ctor's
    normalisation), colour"""
    n = E.shape[0]
    best = np.full(n, F(65535.0), dtype=F)
    idx = np.full(n, -1, dtype=np.int64)
    P = np.zeros((n, 3), dtype=F)
    N = np.zeros((n, 3), dtype=F)
    col = np.zeros((n, 3), dtype=F)
    with np.errstate(all="ignore"):
        for i, o in enumerate(scene.objects):
            hit, dist, Pi, Ni, ci, _ = query_ref._collision(o, E, d, True)
            take = hit & (dist < best)
            if not take.any():
                continue
            if i in scene.images and o.kind != SPHERE:
                ip = d * dist[:, None] + E
                anchor = _v(o.origin if o.kind == query_ref.INFINITE_PLANE else o.plane_origin)
                PO = ip - anchor[None, :]
                x, y = _dot(PO, _v(o.horizontal)), _dot(PO, _v(o.vertical))
                ci = np.array(ci, dtype=F, copy=True)
                ci[take] = texture_ref.colour(x[take], y[take], scene.images[i])
            best = np.where(take, dist, best)
            idx[take] = i
            P[take], N[take], col[take] = Pi[take], Ni[take], ci[take]
    return idx, best, P, N, col


def transmitted(o, E, d, t, P, N, ior):
    """the header's transmitted child of hits on object o: (exists, origin, direction); t, P, N the records' distance, point
    and raw normal, ior the sphere interior's"""
    with np.errstate(all="ignore"):
        if o.kind == SPHERE:
            c = _v(o.origin)[None, :]
            Q = P - c
            ior = F(ior)
            eta = F(1.0) / ior
            c1 = -_dot(N, d)
            k1 = F(1) - (eta * eta) * (F(1) - c1 * c1)
            T1 = _normalize(d * eta + N * (eta * c1 - np.sqrt(k1))[:, None])
            s = F(-2.0) * _dot(T1, Q)
            P2 = P + T1 * s[:, None]
            N2 = _normalize(P2 - c)
            c2 = _dot(N2, T1)
            k2 = F(1) - (ior * ior) * (F(1) - c2 * c2)
            T2 = T1 * ior - N2 * (ior * c2 - np.sqrt(k2))[:, None]
            ok = (t >= F(0)) & ~(k1 < F(0)) & (s > F(0)) & ~(k2 < F(0))
            return ok, P2 + N2 * F(1e-3), _normalize(T2)
        normal = _v(o.normal)
        towards = (_dot(np.broadcast_to(normal, d.shape), d) < F(0))[:, None]
        other = np.where(towards, _v(o.reverse_normal)[None, :], normal[None, :])
        ip = d * t[:, None] + E
        return np.ones(len(t), dtype=bool), ip + other * F(1e-3), d.copy()


def _pixel(scene, E, d, level, depth):
    """calculate_pixel(Ray(E, d), level) of every ray of the batch -> (n, 3)"""
    n = E.shape[0]
    out = np.full((n, 3), NULL, dtype=F)
    if level > depth or n == 0:
        return out
    idx, t, P, N, oc = _nearest(scene, E, d)
    found = idx >= 0
    lights = [k for k, o in enumerate(scene.objects) if o.is_light]
    is_light = np.zeros(n, dtype=bool)
    for k in lights:
        sel = idx == k
        is_light |= sel
        out[sel] = oc[sel] * F(scene.objects[k].intensity)
    shade = found & ~is_light
    s = np.nonzero(shade)[0]
    if len(s) == 0:
        return out
    Es, ds, ts, Ps, Ns, ocs, ids = E[s], d[s], t[s], P[s], N[s], oc[s], idx[s]
    obj = scene.objects
    diffuse = np.array([obj[k].diffuse for k in ids], dtype=F)
    specular = np.array([obj[k].specular for k in ids], dtype=F)
    rf = np.array([obj[k].reflective for k in ids], dtype=F)
    final = np.zeros((len(s), 3), dtype=F)
    with np.errstate(all="ignore"):
        normal_dir = _normalize(Ns)                              # the CollisionObject ctor: Ray(point, normal)
        for k in lights:
            light = obj[k]
            lo, lc, li = _v(light.origin), _v(light.color), F(light.intensity)
            segs = np.concatenate([Ps, np.broadcast_to(lo, Ps.shape)], axis=1)
            lit = ~query_ref.occluded(scene, segs)
            light_ray = _normalize(lo[None, :] - Ps)
            # cosine_shade
            cos = _dot(normal_dir, light_ray)
            add = lit & (diffuse > F(0)) & (cos > F(0))
            factor = (cos * diffuse) * li
            inc = final + (factor[:, None] * ocs) * lc[None, :]
            final = np.where(add[:, None], inc, final)
            clamp = lit & (diffuse > F(0))
            final = np.where(clamp[:, None], np.where(final > F(1), F(1), final), final)
            # specular
            N3 = _normalize(normal_dir)
            R = light_ray - N3 * (F(2.0) * _dot(light_ray, N3))[:, None]
            dot = _dot(ds, R)
            p = dot.copy()
            for _ in range(19):
                p = p * dot
            spec = p * specular
            final = np.where((lit & (dot > F(0)))[:, None], final + lc[None, :] * spec[:, None], final)
        # reflection, first
        r = np.nonzero(rf > F(0))[0]
        if len(r):
            ndot = _dot(Ns[r], ds[r])
            refl = (F(-2) * Ns[r]) * ndot[:, None] + ds[r]
            child = _pixel(scene, Ps[r], _normalize(refl), level + 1, depth)
            final[r] = final[r] + (child * rf[r][:, None]) * ocs[r]
        # transmission, second
        for k, (tf, ior) in scene.refractive.items():
            if not tf > 0:
                continue
            sel = np.nonzero(ids == k)[0]
            if len(sel) == 0:
                continue
            ok, co, cd = transmitted(obj[k], Es[sel], ds[sel], ts[sel], Ps[sel], Ns[sel], ior)
            sel, co, cd = sel[ok], co[ok], cd[ok]
            if len(sel) == 0:
                continue
            child = _pixel(scene, co, cd, level + 1, depth)
            final[sel] = final[sel] + (child * F(tf)) * ocs[sel]
    out[s] = final
    return out


def trace(scene, rays, depth):
    """calculate_pixel(Ray(E, normalize(T - E)), 0) of every ray of float32 (..., 6) -> float32 (..., 3)"""
    flat = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    out = _pixel(scene, flat[:, :3].copy(), query_ref.directions(flat), 0, depth)
    return out.reshape(np.shape(rays)[:-1] + (3,))


def render(scene, cam, W, H, depth, x0=0, x1=None):
    """the (x1 - x0, H, 3) strip rt_render computes, pixels[x][z]"""
    x1 = W if x1 is None else x1
    return trace(scene, camera_rays(cam, W, H)[x0:x1], depth)
