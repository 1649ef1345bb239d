"""The reference of include/rt_capi_soft.h, for the tests: refract_ref's batch calculatePixel (an fp32 numpy restatement of
oracle/rt_oracle.c, calculate_pixel, with the refraction header's transmission term) whose lights listed as area lights are
sampled by the header's definition -- n x n stratified samples on a disc facing the shading point, every sample segment's
verdict query_ref's occlusion, the hash in numpy uint32 arithmetic.  With no area light, render() is refract_ref's frame bit for
bit (test_soft_cpu.py), and so the oracle's.

A scene is Scene(oracle scene, area={light index: (n, r)}, seed=0, refractive=..., images=...) (refractive and images as
refract_ref.Scene); cam is an RtCameraDesc or an OrcCamera.  Every ray carries its sampling key: x * H + z of the (virtual)
launch for a camera frame, the ray index for a batch."""
import numpy as np

import query_ref
import refract_ref
from rays_ref import camera_rays

F = np.float32
U32 = np.uint32
GOLDEN = U32(0x9E3779B9)


class Scene(refract_ref.Scene):
    def __init__(self, oscene, area=None, seed=0, refractive=None, images=None):
        super().__init__(oscene, refractive, images)
        self.area = {k: (int(n), F(r)) for k, (n, r) in (area or {}).items() if F(r) != F(0)}
        self.seed = U32(seed & 0xFFFFFFFF)


def H(x):
    """lowbias32 over uint32 arrays (or scalars)"""
    x = np.asarray(x, dtype=U32)
    with np.errstate(over="ignore"):
        x = x ^ (x >> U32(16))
        x = (x * U32(0x7FEB352D)).astype(U32)
        x = x ^ (x >> U32(15))
        x = (x * U32(0x846CA68B)).astype(U32)
        x = x ^ (x >> U32(16))
    return x


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def disc_samples(seed, P, key, level, ordinal, C, n, r):
    """the header's n x n sample points on the disc of the light of ordinal `ordinal` (centre C, radius r) facing the shading
    points P (n_pts, 3) with keys key (uint32), at ray-tree level `level`, the scene's seed `seed` -> float32 (n_pts, 3) for each
    sample i * n + j, in that order"""
    _normalize = refract_ref._normalize
    with np.errstate(all="ignore"):
        L = _normalize(C[None, :] - P)
        A = np.where((np.abs(L[:, 0]) < F(0.5))[:, None], np.array([1, 0, 0], dtype=F), np.array([0, 1, 0], dtype=F))
        U = _normalize(_cross(A, L))
        V = _cross(L, U)
        h = H(H(H(H(U32(seed) ^ GOLDEN) ^ key) ^ U32(level)) ^ U32(ordinal))
        step = F(2.0) / F(n)
        for i in range(n):
            for j in range(n):
                hs = H(h ^ U32(i * n + j))
                xi1 = (hs >> U32(8)).astype(F) * F(2.0 ** -24)
                xi2 = (H(hs ^ GOLDEN) >> U32(8)).astype(F) * F(2.0 ** -24)
                a = (F(i) + xi1) * step - F(1.0)
                b = (F(j) + xi2) * step - F(1.0)
                dx = a * np.sqrt(F(1.0) - (b * b) * F(0.5))
                dy = b * np.sqrt(F(1.0) - (a * a) * F(0.5))
                yield C[None, :] + (U * (r * dx)[:, None] + V * (r * dy)[:, None])


def visible_fraction(scene, P, key, level, ordinal, C, n, r):
    """the header's (m, f) for the shading points P (n_pts, 3) with keys key (uint32), at ray-tree level `level`, towards the
    light of ordinal `ordinal` with centre C, n x n samples, radius r"""
    m = np.zeros(P.shape[0], dtype=np.int64)
    for Q in disc_samples(scene.seed, P, key, level, ordinal, C, n, r):
        m += ~query_ref.occluded(scene, np.concatenate([P, Q], axis=1))
    return m, (m.astype(F) / F(n * n))


def _pixel(scene, E, d, key, level, depth):
    """calculate_pixel(Ray(E, d), level) of every ray of the batch, keys key -> (n, 3)"""
    n = E.shape[0]
    out = np.full((n, 3), refract_ref.NULL, dtype=F)
    if level > depth or n == 0:
        return out
    idx, t, P, N, oc = refract_ref._nearest(scene, E, d)
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
    Es, ds, ts, Ps, Ns, ocs, ids, keys = E[s], d[s], t[s], P[s], N[s], oc[s], idx[s], key[s]
    obj = scene.objects
    diffuse = np.array([obj[k].diffuse for k in ids], dtype=F)
    specular = np.array([obj[k].specular for k in ids], dtype=F)
    rf = np.array([obj[k].reflective for k in ids], dtype=F)
    final = np.zeros((len(s), 3), dtype=F)
    _normalize = refract_ref._normalize
    _dot = refract_ref._dot
    with np.errstate(all="ignore"):
        normal_dir = _normalize(Ns)                              # the CollisionObject ctor: Ray(point, normal)
        for ordinal, k in enumerate(lights):
            light = obj[k]
            lo, lc, li = refract_ref._v(light.origin), refract_ref._v(light.color), F(light.intensity)
            if k in scene.area:
                sn, sr = scene.area[k]
                m, f = visible_fraction(scene, Ps, keys, level, ordinal, lo, sn, sr)
                lit = m > 0
            else:
                segs = np.concatenate([Ps, np.broadcast_to(lo, Ps.shape)], axis=1)
                lit = ~query_ref.occluded(scene, segs)
                f = None
            light_ray = _normalize(lo[None, :] - Ps)
            # cosine_shade
            cos = _dot(normal_dir, light_ray)
            add = lit & (diffuse > F(0)) & (cos > F(0))
            factor = (cos * diffuse) * li
            if f is not None:
                factor = factor * f
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
            if f is not None:
                spec = spec * f
            final = np.where((lit & (dot > F(0)))[:, None], final + lc[None, :] * spec[:, None], final)
        # reflection, first
        r = np.nonzero(rf > F(0))[0]
        if len(r):
            ndot = _dot(Ns[r], ds[r])
            refl = (F(-2) * Ns[r]) * ndot[:, None] + ds[r]
            child = _pixel(scene, Ps[r], _normalize(refl), keys[r], level + 1, depth)
            final[r] = final[r] + (child * rf[r][:, None]) * ocs[r]
        # transmission, second
        for k, (tf, ior) in scene.refractive.items():
            if not tf > 0:
                continue
            sel = np.nonzero(ids == k)[0]
            if len(sel) == 0:
                continue
            ok, co, cd = refract_ref.transmitted(obj[k], Es[sel], ds[sel], ts[sel], Ps[sel], Ns[sel], ior)
            sel, co, cd = sel[ok], co[ok], cd[ok]
            if len(sel) == 0:
                continue
            child = _pixel(scene, co, cd, keys[sel], level + 1, depth)
            final[sel] = final[sel] + (child * F(tf)) * ocs[sel]
    out[s] = final
    return out


def trace(scene, rays, depth, keys=None):
    """calculate_pixel(Ray(E, normalize(T - E)), 0) of every ray of float32 (..., 6) -> float32 (..., 3); keys: the rays'
    sampling keys (default: the ray index, as rt_trace_rays)"""
    flat = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    key = np.arange(flat.shape[0], dtype=np.uint64).astype(U32) if keys is None else np.asarray(keys, dtype=U32).reshape(-1)
    out = _pixel(scene, flat[:, :3].copy(), query_ref.directions(flat), key, 0, depth)
    return out.reshape(np.shape(rays)[:-1] + (3,))


def render(scene, cam, W, H, depth, x0=0, x1=None):
    """the (x1 - x0, H, 3) strip rt_render computes, pixels[x][z]; key x * H + z"""
    x1 = W if x1 is None else x1
    keys = (np.arange(x0, x1, dtype=np.uint64)[:, None] * np.uint64(H) + np.arange(H, dtype=np.uint64)[None, :])
    return trace(scene, camera_rays(cam, W, H)[x0:x1], depth, (keys & np.uint64(0xFFFFFFFF)).astype(U32))


def render_ssaa(scene, cam, W, H, depth, k):
    """rt_render_ssaa's frame: the virtual kW x kH frame (keys over it), box-filtered in the kernel's order"""
    v = render(scene, cam, k * W, k * H, depth).reshape(W, k, H, k, 3)
    acc = v[:, 0, :, 0]
    for s in range(1, k * k):
        i, j = divmod(s, k)
        acc = acc + v[:, i, :, j]
    return (acc / F(k * k)).astype(F)
