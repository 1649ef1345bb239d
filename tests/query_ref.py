"""The reference of include/rt_capi_query.h, for the tests: an fp32 numpy restatement of the three collision() routines,
getCollision and inShadeCollisionDetection, in oracle/rt_oracle.c's operation order (one rounding per operation, sums left to
right, the finite plane's t compared in f64), vectorised over rays in chunks and looped over objects.  It is pinned to the
oracle -- whose only entry is orc_render, which stays as it is -- by two exact identities (identity_scene(), test_query_cpu.py):
with every object made a light of intensity 1 and colour (i + 1, 0, 0), a depth-0 1 x 1 frame of ray {E, T} returns the winner's
Scene index + 1, or NULL_COLOR on a miss; with the original colours kept, it returns the record's colour."""
import numpy as np

import oracle_lib

F = np.float32
HIT_DTYPE = np.dtype([("object", "<i4"), ("distance", "<f4"), ("point", "<f4", (3,)), ("normal", "<f4", (3,)),
                      ("color", "<f4", (3,)), ("flags", "<i4")])
SPHERE, INFINITE_PLANE, FINITE_PLANE = 0, 1, 2
CHUNK = 1 << 18


def _v(v):
    return np.array([v.x, v.y, v.z], dtype=F)


def _dot(a, b):
    """v_dot: a.x*b.x + a.y*b.y + a.z*b.z, left to right; a (..., 3) arrays or (3,) vectors"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _normalize(v):
    """v_normalize: sqrtf of the left-to-right sum of squares, three divides; -> (unit, length)"""
    length = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    return v / length[..., None], length


class Scene:
    """The oracle scene's objects as numpy records (oracle_lib.OracleScene -> what the restatement reads)."""

    def __init__(self, oscene):
        self.objects = [oscene.get_object(i) for i in range(oscene.object_count)]
        self.shadow_range = oscene.shadow_range()


def _checkerboard(o, x, y):
    """Texture_CheckerBoard::getTexturePixel -> True where the light tile's colour is returned"""
    w, h = F(o.tex_width), F(o.tex_height)
    with np.errstate(invalid="ignore"):
        xm = np.where(x >= 0, np.fmod(x, w), np.fmod(np.fmod(-x, w) + w / F(2.0), w))
        ym = np.where(y >= 0, np.fmod(y, h), np.fmod(np.fmod(-y, h) + h / F(2.0), h))
        return np.where(xm < w / F(2), ym < h / F(2), ~(ym < h / F(2)))


def _collision(o, E, d, want_record):
    """object_collision of one object against rays (E, d): (hit mask, distance[, point, normal, colour, inside])"""
    n = E.shape[0]
    with np.errstate(all="ignore"):
        if o.kind == SPHERE:
            OE = _v(o.origin)[None, :] - E
            v = _dot(OE, d)
            q = F(o.radius_squared) - (_dot(OE, OE) - v * v)
            root = np.sqrt(q)
            root1, root2 = v - root, v + root
            chosen = np.where(root1 < F(0), root2, root1)
            hit = ~(v < F(0)) & ~(q < F(1e-9)) & (root2 > F(0)) & (chosen < F(65535.0))
            dist = root1
            if not want_record:
                return hit, dist
            P = d * root1[:, None] + E
            N, _ = _normalize(P - _v(o.origin)[None, :])
            color = np.broadcast_to(_v(o.color), (n, 3))
            return hit, dist, P, N, color, root1 < F(0)
        normal = _v(o.normal)
        numerator = -F(o.distance_to_origin) - _dot(E, normal)
        denom = _dot(d, normal)
        t = numerator / denom
        if o.kind == INFINITE_PLANE:
            hit = ~(denom == F(0)) & ~(t < F(1e-10))
        else:
            hit = ~(denom == F(0)) & ~(t.astype(np.float64) < 1e-5)
        ip = d * t[:, None] + E
        if o.kind == FINITE_PLANE:
            PO = ip - _v(o.plane_origin)[None, :]
            x, y = _dot(PO, _v(o.horizontal)), _dot(PO, _v(o.vertical))
            hit &= ~((x < F(0)) | (x > F(o.h_distance)) | (y < F(0)) | (y > F(o.v_distance)))
        if not want_record:
            return hit, t
        if o.kind == INFINITE_PLANE:
            PO = ip - _v(o.origin)[None, :]
            x, y = _dot(PO, _v(o.horizontal)), _dot(PO, _v(o.vertical))
        if o.has_texture:
            color = np.where(_checkerboard(o, x, y)[:, None], _v(o.tex_light)[None, :], _v(o.tex_dark)[None, :])
        else:
            color = np.broadcast_to(_v(o.color), (n, 3))
        towards = (_dot(np.broadcast_to(normal, d.shape), d) < F(0))[:, None]
        N = np.where(towards, normal[None, :], _v(o.reverse_normal)[None, :])
        P = ip + N * F(1e-3)
        return hit, t, P, N, color, np.zeros(n, dtype=bool)


def directions(rays):
    """normalize(T - E) of rays (n, 6), createEyeRay's arithmetic"""
    with np.errstate(all="ignore"):
        return _normalize(rays[:, 3:] - rays[:, :3])[0]


def intersect(scene, rays):
    """getCollision(Ray(E, normalize(T - E))) of every ray of float32 (..., 6) -> HIT_DTYPE records of shape (...)"""
    flat = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    out = np.zeros(flat.shape[0], dtype=HIT_DTYPE)
    out["object"] = -1
    for c0 in range(0, flat.shape[0], CHUNK):
        E = flat[c0:c0 + CHUNK, :3]
        d = directions(flat[c0:c0 + CHUNK])
        n = E.shape[0]
        best = np.full(n, F(65535.0), dtype=F)
        idx = np.full(n, -1, dtype=np.int32)
        rec = {k: np.zeros((n, 3), dtype=F) for k in ("point", "normal", "color")}
        inside = np.zeros(n, dtype=bool)
        light = np.zeros(n, dtype=bool)
        for i, o in enumerate(scene.objects):
            hit, dist, P, N, color, ins = _collision(o, E, d, True)
            take = hit & (dist < best)
            if not take.any():
                continue
            best = np.where(take, dist, best)
            idx[take] = i
            rec["point"][take], rec["normal"][take], rec["color"][take] = P[take], N[take], color[take]
            inside[take] = ins[take]
            light[take] = bool(o.is_light)
        found = idx >= 0
        with np.errstate(all="ignore"):
            normal_ray = _normalize(rec["normal"])[0]          # the CollisionObject ctor: Ray(point, normal)
        o = out[c0:c0 + n]
        o["object"] = idx
        o["distance"] = np.where(found, best, F(0))
        o["point"] = np.where(found[:, None], rec["point"], F(0))
        o["normal"] = np.where(found[:, None], normal_ray, F(0))
        o["color"] = np.where(found[:, None], rec["color"], F(0))
        o["flags"] = np.where(found, inside.astype(np.int32) | (light.astype(np.int32) << 1), 0)
    return out.reshape(rays.shape[:-1])


def occluded(scene, segs):
    """inShadeCollisionDetection(Ray(E, T - E), |T - E|) of every segment of float32 (..., 6) -> bool of shape (...)"""
    flat = np.ascontiguousarray(segs, dtype=F).reshape(-1, 6)
    out = np.zeros(flat.shape[0], dtype=bool)
    begin, end = scene.shadow_range
    for c0 in range(0, flat.shape[0], CHUNK):
        E = flat[c0:c0 + CHUNK, :3]
        with np.errstate(all="ignore"):
            d, dist = _normalize(flat[c0:c0 + CHUNK, 3:] - E)
        blocked = np.zeros(E.shape[0], dtype=bool)
        for o in scene.objects[begin:end]:
            if o.is_light:
                continue
            hit, t = _collision(o, E, d, False)
            with np.errstate(invalid="ignore"):
                blocked |= hit & (t < dist)
        out[c0:c0 + E.shape[0]] = blocked
    return out.reshape(segs.shape[:-1])


def identity_scene(build, colours):
    """A fresh oracle scene from build() (a callable returning an OracleScene) with every object a light of intensity 1.
    colours = False: object i gets colour (i + 1, 0, 0), textured objects a checkerboard with both tiles that colour;
    colours = True: the original colours and textures are kept."""
    o = build()
    for i in range(o.object_count):
        ob = o.get_object(i)
        o.set_light(i)
        o.set_intensity(i, 1.0)
        if not colours:
            c = (float(i + 1), 0.0, 0.0)
            o.set_color(i, c)
            if ob.has_texture:
                o.set_checkerboard(i, c, c, ob.tex_width, ob.tex_height)
    return o


def oracle_objects(build, rays):
    """The winner's Scene index per ray through the object identity (-1: a miss), from depth-0 1 x 1 oracle frames"""
    from rays_ref import oracle_trace, positive_zeros
    rgb = oracle_trace(identity_scene(build, False), positive_zeros(rays), 0)
    null = np.float32(0.75)
    miss = (rgb[..., 0] == null) & (rgb[..., 1] == null) & (rgb[..., 2] == null)
    return np.where(miss, -1, rgb[..., 0].astype(np.int64) - 1)


def oracle_colours(build, rays):
    """The hit colour per ray through the colour identity (a miss: NULL_COLOR)"""
    from rays_ref import oracle_trace, positive_zeros
    return oracle_trace(identity_scene(build, True), positive_zeros(rays), 0)


def scene_of(build):
    return Scene(build())


__all__ = ["HIT_DTYPE", "Scene", "intersect", "occluded", "identity_scene", "oracle_objects", "oracle_colours", "scene_of",
           "oracle_lib"]
