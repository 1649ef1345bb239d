"""The reference of include/rt_capi_texture.h, for the tests: an fp32 numpy restatement of the image fold, of the texel
column / row rule and of a ray's plane texture coordinates.  The coordinates come from query_ref's restatement of getCollision
(pinned to the oracle): a plane winner's distance t gives ip = d t + E, PO = ip - the plane's texture origin, x = PO . horizontal,
y = PO . vertical -- the values the checkerboard receives.  With 2 x 2 CHECKER images, colours() is query_ref's checkerboard
colour bit for bit (test_texture_cpu.py), which ties this file to the oracle as well."""
import numpy as np

import query_ref

F = np.float32
CHECKER, REPEAT, CLAMP = 0, 1, 2


def fold(x, w, wrap):
    """x (float32 array) folded into [0, w] by `wrap`, in the definition's fp32 order"""
    x = np.asarray(x, dtype=F)
    w = F(w)
    with np.errstate(invalid="ignore"):
        if wrap == CHECKER:
            return np.where(x >= 0, np.fmod(x, w), np.fmod(np.fmod(-x, w) + w / F(2), w)).astype(F)
        if wrap == REPEAT:
            r = np.fmod(x, w)
            return np.where(r < 0, r + w, r).astype(F)
        if wrap == CLAMP:
            c = np.where(x < 0, F(0), x)
            return np.where(c > w, w, c).astype(F)
    raise ValueError(wrap)


def bounds(w, n):
    """b_k = fl(fl(w k) / n), k = 0 .. n - 1 (w k may overflow to inf, as it does in fp32)"""
    with np.errstate(over="ignore"):
        return (F(w) * np.arange(n, dtype=F)) / F(n)


def cell(u, w, n):
    """(n - 1) - #{k in [1, n) : u < b_k}; a NaN gives n - 1"""
    u = np.asarray(u, dtype=F)
    b = bounds(w, n)[1:]
    # the b_k do not decrease, so #{k : u < b_k} = (n - 1) - #{k : b_k <= u}; a NaN is below no b_k
    i = np.searchsorted(b, u, side="right")
    return np.where(np.isnan(u), n - 1, i).astype(np.int64)


def cell_by_definition(u, w, n):
    """the same, by the definition's count (slow: for the tests of cell())"""
    u = np.asarray(u, dtype=F)
    b = bounds(w, n)
    count = np.zeros(u.shape, dtype=np.int64)
    for k in range(1, n):
        count += (u < b[k])
    return (n - 1) - count


def texel(x, y, image):
    """texel index j * texels_w + i of coordinates (x, y) in image = (texels (h, w, 3), width, height, wrap)"""
    texels, width, height, wrap = image
    th, tw = texels.shape[:2]
    i = cell(fold(x, width, wrap), width, tw)
    j = cell(fold(y, height, wrap), height, th)
    return j * tw + i


def colour(x, y, image):
    t = np.asarray(image[0], dtype=F).reshape(-1, 3)
    return t[texel(x, y, image)]


def checker_image(light, dark, width, height):
    """the 2 x 2 CHECKER image that reproduces a checkerboard"""
    t = np.array([[light, dark], [dark, light]], dtype=F)
    return (t, F(width), F(height), CHECKER)


def plane_coords(scene, rays, hits):
    """the texture coordinates (x, y) of each ray's nearest hit, NaN where it is not a plane; scene: query_ref.Scene,
    rays (n, 6) float32, hits: query_ref.intersect's records of them"""
    rays = np.asarray(rays, dtype=F).reshape(-1, 6)
    hits = hits.reshape(-1)
    d = query_ref.directions(rays)
    E = rays[:, :3]
    x = np.full(len(rays), np.nan, dtype=F)
    y = x.copy()
    for k, o in enumerate(scene.objects):
        sel = hits["object"] == k
        if o.kind == query_ref.SPHERE or not sel.any():
            continue
        t = hits["distance"][sel]
        with np.errstate(all="ignore"):
            ip = d[sel] * t[:, None] + E[sel]
            anchor = query_ref._v(o.origin if o.kind == query_ref.INFINITE_PLANE else o.plane_origin)
            PO = ip - anchor[None, :]
            x[sel] = query_ref._dot(PO, query_ref._v(o.horizontal))
            y[sel] = query_ref._dot(PO, query_ref._v(o.vertical))
    return x, y


def colours(scene, rays, images_of):
    """query_ref's record colours of rays, with the planes in images_of ({Scene index: image}) coloured by their texels"""
    hits = query_ref.intersect(scene, np.asarray(rays, dtype=F).reshape(-1, 6))
    x, y = plane_coords(scene, rays, hits)
    out = hits["color"].reshape(-1, 3).copy()
    for k, image in images_of.items():
        sel = hits["object"].reshape(-1) == k
        if sel.any() and scene.objects[k].kind != query_ref.SPHERE:
            out[sel] = colour(x[sel], y[sel], image)
    return hits, out
