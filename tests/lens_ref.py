"""The reference of include/rt_capi_lens.h, for the tests: the header's definition restated in numpy fp32, one rounding per
operation, the sums in the order written -- the rays of a thin-lens camera and the ordered average of their colours -- and the
frames the GPU tests compare with the CPU oracle, each computed once."""
import functools

import numpy as np

import adaptive_frames
import cameras
import rays_ref
from rays_ref import _xyz
from soft_ref import GOLDEN, H as lowbias32

F = np.float32
U32 = np.uint32


def strata(W, H, x0, x1, n, seed):
    """-> (h uint32 (cols, H), sp int (cols, H, S)): each pixel's hash and the lens stratum of each of its samples"""
    S = n * n
    x = np.arange(x0, x1, dtype=np.int64)[:, None]
    z = np.arange(H, dtype=np.int64)[None, :]
    key = ((x * H + z) & 0xFFFFFFFF).astype(U32)
    h = lowbias32(lowbias32(U32(seed & 0xFFFFFFFF) ^ GOLDEN) ^ key)
    rot = h % U32(S)
    s = np.arange(S, dtype=U32)[None, None, :]
    return h, ((s + rot[..., None]) % U32(S)).astype(np.int64)


def lens_points(W, H, x0, x1, n, seed):
    """-> (u, v) float32 (cols, H, S): every sample's point of the unit disc"""
    S = n * n
    h, sp = strata(W, H, x0, x1, n, seed)
    li, lj = sp // n, sp % n
    s = np.arange(S, dtype=U32)[None, None, :]
    hs = lowbias32(h[..., None] ^ s)
    xi1 = (hs >> U32(8)).astype(F) * F(2.0 ** -24)
    xi2 = (lowbias32(hs ^ GOLDEN) >> U32(8)).astype(F) * F(2.0 ** -24)
    step = F(2.0) / F(n)
    a = (li.astype(F) + xi1) * step - F(1.0)
    b = (lj.astype(F) + xi2) * step - F(1.0)
    u = a * np.sqrt(F(1.0) - (b * b) * F(0.5))
    v = b * np.sqrt(F(1.0) - (a * a) * F(0.5))
    return u.astype(F), v.astype(F)


def rays(cam, W, H, x0, x1, n, seed, aperture, focus):
    """the header's rays of columns [x0, x1) of a W x H frame -> float32 (cols, H, S, 6), ray [x - x0, z, i * n + j] = {O, T}"""
    if hasattr(cam, "contents"):
        cam = cam.contents
    S, cols = n * n, x1 - x0
    aperture, g = F(aperture), F(focus) - F(1.0)
    so, ch, cv, eye = (_xyz(v) for v in (cam.screen_origin, cam.vector_horizontal, cam.vector_vertical, cam.eye_origin))
    i = (np.arange(S) // n)[None, None, :]
    j = (np.arange(S) % n)[None, None, :]
    x = np.arange(x0, x1)[:, None, None]
    z = np.arange(H)[None, :, None]
    dx = np.broadcast_to((n * x + i).astype(F) / F(n * W), (cols, H, S))
    dz = np.broadcast_to((n * z + j).astype(F) / F(n * H), (cols, H, S))
    sx = dx * F(cam.screen_width) - F(cam.screen_halfwidth)
    sz = dz * F(cam.screen_height) - F(cam.screen_halfheight)
    out = np.empty((cols, H, S, 6), dtype=F)
    if aperture != 0:
        u, v = lens_points(W, H, x0, x1, n, seed)
        au, av = aperture * u, aperture * v
    for c in range(3):
        P = (so[c] + ch[c] * sx) + cv[c] * sz
        out[..., 3 + c] = P + (P - eye[c]) * g
        out[..., c] = eye[c] if aperture == 0 else eye[c] + (ch[c] * au + cv[c] * av)
    return out


def camera_copy(host):
    """a HostScene's camera as an RtCameraDesc of its own (host.camera.contents lives only as long as the scene does)"""
    import ctypes as C
    from tilecoderaytracer_amd.capi import RtCameraDesc
    cam = RtCameraDesc()
    C.memmove(C.byref(cam), host.camera, C.sizeof(RtCameraDesc))
    return cam


def resolve(colours, n):
    """colours float32 (..., S, 3) -> (..., 3): the S colours summed strictly in order, then divided by (float)S"""
    S = n * n
    assert colours.shape[-2] == S and colours.dtype == F
    acc = colours[..., 0, :].copy()
    for s in range(1, S):
        acc = acc + colours[..., s, :]
    return acc / F(S)


# ---- the frames compared with the CPU oracle ------------------------------------------------------------------------------------

def focus_on(cam, point):
    """the focus that puts the focal plane through `point`: its distance along the viewing axis over the screen's"""
    if hasattr(cam, "contents"):
        cam = cam.contents
    eye, so = _xyz(cam.eye_origin).astype(np.float64), _xyz(cam.screen_origin).astype(np.float64)
    axis = so - eye
    return float(np.dot(np.asarray(point, np.float64) - eye, axis) / np.dot(axis, axis))


def screen_distance(cam):
    if hasattr(cam, "contents"):
        cam = cam.contents
    return float(np.linalg.norm(_xyz(cam.screen_origin).astype(np.float64) - _xyz(cam.eye_origin).astype(np.float64)))


def lens_of(key, focal_point):
    """(aperture, focus) of scene `key`: the focal plane through focal_point, the lens radius 1 / 20 of the eye's distance to it
    (the aperture is in units of the screen vectors, which are unit vectors in these scenes); both rounded to fp32"""
    cam = adaptive_frames.oracle_scene(key).cam
    focus = focus_on(cam, focal_point)
    return float(F(focus * screen_distance(cam) / 20.0)), float(F(focus))


# (key, W, H, depth, n, seed, the point the focal plane passes through): builtin's is its anchor (cameras.ANCHORS); the sphere
# grid's and the random scene's, which have none, a point among their objects
FRAMES = [
    ("builtin", 61, 37, 4, 4, 0, cameras.ANCHORS["builtin"]["focus"]),
    ("grid16", 48, 44, 5, 3, 7, (0.0, 7.0, 2.5)),
    ("random2", 36, 28, 5, 2, 0x9E3779B9, (0.0, 17.0, 2.5)),
]


@functools.lru_cache(maxsize=None)
def oracle_frame(key, W, H, depth, n, seed, aperture, focus):
    """resolve(oracle_trace(rays(...))) of the whole frame, read-only"""
    orc = adaptive_frames.oracle_scene(key)
    r = rays(orc.cam, W, H, 0, W, n, seed, aperture, focus)
    out = np.ascontiguousarray(resolve(rays_ref.oracle_trace(orc, r, depth), n))
    out.setflags(write=False)
    return out


def distinct_colours(frame):
    return len(np.unique(np.ascontiguousarray(frame).view(np.uint32).reshape(-1, 3), axis=0))


def changed_share(frame, pinhole):
    same = (np.ascontiguousarray(frame).view(np.uint32) == np.ascontiguousarray(pinhole).view(np.uint32)).all(axis=-1)
    return 1.0 - same.mean()
