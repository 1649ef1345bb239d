"""The reference of include/rt_capi_rays.h, for the tests: the rays rt_render traces, built in numpy, and the oracle's result
for any ray.  A ray (E, T) is pixel (0, 0) of a 1 x 1 oracle frame whose camera has eye_origin = E, screen_origin = T and zero
screen vectors and sizes: create_eye_ray then computes normalize(((T + 0) + 0) - E), which is normalize(T - E) once any -0.0 in T
is +0.0 (positive_zeros)."""
import ctypes as C

import numpy as np

import oracle_lib


def _xyz(v):
    """a camera vector of either binding (RtCameraDesc: float[3]; OrcCamera: Vec3) -> float32 (3,)"""
    if hasattr(v, "x"):
        return np.array([v.x, v.y, v.z], dtype=np.float32)
    return np.array([v[0], v[1], v[2]], dtype=np.float32)


def camera_rays(cam, W, H):
    """The (W, H, 6) rays rt_render traces for a W x H frame of `cam` (RtCameraDesc, a pointer to one, or OrcCamera), in
    pixels[x][z] order: {eye, pixel}, the pixel as create_eye_ray computes it in fp32, one rounding per operation."""
    if hasattr(cam, "contents"):
        cam = cam.contents
    f = np.float32
    dx = np.arange(W, dtype=np.float32) / f(W)                   # (float)x / W
    dz = np.arange(H, dtype=np.float32) / f(H)
    scalar_x = dx * f(cam.screen_width) - f(cam.screen_halfwidth)
    scalar_y = dz * f(cam.screen_height) - f(cam.screen_halfheight)
    so, ch, cv = _xyz(cam.screen_origin), _xyz(cam.vector_horizontal), _xyz(cam.vector_vertical)
    pixel = so[None, None, :] + ch[None, None, :] * scalar_x[:, None, None]       # screen_origin + horizontal * scalar_x
    pixel = pixel + cv[None, None, :] * scalar_y[None, :, None]                   # ... + vertical * scalar_y
    rays = np.empty((W, H, 6), dtype=np.float32)
    rays[..., :3] = _xyz(cam.eye_origin)
    rays[..., 3:] = pixel
    return rays


def positive_zeros(rays):
    """rays with every -0.0 of the targets replaced by +0.0 (a copy)"""
    r = np.array(rays, dtype=np.float32, copy=True)
    t = r[..., 3:]
    t[t == 0] = np.float32(0.0)
    return r


def oracle_trace(oscene, rays, depth):
    """The oracle's result for every ray of `rays` (float32 (..., 6)): one 1 x 1 frame per ray -> float32 (..., 3)."""
    flat = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    out = np.empty((flat.shape[0], 3), dtype=np.float32)
    cam = oracle_lib.OrcCamera()
    C.memset(C.byref(cam), 0, C.sizeof(cam))                      # zero screen vectors and sizes
    render, ptr, one = oracle_lib.LIB.orc_render, C.byref(cam), np.empty(3, dtype=np.float32)
    for i, (ex, ey, ez, tx, ty, tz) in enumerate(flat.tolist()):
        cam.eye_origin = oracle_lib.Vec3(ex, ey, ez)
        cam.screen_origin = oracle_lib.Vec3(tx, ty, tz)
        assert render(oscene.h, ptr, 1, 1, 0, 1, depth, one.ctypes.data) == 0
        out[i] = one
    return out.reshape(rays.shape[:-1] + (3,))
