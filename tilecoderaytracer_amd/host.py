"""Bindings to lib/libtcrt_host.so: the C++ host model that mirrors the
reference's Scene / SceneObject / Camera API (csrc/host/celio_model.hpp).

A :class:`HostScene` is a reference ``Scene`` plus a ``Camera``; it is built
with the same calls a user of the reference makes (``add_sphere`` = ``new
SceneSphere`` + ``addObject`` ...), and ``desc`` / ``camera`` give the
flattened plain-old-data views that cross the C ABI.  Nothing here renders.
"""
import ctypes as C
import os

import numpy as np

from .capi import LIB_DIR, RtAreaLightDesc, RtCameraDesc, RtImageTextureDesc, RtRefractionDesc, RtSceneDesc, F3

_hlib = None


def host_library_path():
    return os.path.join(LIB_DIR, "libtcrt_host.so")


def load_host_library():
    global _hlib
    if _hlib is not None:
        return _hlib
    path = host_library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build it with `make -C tilecoderaytracer_amd/csrc`")
    lib = C.CDLL(path)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    pf = C.POINTER(C.c_float)
    lib.rth_scene_new.argtypes = [C.POINTER(vp)]
    lib.rth_scene_builtin.argtypes = [C.POINTER(vp)]
    lib.rth_scene_two_mirrors.argtypes = [C.POINTER(vp)]
    lib.rth_scene_grid.argtypes = [i, i, C.POINTER(vp)]
    lib.rth_scene_free.argtypes = [vp]
    lib.rth_scene_free.restype = None
    lib.rth_add_sphere.argtypes = [vp, pf, f]
    lib.rth_add_infinite_plane.argtypes = [vp, pf, pf, pf]
    lib.rth_add_finite_plane_corners.argtypes = [vp, pf, pf, pf]
    lib.rth_add_finite_plane_axes.argtypes = [vp, pf, pf, pf, f, f]
    lib.rth_object_count.argtypes = [vp]
    lib.rth_set_color.argtypes = [vp, i, pf]
    lib.rth_set_diffuse.argtypes = [vp, i, f]
    lib.rth_set_specular.argtypes = [vp, i, f]
    lib.rth_set_reflective.argtypes = [vp, i, f]
    lib.rth_set_refraction.argtypes = [vp, i, f, f]
    lib.rth_set_area_light.argtypes = [vp, i, i, f]
    lib.rth_set_checkerboard.argtypes = [vp, i, pf, pf, f, f]
    lib.rth_set_image_texture.argtypes = [vp, i, i, i, vp, f, f, i]
    lib.rth_set_light.argtypes = [vp, i]
    lib.rth_set_intensity.argtypes = [vp, i, f]
    lib.rth_set_object_indices.argtypes = [vp, i, i]
    lib.rth_camera_two_mirrors.argtypes = [vp]
    lib.rth_camera_eye_ray.argtypes = [vp, f, f, pf, pf]
    lib.rth_scene_desc.argtypes = [vp]
    lib.rth_scene_desc.restype = C.POINTER(RtSceneDesc)
    lib.rth_scene_images.argtypes = [vp, C.POINTER(C.POINTER(RtImageTextureDesc))]
    lib.rth_scene_images.restype = i
    lib.rth_scene_refractions.argtypes = [vp, C.POINTER(C.POINTER(RtRefractionDesc))]
    lib.rth_scene_refractions.restype = i
    lib.rth_scene_area_lights.argtypes = [vp, C.POINTER(C.POINTER(RtAreaLightDesc))]
    lib.rth_scene_area_lights.restype = i
    lib.rth_camera_desc.argtypes = [vp]
    lib.rth_camera_desc.restype = C.POINTER(RtCameraDesc)
    lib.rth_write_screen_txt.argtypes = [C.c_char_p, i, i, vp, C.c_double, C.c_double]
    lib.rth_write_screen_txt_cores.argtypes = [C.c_char_p, i, i, vp, C.c_double, C.c_double, i]
    lib.rth_write_screen_ppm.argtypes = [C.c_char_p, i, i, vp, C.c_uint64]
    _hlib = lib
    return lib


def _v(p):
    return F3(*[float(x) for x in p])


class HostScene:
    """A reference ``Scene`` + ``Camera`` living in the C++ host model."""

    def __init__(self, handle):
        self._lib = load_host_library()
        self._h = handle

    # -- whole scenes ---------------------------------------------------
    @classmethod
    def _make(cls, fn, *args):
        lib = load_host_library()
        h = C.c_void_p()
        if fn(lib)(*args, C.byref(h)) != 0 or not h:
            raise RuntimeError("host scene construction failed")
        return cls(h)

    @classmethod
    def empty(cls):
        return cls._make(lambda l: l.rth_scene_new)

    @classmethod
    def builtin(cls):
        """``Scene::initialize()`` + default ``Camera()`` (the museum)."""
        return cls._make(lambda l: l.rth_scene_builtin)

    @classmethod
    def two_mirrors(cls):
        """``Scene::initializeTwoMirrors(&camera)``."""
        return cls._make(lambda l: l.rth_scene_two_mirrors)

    @classmethod
    def grid(cls, n, shadows=True):
        """Synthetic grid-n scene; camera = setSceneTwoMirrors()."""
        return cls._make(lambda l: l.rth_scene_grid, int(n), 1 if shadows else 0)

    @classmethod
    def named(cls, name):
        """'builtin' | 'twomirrors' | 'grid<N>' | 'grid<N>-noshadow'."""
        if name == "builtin":
            return cls.builtin()
        if name == "twomirrors":
            return cls.two_mirrors()
        if name.startswith("grid"):
            body = name[4:]
            shadows = not body.endswith("-noshadow")
            if not shadows:
                body = body[: -len("-noshadow")]
            return cls.grid(int(body), shadows)
        raise ValueError(f"unknown scene {name!r}")

    def close(self):
        if self._h:
            self._lib.rth_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- reference-style building ---------------------------------------
    def add_sphere(self, origin, radius):
        return self._lib.rth_add_sphere(self._h, _v(origin), radius)

    def add_infinite_plane(self, o, n, h):
        return self._lib.rth_add_infinite_plane(self._h, _v(o), _v(n), _v(h))

    def add_finite_plane_corners(self, o, vcorner, hcorner):
        return self._lib.rth_add_finite_plane_corners(self._h, _v(o), _v(vcorner), _v(hcorner))

    def add_finite_plane_axes(self, o, n, h, v_dist, h_dist):
        return self._lib.rth_add_finite_plane_axes(self._h, _v(o), _v(n), _v(h), v_dist, h_dist)

    @property
    def object_count(self):
        return self._lib.rth_object_count(self._h)

    def _ok(self, rc):
        if rc != 0:
            raise RuntimeError("host model call failed (bad index?)")

    def set_color(self, idx, rgb): self._ok(self._lib.rth_set_color(self._h, idx, _v(rgb)))
    def set_diffuse(self, idx, f): self._ok(self._lib.rth_set_diffuse(self._h, idx, f))
    def set_specular(self, idx, f): self._ok(self._lib.rth_set_specular(self._h, idx, f))
    def set_reflective(self, idx, f): self._ok(self._lib.rth_set_reflective(self._h, idx, f))
    def set_refraction(self, idx, factor, ior=1.0):
        """ObjMaterial::setRefractiveFactor(factor) and setRefractiveIndex(ior) (include/rt_capi_refract.h)"""
        self._ok(self._lib.rth_set_refraction(self._h, idx, factor, ior))
    def set_area_light(self, idx, samples, radius=None):
        """SceneObject::setAreaLight (include/rt_capi_soft.h): light idx sampled as an area light, samples x samples per
        shading point on a disc of the radius (None: the object's own -- a sphere's radius)"""
        self._ok(self._lib.rth_set_area_light(self._h, idx, samples, -1.0 if radius is None else radius))
    def set_checkerboard(self, idx, light, dark, w, h):
        self._ok(self._lib.rth_set_checkerboard(self._h, idx, _v(light), _v(dark), w, h))
    def set_image_texture(self, idx, texels, w, h, wrap):
        """a Texture_Image (include/rt_capi_texture.h): texels float32 (texels_h, texels_w, 3), texels[j, i] texel (i, j),
        copied; w, h the world size of one copy, wrap RT_TEX_WRAP_*"""
        t = np.ascontiguousarray(texels, dtype=np.float32)
        if t.ndim != 3 or t.shape[2] != 3:
            raise ValueError("texels must be (texels_h, texels_w, 3)")
        self._ok(self._lib.rth_set_image_texture(self._h, idx, t.shape[1], t.shape[0], t.ctypes.data, w, h, wrap))

    def set_light(self, idx): self._ok(self._lib.rth_set_light(self._h, idx))
    def set_intensity(self, idx, f): self._ok(self._lib.rth_set_intensity(self._h, idx, f))
    def set_object_indices(self, my_rank, group_size):
        self._ok(self._lib.rth_set_object_indices(self._h, my_rank, group_size))
    def camera_two_mirrors(self): self._ok(self._lib.rth_camera_two_mirrors(self._h))

    def eye_ray(self, dx, dy):
        o, d = F3(), F3()
        self._ok(self._lib.rth_camera_eye_ray(self._h, dx, dy, o, d))
        return tuple(o), tuple(d)

    # -- flattened views (valid while self is alive and unmodified) -----
    @property
    def desc(self):
        return self._lib.rth_scene_desc(self._h)

    @property
    def images(self):
        """the flattened scene's images (texture indices n_textures + k): (count, pointer to RtImageTextureDesc or None)"""
        ptr = C.POINTER(RtImageTextureDesc)()
        n = self._lib.rth_scene_images(self._h, C.byref(ptr))
        return n, (ptr if n else None)

    @property
    def refractions(self):
        """the flattened scene's refractive objects: (count, pointer to RtRefractionDesc or None)"""
        ptr = C.POINTER(RtRefractionDesc)()
        n = self._lib.rth_scene_refractions(self._h, C.byref(ptr))
        return n, (ptr if n else None)

    @property
    def area_lights(self):
        """the flattened scene's area lights: (count, pointer to RtAreaLightDesc or None)"""
        ptr = C.POINTER(RtAreaLightDesc)()
        n = self._lib.rth_scene_area_lights(self._h, C.byref(ptr))
        return n, (ptr if n else None)

    @property
    def camera(self):
        return self._lib.rth_camera_desc(self._h)


def write_screen_txt(path, rgb, run_time_s=0.0, us_per_pixel=0.0, n_cores=1):
    """Write ``raytracer_screen.txt`` for a (W, H, 3) float32 array; n_cores = GPUs that rendered it
    (CORE_NUM and the partition label of the header, src/RayTracer.cpp:2037-2058)."""
    import numpy as np
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    W, H = a.shape[0], a.shape[1]
    rc = load_host_library().rth_write_screen_txt_cores(os.fsencode(path), W, H, a.ctypes.data,
                                                        run_time_s, us_per_pixel, int(n_cores))
    if rc != 0:
        raise OSError(f"could not write {path}")


def write_ppm(path, image):
    """Write a binary PPM (P6) of a uint8 (H, W, 3) array, row 0 first: encode_image()'s result with 3 channels.  The rows may be
    a view with a pitch (image.strides[0] >= 3 W), e.g. three columns' worth cut out of a wider image."""
    a = np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"image must be uint8 (H, W, 3), not {a.dtype} {a.shape}")
    if a.strides[1:] != (3, 1) or a.strides[0] < 3 * a.shape[1]:
        a = np.ascontiguousarray(a)
    if load_host_library().rth_write_screen_ppm(os.fsencode(path), a.shape[1], a.shape[0], a.ctypes.data, a.strides[0]) != 0:
        raise OSError(f"could not write {path}")
