"""Convenience wrapper over the C ABI for tests and bench.py."""
import ctypes as C

import numpy as np

from . import capi

# rt_hit of include/rt_capi_query.h: 48 bytes
HIT_DTYPE = np.dtype([("object", "<i4"), ("distance", "<f4"), ("point", "<f4", (3,)), ("normal", "<f4", (3,)),
                      ("color", "<f4", (3,)), ("flags", "<i4")])
assert HIT_DTYPE.itemsize == 48


def image_descs(images):
    """(texels, width, height, wrap) tuples -> (the C-contiguous float32 arrays, an RtImageTextureDesc array over them)."""
    arrays = [np.ascontiguousarray(t, dtype=np.float32) for t, _, _, _ in images]
    descs = (capi.RtImageTextureDesc * max(len(images), 1))()
    for k, (a, (_, width, height, wrap)) in enumerate(zip(arrays, images)):
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("image %d: texels must be (texels_h, texels_w, 3)" % k)
        descs[k] = capi.RtImageTextureDesc(a.shape[1], a.shape[0], width, height, wrap,
                                           a.ctypes.data_as(C.POINTER(C.c_float)))
    return arrays, descs


def refraction_descs(refractive):
    """(object, tf, ior) tuples -> an RtRefractionDesc array (include/rt_capi_refract.h)."""
    descs = (capi.RtRefractionDesc * max(len(refractive), 1))()
    for k, (obj, tf, ior) in enumerate(refractive):
        descs[k] = capi.RtRefractionDesc(obj, tf, ior)
    return descs


def area_light_descs(area_lights):
    """(object, samples, radius) tuples -> an RtAreaLightDesc array (include/rt_capi_soft.h)."""
    descs = (capi.RtAreaLightDesc * max(len(area_lights), 1))()
    for k, (obj, n, r) in enumerate(area_lights):
        descs[k] = capi.RtAreaLightDesc(obj, n, r)
    return descs


def denoise(rgb, hits, iterations=2, sigma_color=1.0, normal_squarings=3, device=0):
    """Filter a frame's colours by its hit records (include/rt_capi_denoise.h, rt_denoise): rgb float32 (Wn, H, 3) and hits
    HIT_DTYPE (Wn, H), as render_gbuffer() returns them (a whole frame or a strip) -> the filtered float32 (Wn, H, 3).  Runs on GPU
    `device`; there is no CPU path."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or hits.shape != rgb.shape[:2]:
        raise ValueError(f"rgb must be (Wn, H, 3) and hits (Wn, H), not {rgb.shape} and {hits.shape}")
    params = capi.RtDenoiseParams(int(iterations), int(normal_squarings), float(sigma_color))
    out = np.empty_like(rgb)
    capi.check(capi.load_library().rt_denoise(int(device), C.byref(params), rgb.shape[0], rgb.shape[1], rgb.ctypes.data,
                                              hits.ctypes.data, out.ctypes.data, None))
    return out


def adaptive_params(samples=2, color_threshold=1 / 32, normal_cos=0.9, flag_all=False, chunk_pixels=0):
    """render_adaptive's keywords -> an RtAdaptiveParams (include/rt_capi_adaptive.h); the library checks the values."""
    return capi.RtAdaptiveParams(int(samples), int(flag_all), int(chunk_pixels), float(color_threshold), float(normal_cos))


def adaptive_flags(rgb, hits, color_threshold=1 / 32, normal_cos=0.9, flag_all=False, device=0):
    """Which pixels of a rectangle an edge passes through (include/rt_capi_adaptive.h, rt_adaptive_flags): rgb float32 (Wn, H, 3)
    and hits HIT_DTYPE (Wn, H), as render_gbuffer() returns them -> bool (Wn, H): the pixel differs from one of the three other
    corners of its footprint, (x+1, z), (x, z+1), (x+1, z+1), in object, in normal (cosine below normal_cos) or in a colour
    channel (by more than color_threshold; a NaN flags).  Runs on GPU `device`; there is no CPU path."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or hits.shape != rgb.shape[:2]:
        raise ValueError(f"rgb must be (Wn, H, 3) and hits (Wn, H), not {rgb.shape} and {hits.shape}")
    params = adaptive_params(1, color_threshold, normal_cos, flag_all)
    out = np.empty(rgb.shape[:2], dtype=np.uint8)
    capi.check(capi.load_library().rt_adaptive_flags(int(device), C.byref(params), rgb.shape[0], rgb.shape[1], rgb.ctypes.data,
                                                     hits.ctypes.data, out.ctypes.data))
    return out.view(np.bool_)


def lens_params(samples=4, aperture=0.0, focus=1.0, seed=0, chunk_columns=0):
    """render_lens's keywords -> an RtLensParams (include/rt_capi_lens.h); the library checks the values."""
    return capi.RtLensParams(int(samples), int(chunk_columns), int(seed) & 0xFFFFFFFF, float(aperture), float(focus))


def lens_rays(camera, W, H, samples=4, aperture=0.0, focus=1.0, seed=0, x0=0, x1=None, device=0):
    """The rays of a thin-lens camera (include/rt_capi_lens.h, rt_lens_rays): columns [x0, x1) of a W x H frame of camera (an
    RtCameraDesc), samples x samples rays a pixel -> float32 (x1-x0, H, samples^2, 6), ray [x - x0, z, s] = {O.xyz, T.xyz}: from
    its point of the lens through its target on the focal plane.  What render_lens() traces; trace_rays() takes them as they
    are.  Runs on GPU `device`; there is no CPU path."""
    x1 = W if x1 is None else x1
    params = lens_params(samples, aperture, focus, seed)
    S = params.samples ** 2 if 1 <= params.samples <= 8 else 1        # (a bad count is refused by the call below)
    out = np.empty((max(x1 - x0, 0), max(H, 0), S, 6), dtype=np.float32)
    capi.check(capi.load_library().rt_lens_rays(C.byref(camera), W, H, x0, x1, C.byref(params), int(device), out.ctypes.data))
    return out


def indirect_params(samples=4, gather_depth=1, gain=1.0, seed=0, key0=0, emitters=False, chunk_records=0):
    """indirect_diffuse's keywords -> an RtIndirectParams (include/rt_capi_indirect.h); the library checks the values."""
    return capi.RtIndirectParams(int(samples), int(gather_depth), int(chunk_records), int(emitters), int(seed) & 0xFFFFFFFF,
                                 int(key0) & 0xFFFFFFFF, float(gain))


def paths_params(samples=4, gather_depth=1, gain=1.0, seed=0, key0=0, emitters=False, chunk_records=0, bounces=2):
    """indirect_paths' keywords -> an RtPathsParams (include/rt_paths.h); the library checks the values."""
    return capi.RtPathsParams(int(samples), int(gather_depth), int(chunk_records), int(emitters), int(seed) & 0xFFFFFFFF,
                              int(key0) & 0xFFFFFFFF, float(gain), int(bounces))


def glass_params(max_bounces=8, min_reflective=1.0, min_transmissive=0.5, chunk_rays=0):
    """glass_records' keywords -> an RtGlassParams (include/rt_glass.h); the library checks the values."""
    return capi.RtGlassParams(int(max_bounces), int(chunk_rays), float(min_reflective), float(min_transmissive))


def mirror_params(max_bounces=8, min_reflective=1.0, chunk_rays=0):
    """mirror_records' keywords -> an RtMirrorParams (include/rt_mirror.h); the library checks the values."""
    return capi.RtMirrorParams(int(max_bounces), int(chunk_rays), float(min_reflective))


def _records(hits):
    if not isinstance(hits, np.ndarray) or hits.dtype != HIT_DTYPE or not hits.flags.c_contiguous:
        raise TypeError("hits must be a C-contiguous numpy array of HIT_DTYPE")
    return hits


def indirect_rays(hits, samples, seed=0, key0=0, device=0):
    """The gather rays of one diffuse bounce (include/rt_capi_indirect.h, rt_indirect_rays): for every record of hits (HIT_DTYPE,
    any shape) samples x samples rays from the record's point into the hemisphere around its normal, in ambient_occlusion()'s
    directions -> float32 hits.shape + (samples^2, 6), ray [..., s] = {P.xyz, T.xyz}; a miss's or a light's rays are zeros.
    Record i samples with key0 + i.  What indirect_diffuse() traces; trace_rays() takes them as they are.  Runs on GPU
    `device`; there is no CPU path."""
    hits = _records(hits)
    params = indirect_params(samples, seed=seed, key0=key0)
    S = params.samples ** 2 if 1 <= params.samples <= 8 else 1        # (a bad count is refused by the call below)
    out = np.empty(hits.shape + (S, 6), dtype=np.float32)
    capi.check(capi.load_library().rt_indirect_rays(C.byref(params), hits.size, hits.ctypes.data, int(device), out.ctypes.data))
    return out


def _frame_records(hits):
    hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
    if hits.ndim != 2:
        raise ValueError(f"hits must be (Wn, H), not {hits.shape}")
    return hits


def subsample_hits(hits, scale, white=False, device=0):
    """The records of every scale-th pixel in both directions (include/rt_capi_upsample.h, rt_subsample_hits): hits HIT_DTYPE
    (Wn, H) as render_gbuffer() returns them -> HIT_DTYPE (ceil(Wn / scale), ceil(H / scale)), cell [i, j] = hits[i * scale,
    j * scale] word for word; white: a live record's colour becomes (1, 1, 1), so that indirect_diffuse() of the cells is
    irradiance without albedo.  Runs on GPU `device`; there is no CPU path."""
    hits = _frame_records(hits)
    s = int(scale)
    out = np.empty((-(-hits.shape[0] // s), -(-hits.shape[1] // s)) if 2 <= s <= 8 else (0, 0), dtype=HIT_DTYPE)
    capi.check(capi.load_library().rt_subsample_hits(int(device), s, int(white), hits.shape[0], hits.shape[1], hits.ctypes.data,
                                                     out.ctypes.data if out.size else None))
    return out


def upsample_params(scale, channels=3, normal_squarings=3, match_color=False, modulate=False, sigma_plane=0.0, dead_value=0.0):
    """upsample_guided's keywords -> an RtUpsampleParams (include/rt_capi_upsample.h); the library checks the values."""
    return capi.RtUpsampleParams(int(scale), int(channels), int(normal_squarings), int(match_color), int(modulate),
                                 float(sigma_plane), float(dead_value))


def upsample_guided(hits, lo, scale, normal_squarings=3, match_color=False, modulate=False, sigma_plane=0.0, dead_value=0.0,
                    base=None, return_flags=False, device=0):
    """Values gathered for the cells subsample_hits() picks, carried to every pixel by a tent filter guided by the
    full-resolution records (include/rt_capi_upsample.h, rt_upsample_guided): hits HIT_DTYPE (Wn, H); lo float32 (Wl, Hl) -- one
    channel, AO's plane -- or (Wl, Hl, 3); base None or float32 of the result's shape that the result is added to -> float32
    (Wn, H) or (Wn, H, 3), and with return_flags also bool (Wn, H): the holes, pixels none of whose four cells lies on their
    surface, filled by the unguided tent.  A tap counts only from the pixel's own object (with match_color: its own albedo
    bits), weighted by max(n_p . n_q, 0) ^ (2 ^ normal_squarings) and, with sigma_plane > 0, by the tap's distance from the
    pixel's tangent plane; modulate multiplies by the pixel's own colour; dead_value is the value of a pixel with no surface.
    Runs on GPU `device`; there is no CPU path."""
    hits = _frame_records(hits)
    lo = np.ascontiguousarray(lo, dtype=np.float32)
    s = int(scale)
    channels = 3 if lo.ndim == 3 else 1
    cells = (-(-hits.shape[0] // s), -(-hits.shape[1] // s)) if 2 <= s <= 8 else lo.shape[:2]
    if lo.shape != cells + ((3,) if channels == 3 else ()):
        raise ValueError(f"lo must be {cells} or {cells + (3,)} for hits {hits.shape} at scale {s}, not {lo.shape}")
    shape = hits.shape + ((3,) if channels == 3 else ())
    if base is not None:
        base = np.ascontiguousarray(base, dtype=np.float32)
        if base.shape != shape:
            raise ValueError(f"base must have shape {shape}, not {base.shape}")
    params = upsample_params(s, channels, normal_squarings, match_color, modulate, sigma_plane, dead_value)
    out = np.empty(shape, dtype=np.float32)
    flags = np.zeros(hits.shape, dtype=np.uint8) if return_flags else None
    capi.check(capi.load_library().rt_upsample_guided(int(device), C.byref(params), hits.shape[0], hits.shape[1], hits.ctypes.data,
                                                      lo.ctypes.data, base.ctypes.data if base is not None else None,
                                                      out.ctypes.data, flags.ctypes.data if return_flags else None, None))
    return (out, flags.view(np.bool_)) if return_flags else out


def temporal_params(channels=3, match_color=False, max_history=32, normal_cos=0.9, plane_eps=0.05, alpha=0.0, alpha_moments=0.0):
    """temporal_accumulate's keywords -> an RtTemporalParams (include/rt_temporal.h); the library checks the values."""
    return capi.RtTemporalParams(int(channels), int(match_color), int(max_history), float(normal_cos), float(plane_eps),
                                 float(alpha), float(alpha_moments))


def _camera_ptr(camera):
    """None, an RtCameraDesc or a pointer to one -> what ctypes passes for a const rt_camera_desc *"""
    return C.byref(camera) if isinstance(camera, capi.RtCameraDesc) else camera


def temporal_accumulate(cur, hits, camera, prev=None, x0=0, W=None, device=0, **params):
    """One frame blended into the accumulated history of the frame before (include/rt_temporal.h, rt_temporal_accumulate):
    cur float32 (Wn, H) -- one channel -- or (Wn, H, 3) and hits HIT_DTYPE (Wn, H), columns [x0, x0 + Wn) of a W x H frame seen by
    `camera` (an RtCameraDesc); prev None -- the first frame -- or (camera, hits, value, moments, length) of the WHOLE previous
    frame: its camera, its records (W, H) and what this call returned for it.  -> (value of cur's shape, moments float32
    (Wn, H, 2), length float32 (Wn, H), variance float32 (Wn, H), flags bool (Wn, H): the pixels without history).  params:
    temporal_params()'s keywords but channels, which cur's shape gives.  Runs on GPU `device`; there is no CPU path."""
    return _accumulate(None, cur, hits, camera, prev, x0, W, device, params)


def _motion_table(motions):
    """None or a float32 (n, 12) array -> (the C-contiguous array or None, n)"""
    if motions is None:
        return None, 0
    table = np.ascontiguousarray(motions, dtype=np.float32)
    if table.ndim != 2 or table.shape[1] != 12:
        raise ValueError(f"motions must be (n, 12), not {table.shape}")
    return table, table.shape[0]


def motion_accumulate(cur, hits, camera, prev=None, motions=None, x0=0, W=None, device=0, **params):
    """temporal_accumulate() for a scene whose objects move (include/rt_motion.h, rt_motion_accumulate): motions None or float32
    (n, 12), row o the rigid motion -- rows {m0 m1 m2 | m3}, {m4 .. m7}, {m8 .. m11} -- that carries a point of Scene object o in
    this frame to where it was in the previous one (object_motions() makes the table from two poses).  A record whose object
    has no row, or the identity's bits, is treated as temporal_accumulate() treats it.  Arguments, result and params are
    temporal_accumulate()'s.  Runs on GPU `device`; there is no CPU path."""
    return _accumulate(_motion_table(motions), cur, hits, camera, prev, x0, W, device, params)


def _accumulate(table, cur, hits, camera, prev, x0, W, device, params):
    """temporal_accumulate() (table None) and motion_accumulate() (table (array or None, n))"""
    hits = _frame_records(hits)
    cur = np.ascontiguousarray(cur, dtype=np.float32)
    channels = 3 if cur.ndim == 3 else 1
    Wn, H = hits.shape
    if cur.shape != hits.shape + ((3,) if channels == 3 else ()):
        raise ValueError(f"cur must be {hits.shape} or {hits.shape + (3,)}, not {cur.shape}")
    pr = temporal_params(channels, **params)
    ptr = [None] * 4
    cam_prev = None
    if prev is not None:
        cam_prev, prev_hits, value, moments, length = prev
        prev_hits = _frame_records(prev_hits)
        W = prev_hits.shape[0] if W is None else int(W)
        shapes = ((W, H), (W, H) + ((3,) if channels == 3 else ()), (W, H, 2), (W, H))
        kept = [prev_hits] + [np.ascontiguousarray(a, dtype=np.float32) for a in (value, moments, length)]
        for a, shape, name in zip(kept, shapes, ("hits", "value", "moments", "length")):
            if a.shape != shape:
                raise ValueError(f"the previous frame's {name} must have shape {shape}, not {a.shape}")
        ptr = [a.ctypes.data for a in kept]
    W = int(x0) + Wn if W is None else int(W)
    out = np.empty(cur.shape, dtype=np.float32)
    out_moments, out_len = np.empty((Wn, H, 2), dtype=np.float32), np.empty((Wn, H), dtype=np.float32)
    variance, flags = np.empty((Wn, H), dtype=np.float32), np.empty((Wn, H), dtype=np.uint8)
    lib = capi.load_library()
    head = (int(device), C.byref(pr), _camera_ptr(cam_prev), _camera_ptr(camera), W, H, int(x0), int(x0) + Wn)
    tail = (cur.ctypes.data, hits.ctypes.data, *ptr, out.ctypes.data, out_moments.ctypes.data, out_len.ctypes.data,
            variance.ctypes.data, flags.ctypes.data, None)
    if table is None:
        capi.check(lib.rt_temporal_accumulate(*head, *tail))
    else:
        capi.check(lib.rt_motion_accumulate(*head, table[0].ctypes.data if table[0] is not None else None, table[1], *tail))
    return out, out_moments, out_len, variance, flags.view(np.bool_)


_IDENTITY_MOTION = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32)


def object_motions(desc_prev, desc_cur):
    """The motion table between two poses of the same object list (include/rt_motion.h), given as two HostScene.desc (pointers
    to, or instances of, RtSceneDesc) -> float32 (n_objects, 12), what motion_accumulate() takes for a frame of desc_cur whose
    previous frame was desc_prev's.  A sphere gets the identity matrix and t = origin_prev - origin_cur in fp32.  A plane gets
    R = F_prev F_cur^T, F the columns (horizontal, vertical, normal), and t = o_prev - R o_cur with o the plane_origin of a
    finite plane and the origin of an infinite one, computed in float64 and rounded once.  An object whose geometry words are
    equal as bits in both poses gets the identity's bits, so it is static.  ValueError if the counts or kinds differ.  A
    convenience: the table it makes is as exact as fp32 allows, and outside the bit-exact definition."""
    prev = desc_prev.contents if hasattr(desc_prev, "contents") else desc_prev
    cur = desc_cur.contents if hasattr(desc_cur, "contents") else desc_cur
    n = int(cur.n_objects)
    if int(prev.n_objects) != n:
        raise ValueError(f"the poses have {int(prev.n_objects)} and {n} objects")
    geometry = ("origin", "radius", "radius_squared", "plane_origin", "normal", "vertical", "horizontal", "reverse_normal",
                "v_distance", "h_distance", "distance_to_origin")
    words = lambda o: b"".join(bytes(memoryview(np.array(getattr(o, k), dtype=np.float32))) for k in geometry)
    vec = lambda v: np.array(list(v), dtype=np.float32)
    out = np.tile(_IDENTITY_MOTION, (n, 1))
    for k in range(n):
        a, b = prev.objects[k], cur.objects[k]
        if a.kind != b.kind:
            raise ValueError(f"object {k} is of kind {a.kind} in one pose and {b.kind} in the other")
        if words(a) == words(b):
            continue
        if a.kind == 0:                                                 # a sphere: a translation
            out[k, 3::4] = vec(a.origin) - vec(b.origin)
            continue
        frame = lambda o: np.stack([vec(o.horizontal), vec(o.vertical), vec(o.normal)], axis=1).astype(np.float64)
        R = frame(a) @ frame(b).T
        where = (lambda o: vec(o.plane_origin)) if a.kind == 2 else (lambda o: vec(o.origin))
        t = where(a).astype(np.float64) - R @ where(b).astype(np.float64)
        out[k] = np.concatenate([R, t[:, None]], axis=1).reshape(12).astype(np.float32)
    return out


class TemporalHistory:
    """The accumulated history of a W x H frame sequence on GPU `device` (include/rt_temporal.h): two ping-pong sets of device
    buffers (records, value, moments, length) owned through torch, the previous frame's camera, and rt_temporal_accumulate_device
    between them.  params: temporal_params()'s keywords but channels.  The process must have imported torch before the library
    was loaded."""

    def __init__(self, W, H, channels=3, device=0, **params):
        import torch
        self.W, self.H, self.channels, self._device = int(W), int(H), int(channels), int(device)
        self._params = temporal_params(channels, **params)
        self._lib = capi.load_library()
        if self.channels not in (1, 3) or self.W <= 0 or self.H <= 0:    # (refused by the call itself, before any allocation)
            capi.check(self._lib.rt_temporal_accumulate_device(self._device, C.byref(self._params), None, None, self.W, self.H, 0,
                                                               self.W, *([None] * 12)))
            raise ValueError("channels must be 1 or 3")
        n = self.W * self.H
        with torch.cuda.device(self._device):
            new = lambda words, dtype: torch.empty((words,), dtype=dtype, device="cuda")
            self._sets = [dict(hits=new(n * 12, torch.int32), value=new(n * self.channels, torch.float32),
                               moments=new(n * 2, torch.float32), length=new(n, torch.float32)) for _ in range(2)]
            self._variance, self._flags = new(n, torch.float32), new(n, torch.uint8)
        self._filtered = self._scratch = None                          # filter_device()'s outputs and scratch, made on first use
        self.clamp_flags = None                                        # push_device(clamp=...)'s byte plane, made on first use
        self.gradient_lambda = self.gradient_flags = None              # push_device(gradient=...)'s planes, made on first use
        self.reset()

    def reset(self):
        """forget the history: the next frame is a first frame"""
        self.frames, self._next_column, self._cam_prev, self._cam, self._motions = 0, 0, None, None, None

    def _copy_camera(self, camera):
        cam = capi.RtCameraDesc()
        C.memmove(C.byref(cam), _camera_ptr(camera), C.sizeof(cam))
        return cam

    def push_device(self, value, hits, camera, x0=0, x1=None, stream=None, motions=None, clamp=None, gradient=None):
        """push() of torch tensors on the device (float32 value, the records as 12 int32 words each), enqueued on `stream` (the
        current one by default) without a host wait -> the strip's (value, variance, flags) as views of this history's buffers,
        valid until the next frame's push.  motions: None, a float32 (n, 12) numpy table, which is uploaded, or a float32 device
        tensor of 12 n words, used as it is and kept alive until the next push (include/rt_motion.h).  clamp: None, or a dict of
        clamp_params()'s keywords (but channels): the strip just written is clipped to this frame's neighbourhood in place in
        this history's own set, on the same stream (include/rt_clamp.h, rt_history_clamp_device) -- the returned value and
        variance are then the clamped ones, what history_clamp() of the accumulated strip gives bit for bit, and clamp_flags
        (uint8, W * H) holds the strip's clamp flags.  gradient: None, or a dict of now_lo, then_lo, lo_hits and optionally
        then_hits -- device tensors: the STRIP's cell frames and their records (include/rt_gradient.h; float32, and the records
        as 12 int32 words each) -- plus gradient_params()'s keywords (but channels): the strip just written is re-blended by its
        temporal gradient in place in this history's own set, on the same stream (rt_gradient_reweight_device), after the
        accumulate call and before the clamp -- the returned value and variance are then what gradient_reweight() of the
        accumulated strip gives bit for bit (followed by history_clamp() with clamp), and gradient_lambda (float32, W * H) and
        gradient_flags (uint8, W * H) hold the strip's weights and flags."""
        import torch
        W, H, ch = self.W, self.H, self.channels
        x0, x1 = int(x0), W if x1 is None else int(x1)
        clamp = None if clamp is None else clamp_params(ch, **clamp)
        if gradient is not None:
            gradient = dict(gradient)
            cells = [gradient.pop(k) for k in ("now_lo", "then_lo", "lo_hits")] + [gradient.pop("then_hits", None)]
            gradient = gradient_params(ch, **gradient)
        if x0 != self._next_column or not x0 < x1 <= W:
            raise ValueError(f"a frame's strips are pushed in ascending order: expected a strip from column {self._next_column}")
        n = (x1 - x0) * H
        if value.numel() != n * ch or hits.numel() * hits.element_size() != n * 48:
            raise ValueError(f"columns {x0}:{x1} need {n * ch} values and {n} records")
        if clamp is not None:
            # the clamp's parameters are refused before anything is enqueued: the call without buffers, whose last check is theirs
            rc = self._lib.rt_history_clamp_device(self._device, C.byref(clamp), x1 - x0, H, *([None] * 11))
            if b"is NULL" not in self._lib.rt_last_error():
                capi.check(rc)
        if gradient is not None:
            # likewise the gradient's parameters, and the cell buffers' sizes
            rc = self._lib.rt_gradient_reweight_device(self._device, C.byref(gradient), x1 - x0, H, *([None] * 16))
            if b"is NULL" not in self._lib.rt_last_error():
                capi.check(rc)
            s = gradient.scale
            n_lo = ((x1 - x0 + s - 1) // s) * ((H + s - 1) // s)
            if any(t.numel() != n_lo * ch for t in cells[:2]) or \
                    any(t is not None and t.numel() * t.element_size() != n_lo * 48 for t in cells[2:]):
                raise ValueError(f"columns {x0}:{x1} at scale {s} need {n_lo * ch} cell values and {n_lo} cell records")
        if x0 == 0:
            self._cam = self._copy_camera(camera)
        old, new = self._sets[self.frames % 2], self._sets[(self.frames + 1) % 2]
        first = self.frames == 0
        prev = [None] * 4 if first else [old[k].data_ptr() for k in ("hits", "value", "moments", "length")]
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream() if stream is None else stream
            part = lambda t, words: t[x0 * H * words:x1 * H * words]
            with torch.cuda.stream(stream):
                part(new["hits"], 12).copy_(hits.reshape(-1).view(torch.int32))      # next frame's previous records
            out = [part(new["value"], ch), part(new["moments"], 2), part(new["length"], 1), part(self._variance, 1),
                   part(self._flags, 1)]
            head = (self._device, C.byref(self._params), None if first else C.byref(self._cam_prev), C.byref(self._cam), W, H, x0, x1)
            tail = (value.data_ptr(), part(new["hits"], 12).data_ptr(), *prev, *[t.data_ptr() for t in out], stream.cuda_stream)
            if motions is None:
                capi.check(self._lib.rt_temporal_accumulate_device(*head, *tail))
            else:
                if not isinstance(motions, torch.Tensor):
                    with torch.cuda.stream(stream):
                        motions = torch.tensor(_motion_table(motions)[0].reshape(-1), device="cuda")
                if motions.dtype != torch.float32 or motions.numel() % 12 or not motions.is_contiguous():
                    raise ValueError("a device motion table is a contiguous float32 tensor of 12 n words")
                self._motions = motions                                 # (alive while the launch may read it)
                capi.check(self._lib.rt_motion_accumulate_device(*head, motions.data_ptr() if motions.numel() else None,
                                                                 motions.numel() // 12, *tail))
            if gradient is not None:
                if self.gradient_lambda is None:
                    with torch.cuda.stream(stream):                     # (the fills are ordered before the call's stores)
                        self.gradient_lambda = torch.zeros((W * H,), dtype=torch.float32, device="cuda")
                        self.gradient_flags = torch.zeros((W * H,), dtype=torch.uint8, device="cuda")
                in_place = [t.data_ptr() for t in out[:3]]
                capi.check(self._lib.rt_gradient_reweight_device(
                    self._device, C.byref(gradient), x1 - x0, H, value.data_ptr(), part(new["hits"], 12).data_ptr(), *in_place,
                    *[None if t is None else t.data_ptr() for t in cells], *in_place, out[3].data_ptr(),
                    part(self.gradient_lambda, 1).data_ptr(), part(self.gradient_flags, 1).data_ptr(), stream.cuda_stream))
                self._cells = cells                                     # (alive while the launch may read them)
            if clamp is not None:
                if self.clamp_flags is None:
                    with torch.cuda.stream(stream):                     # (the fill is ordered before the clamp's stores)
                        self.clamp_flags = torch.zeros((W * H,), dtype=torch.uint8, device="cuda")
                in_place = [t.data_ptr() for t in out[:3]]
                capi.check(self._lib.rt_history_clamp_device(self._device, C.byref(clamp), x1 - x0, H, value.data_ptr(),
                                                             part(new["hits"], 12).data_ptr(), *in_place, *in_place,
                                                             out[3].data_ptr(), part(self.clamp_flags, 1).data_ptr(),
                                                             stream.cuda_stream))
        self._next_column = x1
        if x1 == W:                                                     # the frame is whole: swap the sets
            self.frames, self._next_column, self._cam_prev = self.frames + 1, 0, self._cam
        return out[0], out[3], out[4]

    def push(self, rgb, hits, camera, x0=0, x1=None, motions=None, clamp=None, gradient=None):
        """Columns [x0, x1) of the next frame, seen by `camera`: rgb float32 (Wn, H) or (Wn, H, 3) by this history's channels,
        hits HIT_DTYPE (Wn, H) -> (value of rgb's shape, variance float32 (Wn, H), flags bool (Wn, H)), temporal_accumulate()'s
        bit for bit -- with motions (push_device()'s), motion_accumulate()'s; with clamp (push_device()'s), value and variance
        are history_clamp()'s of those; with gradient (push_device()'s, its now_lo, then_lo, lo_hits and then_hits being arrays:
        float32 (Wl, Hl[, 3]) and HIT_DTYPE (Wl, Hl)), gradient_reweight() comes between the two.  A frame's strips are pushed in
        ascending order from column 0; the strip that ends at W completes the frame and swaps the two sets."""
        import torch
        hits = _frame_records(hits)
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        shape = hits.shape + ((3,) if self.channels == 3 else ())
        if rgb.shape != shape:
            raise ValueError(f"rgb must have shape {shape}, not {rgb.shape}")
        with torch.cuda.device(self._device):
            d_rgb = torch.tensor(rgb.reshape(-1), device="cuda")
            d_hits = torch.tensor(hits.reshape(-1).view(np.int32), device="cuda")      # (a copy: the caller's may be read-only)
            if gradient is not None:
                gradient = dict(gradient)
                for k in ("now_lo", "then_lo"):
                    gradient[k] = torch.tensor(np.ascontiguousarray(gradient[k], dtype=np.float32).reshape(-1), device="cuda")
                for k in ("lo_hits", "then_hits"):
                    if gradient.get(k) is not None:
                        gradient[k] = torch.tensor(_frame_records(gradient[k]).reshape(-1).view(np.int32), device="cuda")
            value, variance, flags = self.push_device(d_rgb, d_hits, camera, x0, x1, motions=motions, clamp=clamp,
                                                      gradient=gradient)
            return (value.cpu().numpy().reshape(shape), variance.cpu().numpy().reshape(hits.shape),
                    flags.cpu().numpy().reshape(hits.shape).view(np.bool_))

    def filter_device(self, stream=None, **params):
        """The last completed frame through the variance-steered filter (include/rt_svgf.h, rt_svgf_filter_device), read from
        this history's own buffers and enqueued on `stream` (the current one by default) without a host wait -> the filtered
        (value, variance) as tensors this history owns, valid until the next filter_device().  params: svgf_params()'s keywords
        but channels.  The history itself is left untouched: the next push blends into the unfiltered frame."""
        import torch
        if self.frames == 0:
            raise ValueError("no completed frame to filter")
        pr = svgf_params(self.channels, **params)
        W, H, n = self.W, self.H, self.W * self.H
        need = int(self._lib.rt_svgf_scratch_bytes(C.byref(pr), W, H))
        s = self._sets[self.frames % 2]
        with torch.cuda.device(self._device):
            stream = torch.cuda.current_stream() if stream is None else stream
            if self._filtered is None:
                self._filtered = (torch.empty((n * self.channels,), dtype=torch.float32, device="cuda"),
                                  torch.empty((n,), dtype=torch.float32, device="cuda"))
            if need and (self._scratch is None or self._scratch.numel() < need):
                self._scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
            scratch = self._scratch.data_ptr() if need else None       # (refused arguments: the call itself says why)
            capi.check(self._lib.rt_svgf_filter_device(self._device, C.byref(pr), W, H, s["value"].data_ptr(), s["hits"].data_ptr(),
                                                       s["moments"].data_ptr(), s["length"].data_ptr(),
                                                       self._filtered[0].data_ptr(), self._filtered[1].data_ptr(), None, scratch,
                                                       stream.cuda_stream))
        return self._filtered

    def state(self):
        """-> (camera, hits, value, moments, length) of the last whole frame on the host, what temporal_accumulate() takes as prev;
        None before the first"""
        if self.frames == 0:
            return None
        s, W, H = self._sets[self.frames % 2], self.W, self.H
        return (self._cam_prev, s["hits"].cpu().numpy().view(HIT_DTYPE).reshape(W, H),
                s["value"].cpu().numpy().reshape((W, H, 3) if self.channels == 3 else (W, H)),
                s["moments"].cpu().numpy().reshape(W, H, 2), s["length"].cpu().numpy().reshape(W, H))


def svgf_params(channels=3, iterations=4, sigma_l=2.0, min_history=4, spatial_radius=3, normal_squarings=3, match_color=True,
                sigma_plane=0.0, epsilon=1e-8):
    """svgf_filter's keywords -> an RtSvgfParams (include/rt_svgf.h); the library checks the values."""
    return capi.RtSvgfParams(int(channels), int(iterations), int(normal_squarings), int(match_color), int(min_history),
                             int(spatial_radius), float(sigma_l), float(sigma_plane), float(epsilon))


def svgf_filter(value, hits, moments, length, device=0, **params):
    """The variance-steered filter over an accumulated frame (include/rt_svgf.h, rt_svgf_filter): value float32 (Wn, H) -- one
    channel -- or (Wn, H, 3), hits HIT_DTYPE (Wn, H), moments float32 (Wn, H, 2) and length float32 (Wn, H), as
    temporal_accumulate() returns them (a whole frame or a strip) -> (the filtered value of value's shape, its variance float32
    (Wn, H), the variance estimate the first iteration read, float32 (Wn, H)).  params: svgf_params()'s keywords but channels,
    which value's shape gives.  Runs on GPU `device`; there is no CPU path."""
    hits = _frame_records(hits)
    value = np.ascontiguousarray(value, dtype=np.float32)
    moments = np.ascontiguousarray(moments, dtype=np.float32)
    length = np.ascontiguousarray(length, dtype=np.float32)
    channels = 3 if value.ndim == 3 else 1
    Wn, H = hits.shape
    if value.shape != hits.shape + ((3,) if channels == 3 else ()):
        raise ValueError(f"value must be {hits.shape} or {hits.shape + (3,)}, not {value.shape}")
    if moments.shape != (Wn, H, 2) or length.shape != (Wn, H):
        raise ValueError(f"moments must be {(Wn, H, 2)} and length {(Wn, H)}, not {moments.shape} and {length.shape}")
    pr = svgf_params(channels, **params)
    out = np.empty(value.shape, dtype=np.float32)
    variance, estimate = np.empty((Wn, H), dtype=np.float32), np.empty((Wn, H), dtype=np.float32)
    capi.check(capi.load_library().rt_svgf_filter(int(device), C.byref(pr), Wn, H, value.ctypes.data, hits.ctypes.data,
                                                  moments.ctypes.data, length.ctypes.data, out.ctypes.data, variance.ctypes.data,
                                                  estimate.ctypes.data, None))
    return out, variance, estimate


def clamp_params(channels=3, box=0, radius=1, match_color=True, min_taps=3, clip_history=4, normal_cos=0.9, gamma=1.0):
    """history_clamp's keywords -> an RtClampParams (include/rt_clamp.h); the library checks the values."""
    return capi.RtClampParams(int(channels), int(box), int(radius), int(match_color), int(min_taps), int(clip_history),
                              float(normal_cos), float(gamma))


def history_clamp(cur, hits, value, moments, length, device=0, **params):
    """An accumulated frame clipped to this frame's neighbourhood (include/rt_clamp.h, rt_history_clamp): cur float32 (Wn, H) --
    one channel -- or (Wn, H, 3) and hits HIT_DTYPE (Wn, H), what temporal_accumulate() or motion_accumulate() was given for the
    frame (a whole frame or a strip); value of cur's shape, moments float32 (Wn, H, 2) and length float32 (Wn, H), what it
    returned -> (value, moments, length, variance float32 (Wn, H), flags uint8 (Wn, H): 1 clipped, 2 left alone for fewer than
    min_taps taps).  Where a pixel's value lies outside the box of the samples on its surface around it -- box 0: their
    extremes, box 1: mean -/+ gamma standard deviations -- it is moved onto the box, its length cut to clip_history and its
    moments shifted.  params: clamp_params()'s keywords but channels, which cur's shape gives.  Runs on GPU `device`; there is no
    CPU path."""
    hits = _frame_records(hits)
    cur, value = np.ascontiguousarray(cur, dtype=np.float32), np.ascontiguousarray(value, dtype=np.float32)
    moments, length = np.ascontiguousarray(moments, dtype=np.float32), np.ascontiguousarray(length, dtype=np.float32)
    channels = 3 if cur.ndim == 3 else 1
    Wn, H = hits.shape
    if cur.shape != hits.shape + ((3,) if channels == 3 else ()) or value.shape != cur.shape:
        raise ValueError(f"cur and value must be {hits.shape} or {hits.shape + (3,)}, not {cur.shape} and {value.shape}")
    if moments.shape != (Wn, H, 2) or length.shape != (Wn, H):
        raise ValueError(f"moments must be {(Wn, H, 2)} and length {(Wn, H)}, not {moments.shape} and {length.shape}")
    pr = clamp_params(channels, **params)
    out, out_moments, out_len = np.empty(cur.shape, dtype=np.float32), np.empty((Wn, H, 2), dtype=np.float32), \
        np.empty((Wn, H), dtype=np.float32)
    variance, flags = np.empty((Wn, H), dtype=np.float32), np.empty((Wn, H), dtype=np.uint8)
    capi.check(capi.load_library().rt_history_clamp(int(device), C.byref(pr), Wn, H, cur.ctypes.data, hits.ctypes.data,
                                                    value.ctypes.data, moments.ctypes.data, length.ctypes.data, out.ctypes.data,
                                                    out_moments.ctypes.data, out_len.ctypes.data, variance.ctypes.data,
                                                    flags.ctypes.data, None))
    return out, out_moments, out_len, variance, flags


def gradient_params(channels=3, scale=2, radius=1, match_color=True, normal_cos=0.9, gain=2.0, lambda_min=0.0, den_floor=1e-6):
    """gradient_reweight's keywords -> an RtGradientParams (include/rt_gradient.h); the library checks the values."""
    return capi.RtGradientParams(int(channels), int(scale), int(radius), int(match_color), float(normal_cos), float(gain),
                                 float(lambda_min), float(den_floor))


def gradient_reweight(cur, hits, value, moments, length, now_lo, then_lo, lo_hits, then_hits=None, device=0, **params):
    """An accumulated frame re-blended by its temporal gradient (include/rt_gradient.h, rt_gradient_reweight): cur float32
    (Wn, H) -- one channel -- or (Wn, H, 3) and hits HIT_DTYPE (Wn, H), what temporal_accumulate() or motion_accumulate() was given
    for the frame (a whole frame or a strip); value of cur's shape, moments float32 (Wn, H, 2) and length float32 (Wn, H), what
    it returned; now_lo and then_lo float32 (Wl, Hl) or (Wl, Hl, 3), Wl = ceil(Wn / scale) and Hl = ceil(H / scale): the term at
    every scale-th pixel in this frame's scene and in the previous frame's, shaded with the same random numbers; lo_hits HIT_DTYPE
    (Wl, Hl), the records now_lo was made from, and then_hits, None or those then_lo was made from -> (value, moments, length,
    variance float32 (Wn, H), lam float32 (Wn, H), flags uint8 (Wn, H): 1 re-blended, 2 left alone for no counted cell, 3
    restarted).  params: gradient_params()'s keywords but channels, which cur's shape gives.  Runs on GPU `device`; there is no
    CPU path."""
    hits, lo_hits = _frame_records(hits), _frame_records(lo_hits)
    then_hits = None if then_hits is None else _frame_records(then_hits)
    cur, value = np.ascontiguousarray(cur, dtype=np.float32), np.ascontiguousarray(value, dtype=np.float32)
    moments, length = np.ascontiguousarray(moments, dtype=np.float32), np.ascontiguousarray(length, dtype=np.float32)
    now_lo, then_lo = np.ascontiguousarray(now_lo, dtype=np.float32), np.ascontiguousarray(then_lo, dtype=np.float32)
    channels = 3 if cur.ndim == 3 else 1
    tail = (3,) if channels == 3 else ()
    Wn, H = hits.shape
    if cur.shape != hits.shape + tail or value.shape != cur.shape:
        raise ValueError(f"cur and value must be {hits.shape} or {hits.shape + (3,)}, not {cur.shape} and {value.shape}")
    if moments.shape != (Wn, H, 2) or length.shape != (Wn, H):
        raise ValueError(f"moments must be {(Wn, H, 2)} and length {(Wn, H)}, not {moments.shape} and {length.shape}")
    pr = gradient_params(channels, **params)
    s = pr.scale
    lo = (-(-Wn // s), -(-H // s)) if 2 <= s <= 8 else lo_hits.shape      # (a refused scale: the library says so)
    if lo_hits.shape != lo or now_lo.shape != lo + tail or then_lo.shape != lo + tail or \
            (then_hits is not None and then_hits.shape != lo):
        raise ValueError(f"at scale {s} the cell frames must be {lo + tail} and their records {lo}")
    out, out_moments, out_len = np.empty(cur.shape, dtype=np.float32), np.empty((Wn, H, 2), dtype=np.float32), \
        np.empty((Wn, H), dtype=np.float32)
    variance, lam, flags = np.empty((Wn, H), dtype=np.float32), np.empty((Wn, H), dtype=np.float32), np.empty((Wn, H), dtype=np.uint8)
    capi.check(capi.load_library().rt_gradient_reweight(
        int(device), C.byref(pr), Wn, H, cur.ctypes.data, hits.ctypes.data, value.ctypes.data, moments.ctypes.data,
        length.ctypes.data, now_lo.ctypes.data, then_lo.ctypes.data, lo_hits.ctypes.data,
        None if then_hits is None else then_hits.ctypes.data, out.ctypes.data, out_moments.ctypes.data, out_len.ctypes.data,
        variance.ctypes.data, lam.ctypes.data, flags.ctypes.data, None))
    return out, out_moments, out_len, variance, lam, flags


_TRANSFERS = {"srgb": capi.RT_TRANSFER_SRGB, "linear": capi.RT_TRANSFER_LINEAR, "custom": capi.RT_TRANSFER_CUSTOM}


def image_params(channels=3, exposure=1.0, transfer="srgb", bottom_up=False, thresholds=None):
    """encode_image's keywords -> (an RtImageParams, the float32 array its thresholds point into or None: keep it alive with the
    struct).  thresholds (255 floats T[1..255]) selects RT_TRANSFER_CUSTOM whatever transfer says."""
    table = None
    if thresholds is not None:
        table = np.ascontiguousarray(thresholds, dtype=np.float32)
        if table.shape != (255,):
            raise ValueError(f"thresholds must be 255 floats, not {table.shape}")
        transfer = "custom"
    if transfer not in _TRANSFERS:
        raise ValueError(f"transfer must be one of {sorted(_TRANSFERS)}, not {transfer!r}")
    params = capi.RtImageParams(int(channels), int(bool(bottom_up)), _TRANSFERS[transfer], float(exposure),
                                table.ctypes.data_as(C.POINTER(C.c_float)) if table is not None else None)
    return params, table


def encode_image(rgb, channels=3, exposure=1.0, transfer="srgb", bottom_up=False, thresholds=None, device=0):
    """A frame's colours as 8-bit scanlines (include/rt_capi_image.h, rt_encode_image): rgb float32 (Wn, H, 3) as render() returns
    it, a whole frame or a strip -> uint8 (H, Wn, channels), row 0 the top of the picture (z = H - 1) unless bottom_up; channel 3,
    if any, is 255.  transfer "srgb" or "linear", or thresholds: 255 floats T[1..255], code = the number of T[k] <= rgb * exposure.
    Runs on GPU `device`; there is no CPU path."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"rgb must be (Wn, H, 3), not {rgb.shape}")
    params, table = image_params(channels, exposure, transfer, bottom_up, thresholds)
    Wn, H = rgb.shape[:2]
    out = np.empty((H, Wn, params.channels if params.channels in (3, 4) else 3), dtype=np.uint8)
    capi.check(capi.load_library().rt_encode_image(int(device), C.byref(params), Wn, H, rgb.ctypes.data, out.ctypes.data,
                                                   Wn * out.shape[2], None))
    return out


class Renderer:
    """Owns an ``rt_scene`` (device tables for one HostScene on one GPU)."""

    _CREATE = ("rt_scene_create", "rt_scene_create_textured", "rt_scene_create_refractive", "rt_scene_create_soft")

    def __init__(self, host_scene, device=0):
        self._host = host_scene          # keeps the desc arrays alive
        # the scene's Texture_Image objects (include/rt_capi_texture.h), its refractive materials (include/rt_capi_refract.h)
        # and its area lights (include/rt_capi_soft.h): the plainest entry point that carries what it has
        images, refr, soft = host_scene.images, host_scene.refractions, host_scene.area_lights
        self._create(host_scene.desc, device, images, refr, soft, 3 if soft[0] else 2 if refr[0] else 1 if images[0] else 0)
        self._cam = host_scene.camera

    def _create(self, desc, device, images, refractive, area_lights, entry):
        """The scene of the description at pointer desc by entry point _CREATE[entry], which takes the first `entry` of the
        three (count, array or None) pairs.  (A plain scene must call rt_scene_create: TCRT_LIBRARY may name an older build
        that has nothing else, capi.py.)"""
        self._lib = capi.load_library()
        self._scene = C.c_void_p()
        self._device = device
        lists = (*images, *refractive, *area_lights)[:2 * entry]
        capi.check(getattr(self._lib, self._CREATE[entry])(desc, *lists, device, C.byref(self._scene)))

    @classmethod
    def from_desc(cls, desc, camera, device=0, keepalive=None, images=None, refractive=None, area_lights=None):
        """Build from raw RtSceneDesc / RtCameraDesc (tests with hand-made tables).  images (include/rt_capi_texture.h): a
        list of (texels, width, height, wrap) -- texels a float32 (texels_h, texels_w, 3) array, texels[j, i] texel (i, j),
        width / height the world size of one copy, wrap RT_TEX_WRAP_* -- that texture indices n_textures + k name.  With
        images (even an empty list) the scene is made by rt_scene_create_textured, else by rt_scene_create.  refractive
        (include/rt_capi_refract.h): a list of (object, tf, ior); with it (even an empty list) the scene is made by
        rt_scene_create_refractive, with the images if any.  area_lights (include/rt_capi_soft.h): a list of (object,
        samples, radius); with it (even an empty list) the scene is made by rt_scene_create_soft, with the images and the
        refractive objects if any."""
        self = cls.__new__(cls)
        self._host = keepalive
        given = (images, refractive, area_lights)
        arrays, descs = image_descs(images or [])
        made = (descs, refraction_descs(refractive or []), area_light_descs(area_lights or []))
        self._images = (arrays,) + made            # the texels stay alive with the scene (the library copies them too)
        pairs = [(len(g or []), m if g else None) for g, m in zip(given, made)]       # (an empty list: count 0, no array)
        entry = max(k + 1 if g is not None else 0 for k, g in enumerate(given))      # the last list that is given, even empty
        self._create(C.byref(desc), device, *pairs, entry)
        self._cam = C.pointer(camera)
        return self

    def close(self):
        if getattr(self, "_scene", None):
            self._lib.rt_scene_destroy(self._scene)
            self._scene = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_shadow_seed(self, seed):
        """the sampling seed of this scene's later launches (include/rt_capi_soft.h; 0 by default)"""
        capi.check(self._lib.rt_scene_set_shadow_seed(self._scene, C.c_uint32(int(seed) & 0xFFFFFFFF)))

    def set_option(self, key, value):
        capi.check(self._lib.rt_set_option(self._scene, key.encode(), int(value)))

    def render(self, W, H, max_depth, x0=0, x1=None):
        """Columns [x0, x1) of a W x H image -> float32 array (x1-x0, H, 3)."""
        x1 = W if x1 is None else x1
        out = np.empty((max(x1 - x0, 0), H, 3), dtype=np.float32)
        capi.check(self._lib.rt_render(self._scene, self._cam, W, H, x0, x1, max_depth,
                                       out.ctypes.data))
        return out

    def render_device(self, W, H, max_depth, x0, x1, device_ptr, stream=0):
        """Enqueue a render into device memory on a HIP stream (no sync)."""
        capi.check(self._lib.rt_render_device(self._scene, self._cam, W, H, x0, x1, max_depth,
                                              C.c_void_p(device_ptr), C.c_void_p(stream)))

    def render_ssaa(self, W, H, max_depth, samples, x0=0, x1=None):
        """Columns [x0, x1) of a W x H image with samples x samples samples per pixel, box-filtered in the render kernel
        (include/rt_capi_ssaa.h; samples 1, 2 or 4) -> float32 array (x1-x0, H, 3)."""
        x1 = W if x1 is None else x1
        out = np.empty((max(x1 - x0, 0), H, 3), dtype=np.float32)
        capi.check(self._lib.rt_render_ssaa(self._scene, self._cam, W, H, x0, x1, max_depth, samples,
                                            out.ctypes.data))
        return out

    def render_ssaa_device(self, W, H, max_depth, samples, x0, x1, device_ptr, stream=0):
        """Enqueue a supersampled render (W x H output columns [x0, x1)) into device memory on a HIP stream (no sync)."""
        capi.check(self._lib.rt_render_ssaa_device(self._scene, self._cam, W, H, x0, x1, max_depth, samples,
                                                   C.c_void_p(device_ptr), C.c_void_p(stream)))

    def render_gbuffer(self, W, H, max_depth, x0=0, x1=None):
        """Columns [x0, x1) of a W x H image with each pixel's hit record (include/rt_capi_gbuffer.h) -> (rgb float32
        (x1-x0, H, 3), hits HIT_DTYPE (x1-x0, H)): rgb is render()'s, hits[x - x0, z] the rt_hit of the pixel's camera ray
        (object -1 = no hit)."""
        x1 = W if x1 is None else x1
        rgb = np.empty((max(x1 - x0, 0), H, 3), dtype=np.float32)
        hits = np.empty((max(x1 - x0, 0), H), dtype=HIT_DTYPE)
        capi.check(self._lib.rt_render_gbuffer(self._scene, self._cam, W, H, x0, x1, max_depth, rgb.ctypes.data,
                                               hits.ctypes.data))
        return rgb, hits

    def render_gbuffer_device(self, W, H, max_depth, x0, x1, rgb_ptr, hits_ptr, stream=0):
        """Enqueue a G-buffer frame (colours at rgb_ptr, 48-byte records at hits_ptr, 16-byte aligned) into device memory on a
        HIP stream (no sync)."""
        capi.check(self._lib.rt_render_gbuffer_device(self._scene, self._cam, W, H, x0, x1, max_depth, C.c_void_p(rgb_ptr),
                                                      C.c_void_p(hits_ptr), C.c_void_p(stream)))

    def render_adaptive(self, W, H, max_depth, samples=2, color_threshold=1 / 32, normal_cos=0.9, flag_all=False, chunk_pixels=0,
                        x0=0, x1=None, return_flags=False):
        """Columns [x0, x1) of a W x H image, supersampled only where an edge passes (include/rt_capi_adaptive.h): one sample a
        pixel with its hit record first, then samples x samples samples for the pixels adaptive_flags() marks -> float32
        (x1-x0, H, 3), and with return_flags also bool (x1-x0, H).  The frame is where(flags, render_ssaa(..., samples),
        render(...)) bit for bit; chunk_pixels (the most flagged pixels traced per launch, 0: the default) never changes it.
        adaptive_info() tells how many pixels were refined and what each stage cost."""
        x1 = W if x1 is None else x1
        params = adaptive_params(samples, color_threshold, normal_cos, flag_all, chunk_pixels)
        out = np.empty((max(x1 - x0, 0), H, 3), dtype=np.float32)
        flags = np.zeros((max(x1 - x0, 0), H), dtype=np.uint8) if return_flags else None
        capi.check(self._lib.rt_render_adaptive(self._scene, self._cam, W, H, x0, x1, max_depth, C.byref(params), out.ctypes.data,
                                                flags.ctypes.data if return_flags else None))
        return (out, flags.view(np.bool_)) if return_flags else out

    def render_adaptive_device(self, W, H, max_depth, x0, x1, device_ptr, flags_ptr=0, stream=0, samples=2, color_threshold=1 / 32,
                               normal_cos=0.9, flag_all=False, chunk_pixels=0):
        """An adaptive render into device memory on a HIP stream: colours (12 bytes a pixel) at device_ptr, the flags (a byte a
        pixel) at flags_ptr unless that is 0.  The stream is synchronised once, after the flag pass (the host must know how many
        pixels the second pass has), so the call cannot be captured into a graph; the second pass is only enqueued."""
        params = adaptive_params(samples, color_threshold, normal_cos, flag_all, chunk_pixels)
        capi.check(self._lib.rt_render_adaptive_device(self._scene, self._cam, W, H, x0, x1, max_depth, C.byref(params),
                                                       C.c_void_p(device_ptr), C.c_void_p(flags_ptr or None), C.c_void_p(stream)))

    def adaptive_info(self):
        """The last render_adaptive*() of this scene (include/rt_capi_adaptive.h, rt_adaptive_info): pixels, flagged, rays,
        chunks and the four stage times."""
        info = capi.RtAdaptiveInfo()
        capi.check(self._lib.rt_get_adaptive_info(self._scene, C.byref(info)))
        return info

    def render_lens(self, W, H, max_depth, samples=4, aperture=0.0, focus=1.0, seed=0, chunk_columns=0, x0=0, x1=None):
        """Columns [x0, x1) of a W x H image through a thin lens (include/rt_capi_lens.h): samples x samples rays a pixel, each
        from its own point of a lens of radius aperture through the focal plane at focus times the screen's distance, generated,
        traced and averaged on the GPU -> float32 (x1-x0, H, 3).  aperture 0, focus 1 is render_ssaa(..., samples) bit for bit;
        chunk_columns (the most columns traced per launch, 0: the default) never changes the frame.  lens_info() tells what
        each stage cost."""
        x1 = W if x1 is None else x1
        params = lens_params(samples, aperture, focus, seed, chunk_columns)
        out = np.empty((max(x1 - x0, 0), H, 3), dtype=np.float32)
        capi.check(self._lib.rt_render_lens(self._scene, self._cam, W, H, x0, x1, max_depth, C.byref(params), out.ctypes.data))
        return out

    def render_lens_device(self, W, H, max_depth, x0, x1, device_ptr, stream=0, samples=4, aperture=0.0, focus=1.0, seed=0,
                           chunk_columns=0):
        """Enqueue a thin-lens render into device memory (12 bytes a pixel at device_ptr) on a HIP stream (no sync: nothing is
        read back)."""
        params = lens_params(samples, aperture, focus, seed, chunk_columns)
        capi.check(self._lib.rt_render_lens_device(self._scene, self._cam, W, H, x0, x1, max_depth, C.byref(params),
                                                   C.c_void_p(device_ptr), C.c_void_p(stream)))

    def lens_info(self):
        """The last render_lens*() of this scene (include/rt_capi_lens.h, rt_lens_info): pixels, rays, chunks and the three
        stage times."""
        info = capi.RtLensInfo()
        capi.check(self._lib.rt_get_lens_info(self._scene, C.byref(info)))
        return info

    def render_denoised(self, W, H, max_depth, iterations=2, sigma_color=1.0, normal_squarings=3):
        """A W x H G-buffer frame filtered on the GPU where it was rendered (include/rt_capi_denoise.h): rt_render_gbuffer_device
        and rt_denoise_device enqueued on one stream with no host wait between them, then one download -> (rgb float32
        (W, H, 3), the filtered colours; hits HIT_DTYPE (W, H); kernel_ms, device time from the render's start to the filter's
        end).  The result is denoise(*render_gbuffer(W, H, max_depth), ...) bit for bit.  The device buffers, the stream and the
        events are torch's, so the process must have imported torch before the library was loaded."""
        import torch
        device = int(self._device)
        params = capi.RtDenoiseParams(int(iterations), int(normal_squarings), float(sigma_color))
        scratch_bytes = self._lib.rt_denoise_scratch_bytes(C.byref(params), W, H)
        if not scratch_bytes:
            capi.check(self._lib.rt_denoise_device(device, C.byref(params), W, H, None, None, None, None, None))
        with torch.cuda.device(device):
            noisy = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
            clean = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
            records = torch.empty((W * H * 12,), dtype=torch.int32, device="cuda")
            scratch = torch.empty(((scratch_bytes + 15) // 16 * 4,), dtype=torch.int32, device="cuda")
            stream = torch.cuda.current_stream()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record(stream)
            self.render_gbuffer_device(W, H, max_depth, 0, W, noisy.data_ptr(), records.data_ptr(), stream.cuda_stream)
            capi.check(self._lib.rt_denoise_device(device, C.byref(params), W, H, noisy.data_ptr(), records.data_ptr(),
                                                   clean.data_ptr(), scratch.data_ptr(), stream.cuda_stream))
            stop.record(stream)
            host = torch.cat((clean.view(torch.int32).reshape(-1), records)).cpu().numpy()      # the one download
            kernel_ms = start.elapsed_time(stop)
        rgb = host[:W * H * 3].view(np.float32).reshape(W, H, 3)
        hits = host[W * H * 3:].view(HIT_DTYPE).reshape(W, H)
        return rgb, hits, kernel_ms

    def render_image(self, W, H, max_depth, samples=1, channels=3, exposure=1.0, transfer="srgb", bottom_up=False,
                     thresholds=None, lens=None):
        """A W x H frame as 8-bit scanlines, encoded on the GPU where it was rendered (include/rt_capi_image.h): rt_render_device
        -- rt_render_ssaa_device for samples 2 or 4 -- and rt_encode_image_device enqueued on one stream with no host wait between
        them, then a download of the bytes alone -> uint8 (H, W, channels).  The result is encode_image(render(W, H, max_depth),
        ...) bit for bit.  lens: None, or a dict of render_lens_device's keywords (aperture, focus, seed, chunk_columns; samples
        if it names none is this call's): the frame is then rt_render_lens_device's (include/rt_capi_lens.h).  The device
        buffers and the stream are torch's, so the process must have imported torch before the library was loaded
        (INTEGRATION.md section 3)."""
        import torch
        device = int(self._device)
        params, table = image_params(channels, exposure, transfer, bottom_up, thresholds)
        C_ = params.channels if params.channels in (3, 4) else 3        # (a bad count is refused by the call below)
        with torch.cuda.device(device):
            frame = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
            image = torch.empty((H, W, C_), dtype=torch.uint8, device="cuda")
            stream = torch.cuda.current_stream()
            if lens is not None:
                self.render_lens_device(W, H, max_depth, 0, W, frame.data_ptr(), stream.cuda_stream, **{"samples": samples, **lens})
            elif samples == 1:
                self.render_device(W, H, max_depth, 0, W, frame.data_ptr(), stream.cuda_stream)
            else:
                self.render_ssaa_device(W, H, max_depth, samples, 0, W, frame.data_ptr(), stream.cuda_stream)
            capi.check(self._lib.rt_encode_image_device(device, C.byref(params), W, H, frame.data_ptr(), image.data_ptr(),
                                                        W * C_, stream.cuda_stream))
            return image.cpu().numpy()                            # the one download

    def trace_rays(self, rays, max_depth, rows=None):
        """Trace a batch of primary rays (include/rt_capi_rays.h).  rays: C-contiguous float32, (n, 6) -- rows defaults to n --
        or (X, Z, 6), ray [x, z] = cell (x, z) of the grid, rows = Z; each ray {E.xyz, T.xyz} starts at E towards T.
        -> float32 (n, 3) or (X, Z, 3).  rows only shapes the launch; the results do not depend on it."""
        n, default_rows = self._batch(rays, "rays")
        out = np.empty(rays.shape[:-1] + (3,), dtype=np.float32)
        capi.check(self._lib.rt_trace_rays(self._scene, n, int(default_rows if rows is None else rows), rays.ctypes.data, max_depth,
                                           out.ctypes.data))
        return out

    def trace_rays_device(self, n, rows, rays_ptr, max_depth, out_ptr, stream=0):
        """Enqueue the tracing of n rays (6 float32 each) at device address rays_ptr into 3 n float32 at out_ptr on a HIP
        stream (no sync; rays_ptr must stay valid until the stream has drained)."""
        capi.check(self._lib.rt_trace_rays_device(self._scene, n, rows, C.c_void_p(rays_ptr), max_depth, C.c_void_p(out_ptr),
                                                  C.c_void_p(stream)))

    def _batch(self, rays, what):
        if not isinstance(rays, np.ndarray) or rays.dtype != np.float32 or not rays.flags.c_contiguous:
            raise TypeError(f"{what} must be a C-contiguous float32 numpy array")
        if rays.ndim not in (2, 3) or rays.shape[-1] != 6:
            raise ValueError(f"{what} must have shape (n, 6) or (X, Z, 6), not {rays.shape}")
        n = rays.size // 6
        return n, max(rays.shape[1] if rays.ndim == 3 else n, 1)       # (an empty batch: any rows)

    def intersect_rays(self, rays, rows=None):
        """What each ray hits (include/rt_capi_query.h, rt_intersect_rays).  rays: C-contiguous float32, (n, 6) -- rows defaults
        to n -- or (X, Z, 6), rows = Z; each ray {E.xyz, T.xyz} starts at E towards T.  -> a structured array of HIT_DTYPE
        (rt_hit: object -1 = no hit), shape (n,) or (X, Z).  rows only shapes the launch; the results do not depend on it."""
        n, default_rows = self._batch(rays, "rays")
        out = np.zeros(rays.shape[:-1], dtype=HIT_DTYPE)
        capi.check(self._lib.rt_intersect_rays(self._scene, n, int(default_rows if rows is None else rows), rays.ctypes.data,
                                               out.ctypes.data))
        return out

    def intersect_rays_device(self, n, rows, rays_ptr, out_ptr, stream=0):
        """Enqueue the records (48 bytes each, out_ptr 16-byte aligned) of n rays (6 float32 each) at device address rays_ptr
        on a HIP stream (no sync; rays_ptr must stay valid until the stream has drained)."""
        capi.check(self._lib.rt_intersect_rays_device(self._scene, n, rows, C.c_void_p(rays_ptr), C.c_void_p(out_ptr),
                                                      C.c_void_p(stream)))

    def occluded_rays(self, segs, rows=None):
        """Whether each segment {E.xyz, T.xyz} is blocked (include/rt_capi_query.h, rt_occluded_rays): inShade with the point E
        and a light at T.  segs as intersect_rays' rays.  -> bool, shape (n,) or (X, Z)."""
        n, default_rows = self._batch(segs, "segs")
        out = np.zeros(segs.shape[:-1], dtype=np.uint8)
        capi.check(self._lib.rt_occluded_rays(self._scene, n, int(default_rows if rows is None else rows), segs.ctypes.data,
                                              out.ctypes.data))
        return out.view(np.bool_)

    def occluded_rays_device(self, n, rows, segs_ptr, out_ptr, stream=0):
        """Enqueue the verdicts (one byte each, 0 or 1) of n segments (6 float32 each) at device address segs_ptr on a HIP
        stream (no sync; segs_ptr must stay valid until the stream has drained)."""
        capi.check(self._lib.rt_occluded_rays_device(self._scene, n, rows, C.c_void_p(segs_ptr), C.c_void_p(out_ptr),
                                                     C.c_void_p(stream)))

    @staticmethod
    def _ao_params(samples, radius, seed, key0, channels):
        return capi.RtAoParams(int(samples), float(radius), int(seed) & 0xFFFFFFFF, int(key0) & 0xFFFFFFFF, int(channels))

    def ambient_occlusion(self, hits, samples=4, radius=1.0, seed=0, key0=0, channels=1, rows=None):
        """The open fraction of samples x samples hemisphere directions of length radius around each hit record
        (include/rt_capi_ao.h, rt_ambient_occlusion).  hits: C-contiguous HIT_DTYPE, (n,) -- rows defaults to n -- or (X, Z),
        rows = Z, as render_gbuffer() and intersect_rays() return them; record i samples with key0 + i (a strip of a W x H
        frame from column x0: key0 = x0 * H).  -> float32 of hits' shape, or with channels = 3 of that shape + (3,), the
        three equal.  rows only shapes the launch; the results do not depend on it."""
        if not isinstance(hits, np.ndarray) or hits.dtype != HIT_DTYPE or not hits.flags.c_contiguous:
            raise TypeError("hits must be a C-contiguous numpy array of HIT_DTYPE")
        if hits.ndim not in (1, 2):
            raise ValueError(f"hits must have shape (n,) or (X, Z), not {hits.shape}")
        n = hits.size
        default_rows = max(hits.shape[1] if hits.ndim == 2 else n, 1)
        params = self._ao_params(samples, radius, seed, key0, channels)
        out = np.empty(hits.shape + ((3,) if params.channels == 3 else ()), dtype=np.float32)
        capi.check(self._lib.rt_ambient_occlusion(self._scene, C.byref(params), n, int(default_rows if rows is None else rows),
                                                  hits.ctypes.data, out.ctypes.data))
        return out

    def ambient_occlusion_device(self, n, rows, hits_ptr, out_ptr, samples=4, radius=1.0, seed=0, key0=0, channels=1, stream=0):
        """Enqueue the ambient occlusion of n records (48 bytes each, hits_ptr 16-byte aligned) into n * channels float32 at
        out_ptr on a HIP stream (no sync; hits_ptr must stay valid until the stream has drained)."""
        params = self._ao_params(samples, radius, seed, key0, channels)
        capi.check(self._lib.rt_ambient_occlusion_device(self._scene, C.byref(params), n, rows, C.c_void_p(hits_ptr),
                                                         C.c_void_p(out_ptr), C.c_void_p(stream)))

    def render_ao(self, W, H, samples=4, radius=1.0, seed=0, channels=1, scale=1, normal_squarings=3, sigma_plane=0.0,
                  refine=False, key0_refine=0x80000000, mirrors=None):
        """The ambient-occlusion plane of a W x H frame, computed on the GPU where its records were made: a depth-0
        rt_render_gbuffer_device and rt_ambient_occlusion_device (rows = H) enqueued on one stream with no host wait between
        them, then a download of the plane alone -> float32 (W, H), or (W, H, 3) with channels = 3 (a grey frame for denoise()
        and encode_image()).  The result is ambient_occlusion(render_gbuffer(W, H, 0)[1], ...) bit for bit.  The device buffers
        and the stream are torch's, so the process must have imported torch before the library was loaded (INTEGRATION.md
        section 3).  scale 2..8 (include/rt_capi_upsample.h): the plane is gathered for every scale-th pixel in both directions
        and upsampled, rt_subsample_hits_device, rt_ambient_occlusion_device and rt_upsample_guided_device on that one stream
        with no host wait -- ambient_occlusion_scaled(render_gbuffer(W, H, 0)[1], scale, ...) bit for bit; refine costs exactly
        one read-back of the flags before the holes' batch is enqueued.  mirrors: None, or a dict of max_bounces,
        min_reflective and optionally compact, or min_transmissive and glass_compact (include/rt_mirror.h, rt_mirror_compact.h,
        rt_glass.h, rt_glass_compact.h; scale 1 only): the plane is gathered at the terminal records of the pixel rays,
        ambient_occlusion(render_gbuffer_mirrored(W, H, 0, ...)[1], ...) bit for bit -- an open fraction takes no weight."""
        import torch
        if mirrors is not None:
            if scale != 1:
                raise ValueError("mirrors needs scale 1")
            return self._render_ao_mirrored(W, H, self._ao_params(samples, radius, seed, 0, channels), mirrors)
        if scale != 1:
            return self._render_ao_scaled(W, H, samples, radius, seed, channels, scale, normal_squarings, sigma_plane, refine,
                                          key0_refine)
        params = self._ao_params(samples, radius, seed, 0, channels)
        C_ = 3 if params.channels == 3 else 1                        # (a bad count is refused by the call below)
        with torch.cuda.device(int(self._device)):
            colours = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
            records = torch.empty((W * H * 12,), dtype=torch.int32, device="cuda")
            plane = torch.empty((W, H, C_), dtype=torch.float32, device="cuda")
            stream = torch.cuda.current_stream()
            self.render_gbuffer_device(W, H, 0, 0, W, colours.data_ptr(), records.data_ptr(), stream.cuda_stream)
            capi.check(self._lib.rt_ambient_occlusion_device(self._scene, C.byref(params), W * H, H, records.data_ptr(),
                                                             plane.data_ptr(), stream.cuda_stream))
            out = plane.cpu().numpy()                                 # the one download
        return out if C_ == 3 else out.reshape(W, H)

    def ambient_occlusion_scaled(self, hits, scale, samples=4, radius=1.0, seed=0, key0=0, channels=1, normal_squarings=3,
                                 sigma_plane=0.0, refine=False, key0_refine=0x80000000, return_flags=False):
        """ambient_occlusion() gathered for every scale-th pixel in both directions only and carried to every pixel of the
        frame hits (HIT_DTYPE (Wn, H)) by upsample_guided() (include/rt_capi_upsample.h) -> float32 (Wn, H), or (Wn, H, 3) with
        channels = 3, and with return_flags also the holes, bool (Wn, H).  DEFINITION: cells = subsample_hits(hits, scale,
        white=True); lo = ambient_occlusion(cells, samples, radius, seed, key0, channels); the result is upsample_guided(hits,
        lo, scale, normal_squarings, sigma_plane=sigma_plane, dead_value=1.0, return_flags=True) bit for bit.  refine: the holes,
        in ascending pixel order (np.flatnonzero(flags)), are then gathered as one more batch of their own full-resolution
        records with key0 = key0_refine, and written over the fallback."""
        hits = _frame_records(hits)
        cells = subsample_hits(hits, scale, True, self._device)
        lo = self.ambient_occlusion(cells, samples, radius, seed, key0, channels)
        out, flags = upsample_guided(hits, lo, scale, normal_squarings, False, False, sigma_plane, 1.0, None, True, self._device)
        if refine and flags.any():
            idx = np.flatnonzero(flags)
            holes = np.ascontiguousarray(hits.reshape(-1)[idx])
            out.reshape((hits.size,) + out.shape[2:])[idx] = self.ambient_occlusion(holes, samples, radius, seed, key0_refine, channels)
        return (out, flags) if return_flags else out

    def indirect_diffuse_scaled(self, hits, scale, samples=4, gather_depth=1, gain=1.0, seed=0, key0=0, emitters=False,
                                chunk_records=0, base=None, normal_squarings=3, sigma_plane=0.0, refine=False,
                                key0_refine=0x80000000, return_flags=False, bounces=1, compact=False):
        """indirect_diffuse() gathered for every scale-th pixel in both directions only and carried to every pixel of the frame
        hits (HIT_DTYPE (Wn, H)) by upsample_guided() (include/rt_capi_upsample.h) -> float32 (Wn, H, 3), and with return_flags
        also the holes, bool (Wn, H).  DEFINITION: cells = subsample_hits(hits, scale, white=True); lo = indirect_diffuse(cells,
        samples, gather_depth, gain, seed, key0, emitters) -- no base: irradiance without albedo, (kd gain) mean; the result is
        upsample_guided(hits, lo, scale, normal_squarings, match_color=False, modulate=True, sigma_plane=sigma_plane,
        dead_value=0.0, base=base, return_flags=True) bit for bit: the filter runs across a surface's checker tiles and texels,
        and each pixel multiplies by its own albedo.  refine: the holes, in ascending pixel order (np.flatnonzero(flags)), are
        then gathered as one more batch of their own full-colour, full-resolution records with key0 = key0_refine and no base,
        and base + term (term, without a base: one fp32 add a word) is written over the fallback.  chunk_records never changes
        the result.  bounces and compact: given to both indirect_diffuse() calls."""
        hits = _frame_records(hits)
        kw = dict(samples=samples, gather_depth=gather_depth, gain=gain, seed=seed, emitters=emitters, chunk_records=chunk_records,
                  bounces=bounces, compact=compact)
        cells = subsample_hits(hits, scale, True, self._device)
        lo = self.indirect_diffuse(cells, key0=key0, **kw)
        out, flags = upsample_guided(hits, lo, scale, normal_squarings, False, True, sigma_plane, 0.0, base, True, self._device)
        if refine and flags.any():
            idx = np.flatnonzero(flags)
            term = self.indirect_diffuse(np.ascontiguousarray(hits.reshape(-1)[idx]), key0=key0_refine, **kw)
            if base is not None:
                term = np.ascontiguousarray(base, dtype=np.float32).reshape(-1, 3)[idx] + term
            out.reshape(-1, 3)[idx] = term
        return (out, flags) if return_flags else out

    def _upsample_device(self, params, W, H, records, lo, base, out, flags, stream):
        capi.check(self._lib.rt_upsample_guided_device(int(self._device), C.byref(params), W, H, records.data_ptr(), lo.data_ptr(),
                                                       base.data_ptr() if base is not None else None, out.data_ptr(),
                                                       flags.data_ptr() if flags is not None else None, stream.cuda_stream))

    def _subsample_device(self, scale, W, H, records, stream):
        """-> (the white cells of a frame's records as an int32 tensor, Wl, Hl), enqueued"""
        import torch
        s = int(scale)
        if not 2 <= s <= 8:                                           # (refused by the call itself)
            capi.check(self._lib.rt_subsample_hits_device(int(self._device), s, 1, W, H, None, None, None))
        Wl, Hl = -(-W // s), -(-H // s)
        cells = torch.empty((Wl * Hl * 12,), dtype=torch.int32, device="cuda")
        capi.check(self._lib.rt_subsample_hits_device(int(self._device), s, 1, W, H, records.data_ptr(), cells.data_ptr(),
                                                      stream.cuda_stream))
        return cells, Wl, Hl

    def indirect_diffuse(self, hits, samples=4, gather_depth=1, gain=1.0, seed=0, key0=0, emitters=False, chunk_records=0,
                         base=None, bounces=1, compact=False):
        """One diffuse bounce for every hit record (include/rt_capi_indirect.h, rt_indirect_diffuse): samples x samples gather
        rays per record in ambient_occlusion()'s directions, traced at gather_depth, averaged and weighted by the record's
        colour, its object's diffuse coefficient and gain.  hits: C-contiguous HIT_DTYPE of any shape, as render_gbuffer() and
        intersect_rays() return them; record i samples with key0 + i (a strip of a W x H frame from column x0: key0 = x0 * H).
        base: None, or float32 hits.shape + (3,) that the term is added to (a frame's direct colours).  emitters False: a
        gather ray whose first hit is a light counts black, since the record's direct shading has that light already.
        -> float32 hits.shape + (3,).  chunk_records (the most records gathered per launch, 0: the default) never changes the
        result; indirect_info() tells what each stage cost.  bounces 1: this call; any other count is indirect_paths()
        (include/rt_paths.h), which the library checks.  compact: indirect_paths(compact=True) whatever bounces is."""
        if bounces != 1 or compact:
            return self.indirect_paths(hits, bounces, samples, gather_depth, gain, seed, key0, emitters, chunk_records, base,
                                       compact)
        hits = _records(hits)
        params = indirect_params(samples, gather_depth, gain, seed, key0, emitters, chunk_records)
        if base is not None:
            base = np.ascontiguousarray(base, dtype=np.float32)
            if base.shape != hits.shape + (3,):
                raise ValueError(f"base must have shape {hits.shape + (3,)}, not {base.shape}")
        out = np.empty(hits.shape + (3,), dtype=np.float32)
        capi.check(self._lib.rt_indirect_diffuse(self._scene, C.byref(params), hits.size, hits.ctypes.data,
                                                 base.ctypes.data if base is not None else None, out.ctypes.data))
        return out

    def indirect_diffuse_device(self, n, hits_ptr, base_ptr, out_ptr, stream=0, samples=4, gather_depth=1, gain=1.0, seed=0, key0=0,
                                emitters=False, chunk_records=0, bounces=1, compact=False):
        """Enqueue the indirect term of n records (48 bytes each, hits_ptr 16-byte aligned) into 3 n float32 at out_ptr, added to
        the 3 n float32 at base_ptr unless that is 0 (base_ptr == out_ptr: in place), on a HIP stream (no sync: nothing is read
        back).  bounces 1: rt_indirect_diffuse_device; any other count is indirect_paths_device().  compact:
        indirect_paths_device(compact=True) whatever bounces is -- that call WAITS for the stream."""
        if bounces != 1 or compact:
            return self.indirect_paths_device(n, hits_ptr, base_ptr, out_ptr, stream, bounces, samples, gather_depth, gain, seed,
                                              key0, emitters, chunk_records, compact)
        params = indirect_params(samples, gather_depth, gain, seed, key0, emitters, chunk_records)
        capi.check(self._lib.rt_indirect_diffuse_device(self._scene, C.byref(params), n, C.c_void_p(hits_ptr),
                                                        C.c_void_p(base_ptr or None), C.c_void_p(out_ptr), C.c_void_p(stream)))

    def indirect_info(self):
        """The last indirect_diffuse*() of this scene (include/rt_capi_indirect.h, rt_indirect_info): records, rays, chunks and
        the four stage times."""
        info = capi.RtIndirectInfo()
        capi.check(self._lib.rt_get_indirect_info(self._scene, C.byref(info)))
        return info

    def indirect_paths(self, hits, bounces=2, samples=4, gather_depth=1, gain=1.0, seed=0, key0=0, emitters=False,
                       chunk_records=0, base=None, compact=False):
        """Diffuse light paths of up to `bounces` rays for every hit record (include/rt_paths.h, rt_indirect_paths): each of
        indirect_diffuse()'s samples x samples gather rays is followed from diffuse hit to diffuse hit, one new direction a hit,
        and what every bounce's ray brings in is added, weighted by the surfaces the path has left.  The arguments and the
        result are indirect_diffuse()'s; with bounces 1 so is every word.  paths_info() tells what each stage cost and how many
        paths were alive at every bounce.  compact: trace only the paths still alive (include/rt_paths_compact.h,
        rt_indirect_paths_compact): the same words, fewer rays traced, one host wait per bounce; paths_compact_info() then
        describes the call, and paths_info() does not."""
        hits = _records(hits)
        params = paths_params(samples, gather_depth, gain, seed, key0, emitters, chunk_records, bounces)
        if base is not None:
            base = np.ascontiguousarray(base, dtype=np.float32)
            if base.shape != hits.shape + (3,):
                raise ValueError(f"base must have shape {hits.shape + (3,)}, not {base.shape}")
        out = np.empty(hits.shape + (3,), dtype=np.float32)
        call = self._lib.rt_indirect_paths_compact if compact else self._lib.rt_indirect_paths
        capi.check(call(self._scene, C.byref(params), hits.size, hits.ctypes.data, base.ctypes.data if base is not None else None,
                        out.ctypes.data))
        return out

    def indirect_paths_device(self, n, hits_ptr, base_ptr, out_ptr, stream=0, bounces=2, samples=4, gather_depth=1, gain=1.0, seed=0,
                              key0=0, emitters=False, chunk_records=0, compact=False):
        """Enqueue indirect_paths() of n records (48 bytes each, hits_ptr 16-byte aligned) into 3 n float32 at out_ptr, added to
        the 3 n float32 at base_ptr unless that is 0 (base_ptr == out_ptr: in place), on a HIP stream (no sync: nothing is read
        back).  compact: rt_indirect_paths_compact_device (include/rt_paths_compact.h) -- the same words over the paths still
        alive; it WAITS for the stream once per bounce, so the stream must not be capturing, and returns with its last step and
        its resolve possibly still running."""
        params = paths_params(samples, gather_depth, gain, seed, key0, emitters, chunk_records, bounces)
        call = self._lib.rt_indirect_paths_compact_device if compact else self._lib.rt_indirect_paths_device
        capi.check(call(self._scene, C.byref(params), n, C.c_void_p(hits_ptr), C.c_void_p(base_ptr or None), C.c_void_p(out_ptr),
                        C.c_void_p(stream)))

    def paths_info(self):
        """The last indirect_paths*() of this scene (include/rt_paths.h, rt_paths_info): records, rays, chunks, the five stage
        times and alive[b], the paths alive at bounce b."""
        info = capi.RtPathsInfo()
        capi.check(self._lib.rt_get_paths_info(self._scene, C.byref(info)))
        return info

    def paths_compact_info(self):
        """The last indirect_paths*(compact=True) of this scene (include/rt_paths_compact.h, rt_paths_compact_info): records, the
        rays actually traced, chunks, ray batches, hit queries and stream waits, the five stage times and alive[b]."""
        info = capi.RtPathsCompactInfo()
        capi.check(self._lib.rt_get_paths_compact_info(self._scene, C.byref(info)))
        return info

    def _render_ao_scaled(self, W, H, samples, radius, seed, channels, scale, normal_squarings, sigma_plane, refine, key0_refine):
        import torch
        C_ = 3 if int(channels) == 3 else 1                          # (a bad count is refused by the calls below)
        up = upsample_params(scale, channels, normal_squarings, False, False, sigma_plane, 1.0)
        kw = dict(samples=samples, radius=radius, seed=seed, channels=channels)
        with torch.cuda.device(int(self._device)):
            colours = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
            records = torch.empty((W * H * 12,), dtype=torch.int32, device="cuda")
            plane = torch.empty((W * H, C_), dtype=torch.float32, device="cuda")
            flags = torch.empty((W * H,), dtype=torch.uint8, device="cuda") if refine else None
            stream = torch.cuda.current_stream()
            self.render_gbuffer_device(W, H, 0, 0, W, colours.data_ptr(), records.data_ptr(), stream.cuda_stream)
            cells, Wl, Hl = self._subsample_device(scale, W, H, records, stream)
            lo = torch.empty((Wl * Hl, C_), dtype=torch.float32, device="cuda")
            self.ambient_occlusion_device(Wl * Hl, Hl, cells.data_ptr(), lo.data_ptr(), key0=0, stream=stream.cuda_stream, **kw)
            self._upsample_device(up, W, H, records, lo, None, plane, flags, stream)
            if refine:
                idx = torch.nonzero(flags).reshape(-1)                 # the one read-back: how many holes there are
                if idx.numel():
                    holes = records.view(W * H, 12)[idx].contiguous()
                    term = torch.empty((idx.numel(), C_), dtype=torch.float32, device="cuda")
                    self.ambient_occlusion_device(idx.numel(), idx.numel(), holes.data_ptr(), term.data_ptr(), key0=key0_refine,
                                                  stream=stream.cuda_stream, **kw)
                    plane[idx] = term
            out = plane.cpu().numpy()                                 # the one download
        return out.reshape(W, H, 3) if C_ == 3 else out.reshape(W, H)

    def _render_indirect_scaled(self, W, H, max_depth, kw, denoise, scale, normal_squarings, sigma_plane, refine, key0_refine):
        import torch
        device = int(self._device)
        up = upsample_params(scale, 3, normal_squarings, False, True, sigma_plane, 0.0)
        if denoise is not None:
            dn = capi.RtDenoiseParams(int(denoise.get("iterations", 2)), int(denoise.get("normal_squarings", 3)),
                                      float(denoise.get("sigma_color", 1.0)))
            scratch_bytes = self._lib.rt_denoise_scratch_bytes(C.byref(dn), W, H)
            if not scratch_bytes:                                     # (bad parameters: refused by the call itself)
                capi.check(self._lib.rt_denoise_device(device, C.byref(dn), W, H, None, None, None, None, None))
        with torch.cuda.device(device):
            colours = torch.empty((W * H, 3), dtype=torch.float32, device="cuda")
            records = torch.empty((W * H * 12,), dtype=torch.int32, device="cuda")
            flags = torch.empty((W * H,), dtype=torch.uint8, device="cuda") if refine else None
            stream = torch.cuda.current_stream()
            self.render_gbuffer_device(W, H, max_depth, 0, W, colours.data_ptr(), records.data_ptr(), stream.cuda_stream)
            cells, Wl, Hl = self._subsample_device(scale, W, H, records, stream)
            lo = torch.empty((Wl * Hl, 3), dtype=torch.float32, device="cuda")
            self.indirect_diffuse_device(Wl * Hl, cells.data_ptr(), 0, lo.data_ptr(), stream.cuda_stream, **kw)
            # the upsampled term: onto the colours in place, or alone where a filter or the holes' batch comes before the add
            alone = denoise is not None or refine
            term = torch.empty((W * H, 3), dtype=torch.float32, device="cuda") if alone else colours
            self._upsample_device(up, W, H, records, lo, None if alone else colours, term, flags, stream)
            if refine:
                idx = torch.nonzero(flags).reshape(-1)                 # the one read-back: how many holes there are
                if idx.numel():
                    holes = records.view(W * H, 12)[idx].contiguous()
                    fine = torch.empty((idx.numel(), 3), dtype=torch.float32, device="cuda")
                    self.indirect_diffuse_device(idx.numel(), holes.data_ptr(), 0, fine.data_ptr(), stream.cuda_stream,
                                                 **dict(kw, key0=key0_refine))
                    term[idx] = fine
            if denoise is not None:
                clean = torch.empty((W * H, 3), dtype=torch.float32, device="cuda")
                scratch = torch.empty(((scratch_bytes + 15) // 16 * 4,), dtype=torch.int32, device="cuda")
                capi.check(self._lib.rt_denoise_device(device, C.byref(dn), W, H, term.data_ptr(), records.data_ptr(),
                                                       clean.data_ptr(), scratch.data_ptr(), stream.cuda_stream))
                term = clean
            out = torch.add(colours, term) if alone else colours
            return out.cpu().numpy().reshape(W, H, 3)                 # the one download

    def render_indirect(self, W, H, max_depth, samples=4, gather_depth=1, gain=1.0, seed=0, emitters=False, denoise=None, scale=1,
                        normal_squarings=3, sigma_plane=0.0, refine=False, key0_refine=0x80000000, mirrors=None, bounces=1, compact=False):
        """A W x H frame with one diffuse bounce added, computed on the GPU where its records were made
        (include/rt_capi_indirect.h): rt_render_gbuffer_device and rt_indirect_diffuse_device -- the frame's colours the base,
        in place -- enqueued on one stream with no host wait between them, then one download -> float32 (W, H, 3).  The result
        is indirect_diffuse(hits, ..., base=rgb) of rgb, hits = render_gbuffer(W, H, max_depth) bit for bit.  denoise: None, or
        a dict of denoise()'s keywords (iterations, sigma_color, normal_squarings): the indirect term alone is then computed
        without a base, filtered by rt_denoise_device with the frame's records and added to the direct colours by one fp32
        add -- rgb + denoise(indirect_diffuse(hits, ...), hits, ...) bit for bit.  The device buffers and the stream are
        torch's, so the process must have imported torch before the library was loaded.  scale 2..8
        (include/rt_capi_upsample.h): the term is gathered for every scale-th pixel in both directions and upsampled --
        rt_subsample_hits_device, rt_indirect_diffuse_device and rt_upsample_guided_device on that one stream with no host wait
        -- indirect_diffuse_scaled(hits, scale, ..., base=rgb) bit for bit, and with denoise rgb + denoise(
        indirect_diffuse_scaled(hits, scale, ...), hits, ...); refine costs exactly one read-back of the flags before the holes'
        batch is enqueued.  With scale 1 nothing of this runs and normal_squarings, sigma_plane and refine are not read.
        mirrors: None, or a dict of max_bounces, min_reflective and optionally compact, or min_transmissive and glass_compact (include/rt_mirror.h, rt_mirror_compact.h,
        rt_glass.h, rt_glass_compact.h;
        scale 1 and no denoise only): the term
        is gathered at the terminal records of the pixel rays and multiplied by the path's weight before it is added -- with
        (_, hits, _, weight, _) = render_gbuffer_mirrored(W, H, max_depth, ...), rgb + weight * indirect_diffuse(hits, ...), one
        fp32 multiply and one fp32 add, bit for bit.  bounces: indirect_diffuse()'s, in every one of these compositions (any count
        but 1: rt_indirect_paths_device, include/rt_paths.h, in rt_indirect_diffuse_device's place).  compact:
        rt_indirect_paths_compact_device (include/rt_paths_compact.h) in that place, whatever bounces is -- the same frame bit for
        bit, but the call then WAITS for the stream once per bounce and chunk instead of only before the download."""
        import torch
        device = int(self._device)
        kw = dict(samples=samples, gather_depth=gather_depth, gain=gain, seed=seed, emitters=emitters, bounces=bounces)
        if compact:
            kw["compact"] = True
        if mirrors is not None:
            if scale != 1 or denoise is not None:
                raise ValueError("mirrors needs scale 1 and no denoise")
            return self._render_indirect_mirrored(W, H, max_depth, kw, mirrors)
        if scale != 1:
            return self._render_indirect_scaled(W, H, max_depth, kw, denoise, scale, normal_squarings, sigma_plane, refine,
                                                key0_refine)
        if denoise is not None:
            dn = capi.RtDenoiseParams(int(denoise.get("iterations", 2)), int(denoise.get("normal_squarings", 3)),
                                      float(denoise.get("sigma_color", 1.0)))
            scratch_bytes = self._lib.rt_denoise_scratch_bytes(C.byref(dn), W, H)
            if not scratch_bytes:                                     # (bad parameters: refused by the call itself)
                capi.check(self._lib.rt_denoise_device(device, C.byref(dn), W, H, None, None, None, None, None))
        with torch.cuda.device(device):
            colours = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
            records = torch.empty((W * H * 12,), dtype=torch.int32, device="cuda")
            stream = torch.cuda.current_stream()
            self.render_gbuffer_device(W, H, max_depth, 0, W, colours.data_ptr(), records.data_ptr(), stream.cuda_stream)
            if denoise is None:
                self.indirect_diffuse_device(W * H, records.data_ptr(), colours.data_ptr(), colours.data_ptr(), stream.cuda_stream,
                                             **kw)
                return colours.cpu().numpy()                          # the one download
            term = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
            clean = torch.empty((W, H, 3), dtype=torch.float32, device="cuda")
            scratch = torch.empty(((scratch_bytes + 15) // 16 * 4,), dtype=torch.int32, device="cuda")
            self.indirect_diffuse_device(W * H, records.data_ptr(), 0, term.data_ptr(), stream.cuda_stream, **kw)
            capi.check(self._lib.rt_denoise_device(device, C.byref(dn), W, H, term.data_ptr(), records.data_ptr(), clean.data_ptr(),
                                                   scratch.data_ptr(), stream.cuda_stream))
            return torch.add(colours, clean).cpu().numpy()            # the one download

    MIRROR_OUTPUTS = ("guide", "weight", "path")

    def mirror_records(self, rays, max_bounces=8, min_reflective=1.0, rows=None, chunk_rays=0, outputs=MIRROR_OUTPUTS,
                       compact=False):
        """What each ray sees through the scene's mirrors (include/rt_mirror.h, rt_mirror_records).  rays as intersect_rays'
        (float32 (n, 6) or (X, Z, 6)); a hit is followed while its object's `reflective` >= min_reflective, max_bounces times
        at the most.  -> (hits, guide, weight, path): the terminal records and the guide records (HIT_DTYPE, rays' shape), the
        path's throughput (float32, shape + (3,)) and the path word (uint32: k | cut << 8 | tag << 12).  hits is what
        ambient_occlusion() and indirect_diffuse() gather at; guide is what the filters and the accumulation are steered by --
        its object is a tagged id, never an index.  outputs: which of the three optional ones are asked for; the others are
        None and what is returned does not depend on them.  rows and chunk_rays never change a result.  compact: walk only
        the rays still alive (include/rt_mirror_compact.h, rt_mirror_records_compact): the same words, fewer rays queried, one
        host wait per bounce; mirror_compact_info() then describes the call, and mirror_info() does not."""
        n, default_rows = self._batch(rays, "rays")
        shape = rays.shape[:-1]
        hits = np.zeros(shape, dtype=HIT_DTYPE)
        guide = np.zeros(shape, dtype=HIT_DTYPE) if "guide" in outputs else None
        weight = np.zeros(shape + (3,), dtype=np.float32) if "weight" in outputs else None
        path = np.zeros(shape, dtype=np.uint32) if "path" in outputs else None
        params = mirror_params(max_bounces, min_reflective, chunk_rays)
        ptr = lambda a: a.ctypes.data if a is not None else None
        call = self._lib.rt_mirror_records_compact if compact else self._lib.rt_mirror_records
        capi.check(call(self._scene, C.byref(params), n, int(default_rows if rows is None else rows), rays.ctypes.data,
                        hits.ctypes.data, ptr(guide), ptr(weight), ptr(path)))
        return hits, guide, weight, path

    def mirror_records_device(self, n, rows, rays_ptr, hits_ptr, guide_ptr=0, weight_ptr=0, path_ptr=0, stream=0, max_bounces=8,
                              min_reflective=1.0, chunk_rays=0, compact=False):
        """Enqueue the mirror chains of n rays (6 float32 each) at device address rays_ptr on a HIP stream: the terminal
        records at hits_ptr and, unless 0, the guide records at guide_ptr (48 bytes each, 16-byte aligned), 3 n float32 at
        weight_ptr and n uint32 at path_ptr (no sync: nothing is read back; rays_ptr must stay valid until the stream has
        drained).  compact: rt_mirror_records_compact_device (include/rt_mirror_compact.h) -- the same words over the rays still
        alive; it WAITS for the stream once per bounce, so the stream must not be capturing, and returns with its last step
        possibly still running."""
        params = mirror_params(max_bounces, min_reflective, chunk_rays)
        call = self._lib.rt_mirror_records_compact_device if compact else self._lib.rt_mirror_records_device
        capi.check(call(self._scene, C.byref(params), n, rows, C.c_void_p(rays_ptr), C.c_void_p(hits_ptr),
                        C.c_void_p(guide_ptr or None), C.c_void_p(weight_ptr or None), C.c_void_p(path_ptr or None),
                        C.c_void_p(stream)))

    def glass_records(self, rays, max_bounces=8, min_reflective=1.0, min_transmissive=0.5, rows=None, chunk_rays=0,
                      outputs=MIRROR_OUTPUTS, compact=False):
        """What each ray sees through the scene's mirrors and its glass (include/rt_glass.h, rt_glass_records): mirror_records()
        with one more way to go on -- a hit on an object whose transmission factor is > 0 and >= min_transmissive is looked
        through along rt_capi_refract.h's transmitted child where that child exists.  max_bounces counts mirrors and glass
        objects together.  -> mirror_records()'s (hits, guide, weight, path); the path word is k | cut << 8 | g << 10 |
        tag << 12, g: some glass was looked through.  With min_transmissive = inf every word is mirror_records()'s.  compact:
        walk only the rays still alive (include/rt_glass_compact.h, rt_glass_records_compact): the same words, fewer rays queried,
        one host wait per bounce; glass_compact_info() then describes the call, and glass_info() does not."""
        n, default_rows = self._batch(rays, "rays")
        shape = rays.shape[:-1]
        hits = np.zeros(shape, dtype=HIT_DTYPE)
        guide = np.zeros(shape, dtype=HIT_DTYPE) if "guide" in outputs else None
        weight = np.zeros(shape + (3,), dtype=np.float32) if "weight" in outputs else None
        path = np.zeros(shape, dtype=np.uint32) if "path" in outputs else None
        params = glass_params(max_bounces, min_reflective, min_transmissive, chunk_rays)
        ptr = lambda a: a.ctypes.data if a is not None else None
        call = self._lib.rt_glass_records_compact if compact else self._lib.rt_glass_records
        capi.check(call(self._scene, C.byref(params), n, int(default_rows if rows is None else rows), rays.ctypes.data,
                        hits.ctypes.data, ptr(guide), ptr(weight), ptr(path)))
        return hits, guide, weight, path

    def glass_records_device(self, n, rows, rays_ptr, hits_ptr, guide_ptr=0, weight_ptr=0, path_ptr=0, stream=0, max_bounces=8,
                             min_reflective=1.0, min_transmissive=0.5, chunk_rays=0, compact=False):
        """mirror_records_device() through glass as well (include/rt_glass.h, rt_glass_records_device): enqueued on the HIP
        stream with no sync, nothing read back, so the stream may be capturing once an eager call has grown the scratch.
        compact: rt_glass_records_compact_device (include/rt_glass_compact.h) -- the same words over the rays still alive; it
        WAITS for the stream once per bounce, so the stream must not be capturing, and returns with its last step possibly
        still running."""
        params = glass_params(max_bounces, min_reflective, min_transmissive, chunk_rays)
        call = self._lib.rt_glass_records_compact_device if compact else self._lib.rt_glass_records_device
        capi.check(call(self._scene, C.byref(params), n, rows, C.c_void_p(rays_ptr), C.c_void_p(hits_ptr),
                        C.c_void_p(guide_ptr or None), C.c_void_p(weight_ptr or None), C.c_void_p(path_ptr or None),
                        C.c_void_p(stream)))

    def glass_info(self):
        """The last glass_records*() of this scene (include/rt_glass.h, rt_glass_info): rays, chunks, queries and the two
        stage times."""
        info = capi.RtGlassInfo()
        capi.check(self._lib.rt_get_glass_info(self._scene, C.byref(info)))
        return info

    def glass_compact_info(self):
        """The last glass_records*(compact=True) of this scene (include/rt_glass_compact.h, rt_glass_compact_info): rays,
        rays_queried, chunks, queries, syncs, the two stage times and alive[b]."""
        info = capi.RtGlassCompactInfo()
        capi.check(self._lib.rt_get_glass_compact_info(self._scene, C.byref(info)))
        return info

    def mirror_info(self):
        """The last mirror_records*() of this scene (include/rt_mirror.h, rt_mirror_info): rays, chunks, queries and the two
        stage times."""
        info = capi.RtMirrorInfo()
        capi.check(self._lib.rt_get_mirror_info(self._scene, C.byref(info)))
        return info

    def mirror_compact_info(self):
        """The last mirror_records*(compact=True) of this scene (include/rt_mirror_compact.h, rt_mirror_compact_info): rays,
        rays_queried, chunks, queries, syncs, the two stage times and alive[b]."""
        info = capi.RtMirrorCompactInfo()
        capi.check(self._lib.rt_get_mirror_compact_info(self._scene, C.byref(info)))
        return info

    def _mirror_device(self, W, H, x0, x1, mirrors, stream):
        """the four outputs of the pixel rays of columns [x0, x1) as torch tensors on the device (records as 12 int32 words),
        enqueued on `stream`: rt_lens_rays_device at one sample, aperture 0, focus 1 -- rt_render's own pixel rays -- and
        rt_mirror_records_device (rows = H); mirrors: a dict of max_bounces and min_reflective and, optionally, compact
        (rt_mirror_records_compact_device in its place: the same words, with host waits) or min_transmissive
        (rt_glass_records_device in its place, include/rt_glass.h: glass is looked through) and, with that, glass_compact
        (rt_glass_records_compact_device, include/rt_glass_compact.h: the same words, with host waits)"""
        import torch
        unknown = set(mirrors) - {"max_bounces", "min_reflective", "compact", "min_transmissive", "glass_compact"}
        if unknown:
            raise ValueError(f"mirrors takes max_bounces, min_reflective and compact, or min_transmissive and glass_compact, "
                             f"not {sorted(unknown)}")
        glass = mirrors.get("min_transmissive") is not None
        if glass and mirrors.get("compact"):
            raise ValueError("mirrors: with min_transmissive the compact form is asked for by glass_compact, not compact "
                             "(include/rt_glass_compact.h)")
        if mirrors.get("glass_compact") and not glass:
            raise ValueError("mirrors: glass_compact is valid only with min_transmissive (include/rt_glass_compact.h)")
        n = max(x1 - x0, 0) * H
        lens = lens_params(1, 0.0, 1.0, 0)
        rays = torch.empty((n * 6,), dtype=torch.float32, device="cuda")
        hits = torch.empty((n * 12,), dtype=torch.int32, device="cuda")
        guide = torch.empty((n * 12,), dtype=torch.int32, device="cuda")
        weight = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        path = torch.empty((n,), dtype=torch.int32, device="cuda")
        capi.check(self._lib.rt_lens_rays_device(self._cam, W, H, x0, x1, C.byref(lens), int(self._device), rays.data_ptr(),
                                                 stream.cuda_stream))
        if glass:
            kw = {k: v for k, v in mirrors.items() if k not in ("compact", "glass_compact")}
            kw["compact"] = bool(mirrors.get("glass_compact"))
            self.glass_records_device(n, max(H, 1), rays.data_ptr(), hits.data_ptr(), guide.data_ptr(), weight.data_ptr(),
                                      path.data_ptr(), stream.cuda_stream, **kw)
            return hits, guide, weight, path
        kw = {k: v for k, v in mirrors.items() if k not in ("min_transmissive", "glass_compact")}
        self.mirror_records_device(n, max(H, 1), rays.data_ptr(), hits.data_ptr(), guide.data_ptr(), weight.data_ptr(),
                                   path.data_ptr(), stream.cuda_stream, **kw)
        return hits, guide, weight, path                               # (rays: torch frees them in the stream's order)

    def render_gbuffer_mirrored(self, W, H, max_depth, max_bounces=8, min_reflective=1.0, x0=0, x1=None, compact=False,
                                min_transmissive=None, glass_compact=False):
        """Columns [x0, x1) of a W x H frame with what each pixel sees through the mirrors (include/rt_mirror.h):
        render_gbuffer()'s colours, and mirror_records()'s four outputs for the pixel rays that lens_rays(camera, W, H,
        samples=1, aperture=0, focus=1) makes, generated and walked on the device with no host wait between the calls ->
        (rgb float32 (Wn, H, 3), hits HIT_DTYPE (Wn, H), guide HIT_DTYPE (Wn, H), weight float32 (Wn, H, 3), path uint32
        (Wn, H)).  Where no mirror was followed (path & 0xff == 0) hits is render_gbuffer()'s record.  The device buffers and
        the stream are torch's, so the process must have imported torch before the library was loaded.  compact: the chains
        are walked by rt_mirror_records_compact_device (include/rt_mirror_compact.h): the same words, with one host wait per
        bounce between the calls.  min_transmissive: None, or the transmission factor from which glass is looked through
        (include/rt_glass.h, rt_glass_records_device in the mirror call's place; not together with compact).  glass_compact:
        valid only with min_transmissive -- rt_glass_records_compact_device (include/rt_glass_compact.h) in its place: the same
        words, with one host wait per bounce."""
        import torch
        x1 = W if x1 is None else x1
        Wn = max(x1 - x0, 0)
        with torch.cuda.device(int(self._device)):
            colours = torch.empty((Wn, H, 3), dtype=torch.float32, device="cuda")
            records = torch.empty((Wn * H * 12,), dtype=torch.int32, device="cuda")
            stream = torch.cuda.current_stream()
            self.render_gbuffer_device(W, H, max_depth, x0, x1, colours.data_ptr(), records.data_ptr(), stream.cuda_stream)
            mirrors = dict(max_bounces=max_bounces, min_reflective=min_reflective, compact=compact)
            if min_transmissive is not None:
                mirrors["min_transmissive"] = min_transmissive
            if glass_compact:
                mirrors["glass_compact"] = True
            hits, guide, weight, path = self._mirror_device(W, H, x0, x1, mirrors, stream)
            return (colours.cpu().numpy(), hits.cpu().numpy().view(HIT_DTYPE).reshape(Wn, H),
                    guide.cpu().numpy().view(HIT_DTYPE).reshape(Wn, H), weight.cpu().numpy().reshape(Wn, H, 3),
                    path.cpu().numpy().view(np.uint32).reshape(Wn, H))

    def _render_indirect_mirrored(self, W, H, max_depth, kw, mirrors):
        """render_indirect(mirrors=...): rgb + weight * indirect_diffuse(terminal records), one fp32 multiply and one fp32 add"""
        import torch
        with torch.cuda.device(int(self._device)):
            colours = torch.empty((W * H, 3), dtype=torch.float32, device="cuda")
            records = torch.empty((W * H * 12,), dtype=torch.int32, device="cuda")
            term = torch.empty((W * H, 3), dtype=torch.float32, device="cuda")
            stream = torch.cuda.current_stream()
            self.render_gbuffer_device(W, H, max_depth, 0, W, colours.data_ptr(), records.data_ptr(), stream.cuda_stream)
            hits, _, weight, _ = self._mirror_device(W, H, 0, W, mirrors, stream)
            self.indirect_diffuse_device(W * H, hits.data_ptr(), 0, term.data_ptr(), stream.cuda_stream, **kw)
            return torch.add(colours, torch.mul(weight, term)).cpu().numpy().reshape(W, H, 3)       # the one download

    def _render_ao_mirrored(self, W, H, params, mirrors):
        """render_ao(mirrors=...): ambient_occlusion(terminal records); an open fraction is no radiance and takes no weight"""
        import torch
        C_ = 3 if params.channels == 3 else 1
        with torch.cuda.device(int(self._device)):
            plane = torch.empty((W, H, C_), dtype=torch.float32, device="cuda")
            stream = torch.cuda.current_stream()
            hits, _, _, _ = self._mirror_device(W, H, 0, W, mirrors, stream)
            capi.check(self._lib.rt_ambient_occlusion_device(self._scene, C.byref(params), W * H, H, hits.data_ptr(),
                                                             plane.data_ptr(), stream.cuda_stream))
            out = plane.cpu().numpy()                                 # the one download
        return out if C_ == 3 else out.reshape(W, H)

    def _accumulated_term_mirrored(self, W, H, term, samples, k, kw, mirrors, colours, plane, stream):
        """render_accumulated(mirrors=...): frame k's value from its colours, gathered at the terminal records -> (value, the
        guide records)"""
        import torch
        hits, guide, weight, _ = self._mirror_device(W, H, 0, W, mirrors, stream)
        if term == "indirect":
            gathered = torch.empty((W * H, 3), dtype=torch.float32, device="cuda")
            self.indirect_diffuse_device(W * H, hits.data_ptr(), 0, gathered.data_ptr(), stream.cuda_stream, samples=samples, seed=k,
                                         **kw)
            return torch.add(colours.view(W * H, 3), torch.mul(weight, gathered)).reshape(-1), guide
        if term == "ao":
            self.ambient_occlusion_device(W * H, H, hits.data_ptr(), plane.data_ptr(), samples=samples, seed=k,
                                          stream=stream.cuda_stream, **kw)
            return plane, guide
        return colours, guide

    def render_accumulated(self, cameras, W, H, max_depth, term="indirect", samples=1, filter=None, mirrors=None, clamp=None, **kw):
        """A sequence of W x H frames, one per camera of `cameras` (RtCameraDesc), accumulated on the GPU where they were made
        (include/rt_temporal.h): frame k is the G-buffer at max_depth and its term sampled with seed k -- "indirect": the
        colours plus indirect_diffuse(hits, samples, seed=k, base=rgb); "ao": ambient_occlusion(hits, samples, seed=k), one
        channel; "direct": the colours themselves after set_shadow_seed(k), for scenes with area lights (the scene's seed is
        left at the last k) -- pushed into one TemporalHistory with no host wait and no download between the frames.  kw:
        temporal_params()'s keywords (but channels) for the history, every other one for the term.  -> the last frame's (value,
        variance, flags), what temporal_accumulate() over the public calls' frames gives bit for bit.  filter: None, or a dict of
        svgf_params()'s keywords (but channels): the last frame goes through the variance-steered filter on the same stream
        (include/rt_svgf.h) and value and variance are the filtered ones, svgf_filter()'s of that frame bit for bit.
        mirrors: None, or a dict of max_bounces, min_reflective and optionally compact, or min_transmissive and glass_compact (include/rt_mirror.h, rt_mirror_compact.h,
        rt_glass.h, rt_glass_compact.h): the term is gathered at the terminal
        records of the pixel rays ("indirect": weighted as render_indirect(mirrors=...) does) and the history and the filter
        are given the guide records in place of the G-buffer's.  clamp: None, or a dict of clamp_params()'s keywords (but
        channels), given to every push (include/rt_clamp.h): each frame's history is clipped to that frame's neighbourhood
        before the next one blends into it, history_clamp() after every temporal_accumulate() bit for bit."""
        import torch
        if term not in ("indirect", "ao", "direct"):
            raise ValueError(f'term must be "indirect", "ao" or "direct", not {term!r}')
        names = ("match_color", "max_history", "normal_cos", "plane_eps", "alpha", "alpha_moments")
        history = TemporalHistory(W, H, 1 if term == "ao" else 3, self._device, **{k: kw.pop(k) for k in names if k in kw})
        cameras = list(cameras)
        if not cameras:
            raise ValueError("no cameras")
        own = self._cam
        try:
            with torch.cuda.device(int(self._device)):
                colours = torch.empty((W * H * 3,), dtype=torch.float32, device="cuda")
                records = torch.empty((W * H * 12,), dtype=torch.int32, device="cuda")
                plane = torch.empty((W * H,), dtype=torch.float32, device="cuda") if term == "ao" else None
                stream = torch.cuda.current_stream()
                for k, camera in enumerate(cameras):
                    self._cam = C.pointer(camera)
                    if term == "direct":
                        self.set_shadow_seed(k)
                    self.render_gbuffer_device(W, H, max_depth, 0, W, colours.data_ptr(), records.data_ptr(), stream.cuda_stream)
                    if mirrors is not None:
                        value, guide = self._accumulated_term_mirrored(W, H, term, samples, k, kw, mirrors, colours, plane, stream)
                        value, variance, flags = history.push_device(value, guide, camera, stream=stream, clamp=clamp)
                        continue
                    if term == "indirect":
                        self.indirect_diffuse_device(W * H, records.data_ptr(), colours.data_ptr(), colours.data_ptr(),
                                                     stream.cuda_stream, samples=samples, seed=k, **kw)
                    elif term == "ao":
                        self.ambient_occlusion_device(W * H, H, records.data_ptr(), plane.data_ptr(), samples=samples, seed=k,
                                                      stream=stream.cuda_stream, **kw)
                    value, variance, flags = history.push_device(plane if term == "ao" else colours, records, camera, stream=stream,
                                                                 clamp=clamp)
                if filter is not None:
                    value, variance = history.filter_device(stream=stream, **filter)
                shape = (W, H) if term == "ao" else (W, H, 3)
                return (value.cpu().numpy().reshape(shape), variance.cpu().numpy().reshape(W, H),
                        flags.cpu().numpy().reshape(W, H).view(np.bool_))
        finally:
            self._cam = own

    STAT_NAMES = ("nearest_rays", "shadow_rays", "wave_nearest_scans", "wave_shadow_scans",
                  "wave_sphere_tests", "wave_plane_tests", "wave_box_tests", "lane_sphere_tests",
                  "cycles_nearest", "cycles_shadow", "cycles_tile",
                  "cycles_winner", "cycles_lights", "cycles_reflect",
                  "shadow_candidates", "shadow_leaves_union", "shadow_leaves_maxlane",
                  "nearest_scans_1_16", "nearest_scans_17_32", "nearest_scans_33_48", "nearest_scans_49_64",
                  "nearest_scans_unculled", "nearest_unculled_box_tests", "nearest_unculled_sphere_tests", "nearest_sphere_tests")

    def learn_tile_order(self, W, H, max_depth, x0=0, x1=None):
        """rt_learn_tile_order: one frame of the counting build on this launch shape; later renders of the same shape hand their
        tile rows out most expensive first (speed only; set_option("learned_order", 0) forgets it)."""
        capi.check(self._lib.rt_learn_tile_order(self._scene, self._cam, W, H, x0, W if x1 is None else x1, max_depth))

    def render_stats(self, W, H, max_depth, x0=0, x1=None, wave_cycles=False):
        """Counting build: returns (image, {counter: value}[, per wavefront tile (tiles_z, tiles_x, 6) = cycles, sphere tests, box tests, scans, start, end (100 MHz)])."""
        x1 = W if x1 is None else x1
        out = np.empty((max(x1 - x0, 0), H, 3), dtype=np.float32)
        st = (C.c_uint64 * len(self.STAT_NAMES))()
        li = self.launch_info()
        tz = li.tile_z or 4
        tx = 64 // tz
        tiles = ((H + tz - 1) // tz, (x1 - x0 + tx - 1) // tx)      # (tile rows, tile columns), row-major
        cyc = np.zeros(tiles + (6,), dtype=np.uint64)
        capi.check(self._lib.rt_render_stats(self._scene, self._cam, W, H, x0, x1, max_depth,
                                             out.ctypes.data, st, len(self.STAT_NAMES),
                                             cyc.ctypes.data if wave_cycles else None, cyc.size if wave_cycles else 0))
        stats = dict(zip(self.STAT_NAMES, [int(v) for v in st]))
        return (out, stats, cyc) if wave_cycles else (out, stats)

    def timeline(self, x0, x1, H):
        """Per wavefront tile of the last launch (option "timeline" = 1): array (tile rows, tile columns, 4) =
        start, end (100 MHz clock), workgroup * 16 + wavefront, rendered-as-a-HEAVY-tile."""
        li = self.launch_info()
        tiles = ((H + li.tile_z - 1) // li.tile_z, (x1 - x0 + li.tile_x - 1) // li.tile_x)
        rec = np.zeros(tiles + (4,), dtype=np.uint64)
        capi.check(self._lib.rt_get_timeline(self._scene, rec.ctypes.data, rec.size))
        return rec

    def timing(self):
        t = capi.RtTiming()
        capi.check(self._lib.rt_get_timing(self._scene, C.byref(t)))
        return t

    def reset_timing(self):
        capi.check(self._lib.rt_reset_timing(self._scene))

    def kernel_name(self):
        """The whole name of the kernel the last launch ran (include/rt_capi_launch.h; launch_info().kernel is its first 47
        characters)."""
        buf = C.create_string_buffer(capi.RT_KERNEL_NAME_BYTES)
        capi.check(self._lib.rt_get_launch_kernel(self._scene, buf, len(buf)))
        return buf.value.decode()

    def launch_info(self):
        li = capi.RtLaunchInfo()
        capi.check(self._lib.rt_get_launch_info(self._scene, C.byref(li)))
        return li


def render_animated(frames, W, H, max_depth, term="indirect", samples=1, filter=None, clamp=None, gradient=None, **kw):
    """Renderer.render_accumulated() for a scene whose objects move (include/rt_motion.h): frames is a sequence of (Renderer,
    camera, motions or None), one per W x H frame -- the Renderer of that frame's pose (all on one device), its camera (an
    RtCameraDesc) and the motion table from that pose to the previous frame's (object_motions(); push_device()'s motions; the
    first frame's is never read).  Frame k is its renderer's G-buffer at max_depth and its term sampled with seed k, as
    render_accumulated() makes them, pushed into one TemporalHistory with the frame's table, with no host wait and no download
    between the frames.  kw, filter and clamp are render_accumulated()'s.  -> the last frame's (value, variance, flags), what
    motion_accumulate() -- with clamp, followed by history_clamp() -- over the public calls' frames gives bit for bit.
    gradient: None, or a dict of gradient_params()'s keywords (but channels), s its scale (include/rt_gradient.h): for every
    frame k >= 1 a (W/s) x (H/s) G-buffer is rendered under frame k's camera on frame k's renderer and on frame k-1's, the term
    is evaluated on both with the same samples, seed k and key0 0 ("direct": set_shadow_seed(k) on both, which is where frame
    k-1's renderer's seed is left), and the two results and the two record sets go to the push, all on the one stream with no
    host wait.  ValueError if W or H is not a multiple of s.  The result is then what, frame by frame, motion_accumulate(),
    gradient_reweight(now_lo, then_lo, lo_hits, then_hits) from frame 1 on -- the cell frames made by the public calls:
    render_gbuffer(W/s, H/s) of both renderers under the frame's camera and the term of each -- and, with clamp,
    history_clamp() give bit for bit.  Frame 0 and gradient=None are the calls without it, word for word."""
    import torch
    if term not in ("indirect", "ao", "direct"):
        raise ValueError(f'term must be "indirect", "ao" or "direct", not {term!r}')
    frames = list(frames)
    if not frames:
        raise ValueError("no frames")
    device = int(frames[0][0]._device)
    if any(int(r._device) != device for r, _, _ in frames):
        raise ValueError("the frames' renderers must be on one device")
    if gradient is not None:
        # refused before anything is rendered: the call without buffers, whose last check is the parameters' and the rectangle's
        gradient, lib = dict(gradient), capi.load_library()
        pr = gradient_params(1 if term == "ao" else 3, **gradient)
        rc = lib.rt_gradient_reweight_device(device, C.byref(pr), W, H, *([None] * 16))
        if b"is NULL" not in lib.rt_last_error():
            capi.check(rc)
        scale = pr.scale
        if W % scale or H % scale:
            raise ValueError(f"W and H must be multiples of the gradient's scale {scale}, not {W} x {H}")
    names = ("match_color", "max_history", "normal_cos", "plane_eps", "alpha", "alpha_moments")
    history = TemporalHistory(W, H, 1 if term == "ao" else 3, device, **{k: kw.pop(k) for k in names if k in kw})
    own = [(r, r._cam) for r, _, _ in frames]
    try:
        with torch.cuda.device(device):
            colours = torch.empty((W * H * 3,), dtype=torch.float32, device="cuda")
            records = torch.empty((W * H * 12,), dtype=torch.int32, device="cuda")
            plane = torch.empty((W * H,), dtype=torch.float32, device="cuda") if term == "ao" else None
            stream = torch.cuda.current_stream()
            if gradient is not None:
                Wl, Hl = W // scale, H // scale
                lo = [dict(colours=torch.empty((Wl * Hl * 3,), dtype=torch.float32, device="cuda"),
                           records=torch.empty((Wl * Hl * 12,), dtype=torch.int32, device="cuda"),
                           plane=torch.empty((Wl * Hl,), dtype=torch.float32, device="cuda") if term == "ao" else None)
                      for _ in range(2)]
            for k, (r, camera, motions) in enumerate(frames):
                r._cam = C.pointer(camera)
                if term == "direct":
                    r.set_shadow_seed(k)
                cells = None
                if gradient is not None and k >= 1:
                    # the two cell frames: this frame's points, shaded in this frame's scene and in the previous frame's
                    then = frames[k - 1][0]
                    then._cam = C.pointer(camera)
                    if term == "direct":
                        then.set_shadow_seed(k)
                    for q, b in ((r, lo[0]), (then, lo[1])):
                        q.render_gbuffer_device(Wl, Hl, max_depth, 0, Wl, b["colours"].data_ptr(), b["records"].data_ptr(),
                                                stream.cuda_stream)
                        if term == "indirect":
                            q.indirect_diffuse_device(Wl * Hl, b["records"].data_ptr(), b["colours"].data_ptr(),
                                                      b["colours"].data_ptr(), stream.cuda_stream, samples=samples, seed=k, **kw)
                        elif term == "ao":
                            q.ambient_occlusion_device(Wl * Hl, Hl, b["records"].data_ptr(), b["plane"].data_ptr(), samples=samples,
                                                       seed=k, stream=stream.cuda_stream, **kw)
                    name = "plane" if term == "ao" else "colours"
                    cells = dict(gradient, now_lo=lo[0][name], then_lo=lo[1][name], lo_hits=lo[0]["records"],
                                 then_hits=lo[1]["records"])
                r.render_gbuffer_device(W, H, max_depth, 0, W, colours.data_ptr(), records.data_ptr(), stream.cuda_stream)
                if term == "indirect":
                    r.indirect_diffuse_device(W * H, records.data_ptr(), colours.data_ptr(), colours.data_ptr(), stream.cuda_stream,
                                              samples=samples, seed=k, **kw)
                elif term == "ao":
                    r.ambient_occlusion_device(W * H, H, records.data_ptr(), plane.data_ptr(), samples=samples, seed=k,
                                               stream=stream.cuda_stream, **kw)
                value, variance, flags = history.push_device(plane if term == "ao" else colours, records, camera, stream=stream,
                                                             motions=motions, clamp=clamp, gradient=cells)
            if filter is not None:
                value, variance = history.filter_device(stream=stream, **filter)
            shape = (W, H) if term == "ao" else (W, H, 3)
            return (value.cpu().numpy().reshape(shape), variance.cpu().numpy().reshape(W, H),
                    flags.cpu().numpy().reshape(W, H).view(np.bool_))
    finally:
        for r, cam in own:
            r._cam = cam
