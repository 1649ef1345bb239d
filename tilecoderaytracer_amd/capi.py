"""ctypes bindings for the drop-in boundary, include/rt_capi.h, and for the
speed-only options and diagnostics of include/rt_capi_tuning.h.

Struct layouts below must match the headers field for field.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

RT_OK, RT_ERR_INVALID, RT_ERR_NO_DEVICE, RT_ERR_HIP, RT_ERR_CAPACITY, RT_ERR_RCCL = range(6)
RT_KIND_SPHERE, RT_KIND_INFINITE_PLANE, RT_KIND_FINITE_PLANE = 0, 1, 2

F3 = C.c_float * 3


class RtObjectDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("is_light", C.c_int32), ("texture", C.c_int32),
        ("intensity", C.c_float),
        ("origin", F3), ("color", F3),
        ("diffuse", C.c_float), ("specular", C.c_float), ("reflective", C.c_float),
        ("radius", C.c_float), ("radius_squared", C.c_float),
        ("plane_origin", F3),
        ("normal", F3), ("vertical", F3), ("horizontal", F3), ("reverse_normal", F3),
        ("v_distance", C.c_float), ("h_distance", C.c_float),
        ("distance_to_origin", C.c_float),
    ]


class RtTextureDesc(C.Structure):
    _fields_ = [("light", F3), ("dark", F3), ("width", C.c_float), ("height", C.c_float)]


RT_TEX_WRAP_CHECKER, RT_TEX_WRAP_REPEAT, RT_TEX_WRAP_CLAMP = 0, 1, 2
RT_MAX_SCENE_TEXELS = 1 << 20


class RtImageTextureDesc(C.Structure):
    """include/rt_capi_texture.h: an image texture for planes, texel (i, j) at texels[(j * texels_w + i) * 3 + c]."""
    _fields_ = [("texels_w", C.c_int32), ("texels_h", C.c_int32), ("width", C.c_float), ("height", C.c_float),
                ("wrap", C.c_int32), ("texels", C.POINTER(C.c_float))]


class RtRefractionDesc(C.Structure):
    """include/rt_capi_refract.h: a refractive object -- Scene index, transmission factor tf, a sphere interior's ior."""
    _fields_ = [("object", C.c_int32), ("refractive", C.c_float), ("ior", C.c_float)]


class RtAreaLightDesc(C.Structure):
    """include/rt_capi_soft.h: an area light -- Scene index of a light, n (n x n samples), the disc's radius."""
    _fields_ = [("object", C.c_int32), ("samples", C.c_int32), ("radius", C.c_float)]


class RtDenoiseParams(C.Structure):
    """include/rt_capi_denoise.h: the filter's iterations (1..5), normal squarings (0..6) and colour sigma (0: no colour term)."""
    _fields_ = [("iterations", C.c_int32), ("normal_squarings", C.c_int32), ("sigma_color", C.c_float)]


class RtUpsampleParams(C.Structure):
    """include/rt_capi_upsample.h: the scale s (2..8), channels (1 or 3), normal squarings (0..6), match_color and modulate
    (0 / 1), the plane term's sigma (0: none) and the value of a pixel with no surface."""
    _fields_ = [("scale", C.c_int32), ("channels", C.c_int32), ("normal_squarings", C.c_int32), ("match_color", C.c_int32),
                ("modulate", C.c_int32), ("sigma_plane", C.c_float), ("dead_value", C.c_float)]


class RtTemporalParams(C.Structure):
    """include/rt_temporal.h: channels (1 or 3), match_color (0 / 1), the cap of the history length (1..65535), the normals'
    cosine (-1..1) and the tangent-plane distance (0: no test) a tap must keep, and the floors of the two blend weights (0..1)."""
    _fields_ = [("channels", C.c_int32), ("match_color", C.c_int32), ("max_history", C.c_int32), ("normal_cos", C.c_float),
                ("plane_eps", C.c_float), ("alpha", C.c_float), ("alpha_moments", C.c_float)]


class RtObjectMotion(C.Structure):
    """include/rt_motion.h: the rows {m0 m1 m2 | m3}, {m4 .. m7}, {m8 .. m11} of the rigid motion that carries a point of an
    object in the current frame to where it was in the previous frame."""
    _fields_ = [("m", C.c_float * 12)]


class RtSvgfParams(C.Structure):
    """include/rt_svgf.h: channels (1 or 3), iterations (1..5), normal squarings (0..6), match_color (0 / 1), the history length
    below which the variance is estimated spatially (1..65535), that estimate's radius (1..3), the luminance term's sigma (0:
    none), the plane term's (0: none) and the epsilon added to sigma_l^2 * variance (> 0)."""
    _fields_ = [("channels", C.c_int32), ("iterations", C.c_int32), ("normal_squarings", C.c_int32), ("match_color", C.c_int32),
                ("min_history", C.c_int32), ("spatial_radius", C.c_int32), ("sigma_l", C.c_float), ("sigma_plane", C.c_float),
                ("epsilon", C.c_float)]


class RtClampParams(C.Structure):
    """include/rt_clamp.h: channels (1 or 3), box (0 extremes, 1 moments), radius (1..3), match_color (0 / 1), the fewest counted
    taps a pixel is clipped with (1..49), the length a clipped pixel keeps at most (1..65535), the normals' cosine a tap must keep
    (-1..1) and the moments box's width in standard deviations (>= 0)."""
    _fields_ = [("channels", C.c_int32), ("box", C.c_int32), ("radius", C.c_int32), ("match_color", C.c_int32),
                ("min_taps", C.c_int32), ("clip_history", C.c_int32), ("normal_cos", C.c_float), ("gamma", C.c_float)]


class RtGradientParams(C.Structure):
    """include/rt_gradient.h: channels (1 or 3), scale (one cell per s x s pixels, 2..8), radius (0..2: a window of (2r+2)^2
    cells), match_color (0 / 1), the normals' cosine a cell must keep (-1..1), the gain on the relative gradient (>= 0), the
    weight at or below which a pixel is left alone (0..1) and the cells' light at or below which there is no gradient (>= 0)."""
    _fields_ = [("channels", C.c_int32), ("scale", C.c_int32), ("radius", C.c_int32), ("match_color", C.c_int32),
                ("normal_cos", C.c_float), ("gain", C.c_float), ("lambda_min", C.c_float), ("den_floor", C.c_float)]


class RtAoParams(C.Structure):
    """include/rt_capi_ao.h: n (n x n directions per record, 1..8), the radius a direction is followed for, the seed, the first
    record's key, channels (1, or 3 equal ones)."""
    _fields_ = [("samples", C.c_int32), ("radius", C.c_float), ("seed", C.c_uint32), ("key0", C.c_uint32),
                ("channels", C.c_int32)]


class RtAdaptiveParams(C.Structure):
    """include/rt_capi_adaptive.h: k (1, 2 or 4), flag_all (0 / 1), the most flagged pixels a launch traces (0: the default),
    the colour threshold (finite, >= 0) and the normals' cosine (-1..1) of the flag test."""
    _fields_ = [("samples", C.c_int32), ("flag_all", C.c_int32), ("chunk_pixels", C.c_int32), ("color_threshold", C.c_float),
                ("normal_cos", C.c_float)]


class RtAdaptiveInfo(C.Structure):
    """include/rt_capi_adaptive.h: the scene's last rt_render_adaptive* call -- strip pixels, of them refined, rays traced in the
    second pass, its launches, and the four stages' HIP-event times."""
    _fields_ = [("pixels", C.c_int64), ("flagged", C.c_int64), ("rays", C.c_int64), ("chunks", C.c_int32),
                ("first_pass_ms", C.c_double), ("flag_ms", C.c_double), ("trace_ms", C.c_double), ("resolve_ms", C.c_double)]


class RtLensParams(C.Structure):
    """include/rt_capi_lens.h: n (n x n samples per pixel, 1..8), the most columns a launch traces (0: the default), the seed,
    the lens radius (finite, >= 0) and the focal plane's distance as a multiple of the screen's (finite, > 0)."""
    _fields_ = [("samples", C.c_int32), ("chunk_columns", C.c_int32), ("seed", C.c_uint32), ("aperture", C.c_float),
                ("focus", C.c_float)]


class RtLensInfo(C.Structure):
    """include/rt_capi_lens.h: the scene's last rt_render_lens* call -- strip pixels, rays traced, chunks of columns, and the
    three stages' HIP-event times."""
    _fields_ = [("pixels", C.c_int64), ("rays", C.c_int64), ("chunks", C.c_int32), ("raygen_ms", C.c_double),
                ("trace_ms", C.c_double), ("resolve_ms", C.c_double)]


class RtIndirectParams(C.Structure):
    """include/rt_capi_indirect.h: n (n x n gather rays per record, 1..8), the gather rays' max_depth, the most records a launch
    gathers for (0: the default), emitters (0: a gather ray whose first hit is a light counts black; 1: as traced), the seed,
    the first record's key and the term's gain (finite)."""
    _fields_ = [("samples", C.c_int32), ("gather_depth", C.c_int32), ("chunk_records", C.c_int32), ("emitters", C.c_int32),
                ("seed", C.c_uint32), ("key0", C.c_uint32), ("gain", C.c_float)]


class RtIndirectInfo(C.Structure):
    """include/rt_capi_indirect.h: the scene's last rt_indirect_diffuse* call -- its records, gather rays traced, chunks of
    records, and the four stages' HIP-event times (query_ms 0 with emitters 1)."""
    _fields_ = [("records", C.c_int64), ("rays", C.c_int64), ("chunks", C.c_int32), ("raygen_ms", C.c_double),
                ("trace_ms", C.c_double), ("query_ms", C.c_double), ("resolve_ms", C.c_double)]


RT_PATHS_MAX_BOUNCES = 8


class RtPathsParams(C.Structure):
    """include/rt_paths.h: RtIndirectParams' seven fields in their order, then the most rays a path traces (1..8)."""
    _fields_ = RtIndirectParams._fields_ + [("bounces", C.c_int32)]


class RtPathsInfo(C.Structure):
    """include/rt_paths.h: the scene's last rt_indirect_paths* call -- its records, rays traced over all bounces, chunks of
    records, the five stages' HIP-event times and the paths alive at every bounce."""
    _fields_ = [("records", C.c_int64), ("rays", C.c_int64), ("chunks", C.c_int32), ("raygen_ms", C.c_double),
                ("trace_ms", C.c_double), ("query_ms", C.c_double), ("step_ms", C.c_double), ("resolve_ms", C.c_double),
                ("alive", C.c_int64 * RT_PATHS_MAX_BOUNCES)]


class RtPathsCompactInfo(C.Structure):
    """include/rt_paths_compact.h: the scene's last rt_indirect_paths_compact* call -- its records, the rays its ray batches were
    asked (records * S + the sum of alive[b >= 1]), chunks, ray batches and hit queries launched, stream waits made, the five
    stages' HIP-event times and the paths alive at every bounce."""
    _fields_ = [("records", C.c_int64), ("rays", C.c_int64), ("chunks", C.c_int32), ("traces", C.c_int32),
                ("queries", C.c_int32), ("syncs", C.c_int32), ("raygen_ms", C.c_double), ("trace_ms", C.c_double),
                ("query_ms", C.c_double), ("step_ms", C.c_double), ("resolve_ms", C.c_double),
                ("alive", C.c_int64 * RT_PATHS_MAX_BOUNCES)]


RT_MIRROR_MAX_BOUNCES = 64


class RtMirrorParams(C.Structure):
    """include/rt_mirror.h: the most mirrors followed (0..64), the most rays walked per launch (0: the default) and the
    `reflective` at or above which a hit is followed (not NaN)."""
    _fields_ = [("max_bounces", C.c_int32), ("chunk_rays", C.c_int32), ("min_reflective", C.c_float)]


class RtMirrorInfo(C.Structure):
    """include/rt_mirror.h: the scene's last rt_mirror_records* call -- its rays, chunks of rays, hit queries launched, and the
    two stages' HIP-event times."""
    _fields_ = [("rays", C.c_int64), ("chunks", C.c_int32), ("queries", C.c_int32), ("query_ms", C.c_double),
                ("step_ms", C.c_double)]


class RtMirrorCompactInfo(C.Structure):
    """include/rt_mirror_compact.h: the scene's last rt_mirror_records_compact* call -- its rays, the rays its queries were
    asked (the sum of alive), chunks, hit queries launched, stream waits made, the two stages' HIP-event times, and alive[b], the
    rays whose chain reached query b."""
    _fields_ = [("rays", C.c_int64), ("rays_queried", C.c_int64), ("chunks", C.c_int32), ("queries", C.c_int32),
                ("syncs", C.c_int32), ("reserved", C.c_int32), ("query_ms", C.c_double), ("step_ms", C.c_double),
                ("alive", C.c_int64 * (RT_MIRROR_MAX_BOUNCES + 1))]


class RtGlassParams(C.Structure):
    """include/rt_glass.h: RtMirrorParams and the transmission factor at or above which a hit is looked through (not NaN;
    +inf: never)."""
    _fields_ = [("max_bounces", C.c_int32), ("chunk_rays", C.c_int32), ("min_reflective", C.c_float),
                ("min_transmissive", C.c_float)]


class RtGlassInfo(C.Structure):
    """include/rt_glass.h: the scene's last rt_glass_records* call, RtMirrorInfo's fields."""
    _fields_ = [("rays", C.c_int64), ("chunks", C.c_int32), ("queries", C.c_int32), ("query_ms", C.c_double),
                ("step_ms", C.c_double)]


class RtGlassCompactInfo(C.Structure):
    """include/rt_glass_compact.h: the scene's last rt_glass_records_compact* call, RtMirrorCompactInfo's fields."""
    _fields_ = [("rays", C.c_int64), ("rays_queried", C.c_int64), ("chunks", C.c_int32), ("queries", C.c_int32),
                ("syncs", C.c_int32), ("reserved", C.c_int32), ("query_ms", C.c_double), ("step_ms", C.c_double),
                ("alive", C.c_int64 * (RT_MIRROR_MAX_BOUNCES + 1))]


RT_TRANSFER_SRGB, RT_TRANSFER_LINEAR, RT_TRANSFER_CUSTOM = 0, 1, 2


class RtImageParams(C.Structure):
    """include/rt_capi_image.h: channels (3 or 4), bottom_up (0: row 0 is the top), transfer (RT_TRANSFER_*), exposure (finite,
    > 0), thresholds (RT_TRANSFER_CUSTOM: 255 floats T[1..255])."""
    _fields_ = [("channels", C.c_int32), ("bottom_up", C.c_int32), ("transfer", C.c_int32), ("exposure", C.c_float),
                ("thresholds", C.POINTER(C.c_float))]


class RtSceneDesc(C.Structure):
    _fields_ = [
        ("n_objects", C.c_int32), ("objects", C.POINTER(RtObjectDesc)),
        ("n_textures", C.c_int32), ("textures", C.POINTER(RtTextureDesc)),
        ("shadow_begin", C.c_int32), ("shadow_end", C.c_int32),
        ("null_color", F3),
    ]


class RtCameraDesc(C.Structure):
    _fields_ = [
        ("screen_width", C.c_float), ("screen_height", C.c_float),
        ("screen_halfwidth", C.c_float), ("screen_halfheight", C.c_float),
        ("screen_origin", F3), ("vector_horizontal", F3), ("vector_vertical", F3),
        ("eye_origin", F3),
    ]


class RtTiming(C.Structure):
    _fields_ = [
        ("last_kernel_ms", C.c_double), ("sum_kernel_ms", C.c_double),
        ("launches", C.c_uint64),
        ("last_upload_ms", C.c_double), ("last_download_ms", C.c_double),
    ]


class RtLaunchInfo(C.Structure):
    _fields_ = [
        ("block_threads", C.c_int32), ("lds_bytes", C.c_int32), ("scene_lds_bytes", C.c_int32),
        ("grid_blocks", C.c_int32), ("tile_x", C.c_int32), ("tile_z", C.c_int32),
        ("kernel", C.c_char * 48),
    ]


class RtPrimaryItem(C.Structure):
    """include/rt_capi_tuning.h: one item of the PRIMARY table -- its object's Scene index, its pixel rectangle, its entry distance"""
    _fields_ = [("object", C.c_int32), ("x_lo", C.c_int32), ("x_hi", C.c_int32), ("z_lo", C.c_int32), ("z_hi", C.c_int32),
                ("entry", C.c_float)]


RT_PRIMARY_ITEMS_MAX = 64
RT_MULTI_MAX_GPUS = 16
RT_KERNEL_NAME_BYTES = 64                 # include/rt_capi_launch.h


class RtMultiInfo(C.Structure):
    _fields_ = [
        ("ngpu", C.c_int32), ("chunks", C.c_int32), ("balanced", C.c_int32), ("transport", C.c_int32),
        ("bounds", C.c_int32 * (RT_MULTI_MAX_GPUS + 1)),
        ("kernel_ms", C.c_double * RT_MULTI_MAX_GPUS),
        ("frame_ms", C.c_double),
        ("measured_kernel_ms", C.c_double * RT_MULTI_MAX_GPUS),
        ("measured_gather_ms", C.c_double),
        ("trial_image_ok", C.c_int32 * 2),
        ("trial_frame_ms", C.c_double * 2),
    ]


class RtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"rt_capi error {code}: {message}")
        self.code = code
        self.message = message


_lib = None


def library_path():
    """lib/libtcrt.so next to this package, unless TCRT_LIBRARY names another build of it."""
    return os.environ.get("TCRT_LIBRARY") or os.path.join(LIB_DIR, "libtcrt.so")


def load_library():
    """Load lib/libtcrt.so.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `make -C tilecoderaytracer_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    lib = C.CDLL(path)
    vp, i = C.c_void_p, C.c_int
    lib.rt_capi_version.restype = i
    lib.rt_last_error.restype = C.c_char_p
    lib.rt_device_count.argtypes = [C.POINTER(i)]
    lib.rt_scene_create.argtypes = [C.POINTER(RtSceneDesc), i, C.POINTER(vp)]
    lib.rt_scene_destroy.argtypes = [vp]
    lib.rt_render.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, vp]
    lib.rt_render_device.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, vp, vp]
    lib.rt_render_multi.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(RtCameraDesc), i, i, i, i, vp]
    lib.rt_strip_bounds.argtypes = [i, i, i, C.POINTER(i), C.POINTER(i)]
    lib.rt_strip_bounds.restype = i
    lib.rt_chunk_bounds.argtypes = [i, i, i, i, i, C.POINTER(i), C.POINTER(i)]
    lib.rt_multi_create.argtypes = [C.POINTER(RtSceneDesc), i, C.POINTER(vp)]
    lib.rt_multi_render.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, vp]
    lib.rt_multi_set_option.argtypes = [vp, C.c_char_p, i]
    lib.rt_multi_set_bounds.argtypes = [vp, i, C.POINTER(i), i]
    lib.rt_multi_get_info.argtypes = [vp, C.POINTER(RtMultiInfo)]
    lib.rt_balance_strips.argtypes = [i, i, C.POINTER(i), C.POINTER(C.c_double), C.c_double, i, C.POINTER(i)]
    lib.rt_suggest_chunks.argtypes = [C.c_double, C.c_double, i]
    lib.rt_capi_tuning_version.restype = i
    lib.rt_shared_image_create.argtypes = [i, C.c_uint64, C.POINTER(vp), C.c_char_p]
    lib.rt_shared_image_open.argtypes = [i, C.c_char_p, C.POINTER(vp)]
    lib.rt_shared_image_close.argtypes = [i, vp]
    lib.rt_shared_image_destroy.argtypes = [i, vp]
    lib.rt_multi_destroy.argtypes = [vp]
    lib.rt_render_stats.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, vp, C.POINTER(C.c_uint64), i, vp, i]
    lib.rt_learn_tile_order.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i]
    lib.rt_get_timing.argtypes = [vp, C.POINTER(RtTiming)]
    lib.rt_get_timeline.argtypes = [vp, vp, i]
    lib.rt_get_timeline.restype = i
    lib.rt_reset_timing.argtypes = [vp]
    lib.rt_get_launch_info.argtypes = [vp, C.POINTER(RtLaunchInfo)]
    lib.rt_set_option.argtypes = [vp, C.c_char_p, i]
    # (absent from builds older than it, which TCRT_LIBRARY may name for A/B timing)
    if hasattr(lib, "rt_primary_rectangles"):
        lib.rt_primary_rectangles.argtypes = [C.POINTER(RtSceneDesc), C.POINTER(RtCameraDesc), i, i, C.POINTER(RtPrimaryItem), i,
                                              C.POINTER(i)]
        lib.rt_primary_rectangles.restype = i
    # include/rt_capi_ssaa.h (absent from builds older than it, which TCRT_LIBRARY may name for A/B timing)
    if hasattr(lib, "rt_render_ssaa"):
        lib.rt_capi_ssaa_version.restype = i
        lib.rt_render_ssaa.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, i, vp]
        lib.rt_render_ssaa_device.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, i, vp, vp]
        lib.rt_render_ssaa.restype = lib.rt_render_ssaa_device.restype = i
    # include/rt_capi_rays.h (likewise absent from older builds)
    if hasattr(lib, "rt_trace_rays"):
        lib.rt_capi_rays_version.restype = i
        lib.rt_trace_rays.argtypes = [vp, i, i, vp, i, vp]
        lib.rt_trace_rays_device.argtypes = [vp, i, i, vp, i, vp, vp]
        lib.rt_trace_rays.restype = lib.rt_trace_rays_device.restype = i
    # include/rt_capi_query.h (likewise absent from older builds)
    if hasattr(lib, "rt_intersect_rays"):
        lib.rt_capi_query_version.restype = i
        lib.rt_intersect_rays.argtypes = lib.rt_occluded_rays.argtypes = [vp, i, i, vp, vp]
        lib.rt_intersect_rays_device.argtypes = lib.rt_occluded_rays_device.argtypes = [vp, i, i, vp, vp, vp]
        for name in ("rt_intersect_rays", "rt_intersect_rays_device", "rt_occluded_rays", "rt_occluded_rays_device"):
            getattr(lib, name).restype = i
    # include/rt_capi_gbuffer.h (likewise absent from older builds)
    if hasattr(lib, "rt_render_gbuffer"):
        lib.rt_capi_gbuffer_version.restype = i
        lib.rt_render_gbuffer.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, vp, vp]
        lib.rt_render_gbuffer_device.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, vp, vp, vp]
        lib.rt_render_gbuffer.restype = lib.rt_render_gbuffer_device.restype = i
    # include/rt_capi_texture.h (likewise absent from older builds)
    if hasattr(lib, "rt_scene_create_textured"):
        lib.rt_capi_texture_version.restype = i
        lib.rt_scene_create_textured.argtypes = [C.POINTER(RtSceneDesc), i, C.POINTER(RtImageTextureDesc), i, C.POINTER(vp)]
        lib.rt_scene_create_textured.restype = i
    # include/rt_capi_refract.h (likewise absent from older builds)
    if hasattr(lib, "rt_scene_create_refractive"):
        lib.rt_capi_refract_version.restype = i
        lib.rt_scene_create_refractive.argtypes = [C.POINTER(RtSceneDesc), i, C.POINTER(RtImageTextureDesc), i,
                                                   C.POINTER(RtRefractionDesc), i, C.POINTER(vp)]
        lib.rt_scene_create_refractive.restype = i
    # include/rt_capi_soft.h (likewise absent from older builds)
    if hasattr(lib, "rt_scene_create_soft"):
        lib.rt_capi_soft_version.restype = i
        lib.rt_scene_create_soft.argtypes = [C.POINTER(RtSceneDesc), i, C.POINTER(RtImageTextureDesc), i,
                                             C.POINTER(RtRefractionDesc), i, C.POINTER(RtAreaLightDesc), i, C.POINTER(vp)]
        lib.rt_scene_create_soft.restype = i
        lib.rt_scene_set_shadow_seed.argtypes = [vp, C.c_uint32]
        lib.rt_scene_set_shadow_seed.restype = i
    # include/rt_capi_denoise.h (likewise absent from older builds)
    if hasattr(lib, "rt_denoise"):
        lib.rt_capi_denoise_version.restype = i
        lib.rt_denoise.argtypes = [i, C.POINTER(RtDenoiseParams), i, i, vp, vp, vp, C.POINTER(C.c_double)]
        lib.rt_denoise_device.argtypes = [i, C.POINTER(RtDenoiseParams), i, i, vp, vp, vp, vp, vp]
        lib.rt_denoise.restype = lib.rt_denoise_device.restype = i
        lib.rt_denoise_scratch_bytes.argtypes = [C.POINTER(RtDenoiseParams), i, i]
        lib.rt_denoise_scratch_bytes.restype = C.c_uint64
    # include/rt_capi_image.h (likewise absent from older builds)
    if hasattr(lib, "rt_encode_image"):
        lib.rt_capi_image_version.restype = i
        lib.rt_image_transfer_table.argtypes = [i, C.POINTER(C.c_float)]
        lib.rt_encode_image.argtypes = [i, C.POINTER(RtImageParams), i, i, vp, vp, C.c_uint64, C.POINTER(C.c_double)]
        lib.rt_encode_image_device.argtypes = [i, C.POINTER(RtImageParams), i, i, vp, vp, C.c_uint64, vp]
        lib.rt_image_transfer_table.restype = lib.rt_encode_image.restype = lib.rt_encode_image_device.restype = i
    # include/rt_capi_ao.h (likewise absent from older builds)
    if hasattr(lib, "rt_ambient_occlusion"):
        lib.rt_capi_ao_version.restype = i
        lib.rt_ambient_occlusion.argtypes = [vp, C.POINTER(RtAoParams), i, i, vp, vp]
        lib.rt_ambient_occlusion_device.argtypes = [vp, C.POINTER(RtAoParams), i, i, vp, vp, vp]
        lib.rt_ambient_occlusion.restype = lib.rt_ambient_occlusion_device.restype = i
    # include/rt_capi_adaptive.h (likewise absent from older builds)
    if hasattr(lib, "rt_render_adaptive"):
        lib.rt_capi_adaptive_version.restype = i
        lib.rt_adaptive_flags.argtypes = [i, C.POINTER(RtAdaptiveParams), i, i, vp, vp, vp]
        lib.rt_adaptive_flags_device.argtypes = [i, C.POINTER(RtAdaptiveParams), i, i, vp, vp, vp, vp]
        lib.rt_render_adaptive.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, C.POINTER(RtAdaptiveParams), vp, vp]
        lib.rt_render_adaptive_device.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, C.POINTER(RtAdaptiveParams), vp, vp,
                                                  vp]
        lib.rt_get_adaptive_info.argtypes = [vp, C.POINTER(RtAdaptiveInfo)]
        for name in ("rt_adaptive_flags", "rt_adaptive_flags_device", "rt_render_adaptive", "rt_render_adaptive_device",
                     "rt_get_adaptive_info"):
            getattr(lib, name).restype = i
    # include/rt_capi_lens.h (likewise absent from older builds)
    if hasattr(lib, "rt_render_lens"):
        lib.rt_capi_lens_version.restype = i
        lib.rt_lens_rays.argtypes = [C.POINTER(RtCameraDesc), i, i, i, i, C.POINTER(RtLensParams), i, vp]
        lib.rt_lens_rays_device.argtypes = [C.POINTER(RtCameraDesc), i, i, i, i, C.POINTER(RtLensParams), i, vp, vp]
        lib.rt_render_lens.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, C.POINTER(RtLensParams), vp]
        lib.rt_render_lens_device.argtypes = [vp, C.POINTER(RtCameraDesc), i, i, i, i, i, C.POINTER(RtLensParams), vp, vp]
        lib.rt_get_lens_info.argtypes = [vp, C.POINTER(RtLensInfo)]
        for name in ("rt_lens_rays", "rt_lens_rays_device", "rt_render_lens", "rt_render_lens_device", "rt_get_lens_info"):
            getattr(lib, name).restype = i
    # include/rt_capi_indirect.h (likewise absent from older builds)
    if hasattr(lib, "rt_indirect_diffuse"):
        lib.rt_capi_indirect_version.restype = i
        lib.rt_indirect_rays.argtypes = [C.POINTER(RtIndirectParams), i, vp, i, vp]
        lib.rt_indirect_rays_device.argtypes = [C.POINTER(RtIndirectParams), i, vp, i, vp, vp]
        lib.rt_indirect_diffuse.argtypes = [vp, C.POINTER(RtIndirectParams), i, vp, vp, vp]
        lib.rt_indirect_diffuse_device.argtypes = [vp, C.POINTER(RtIndirectParams), i, vp, vp, vp, vp]
        lib.rt_get_indirect_info.argtypes = [vp, C.POINTER(RtIndirectInfo)]
        for name in ("rt_indirect_rays", "rt_indirect_rays_device", "rt_indirect_diffuse", "rt_indirect_diffuse_device",
                     "rt_get_indirect_info"):
            getattr(lib, name).restype = i
    # include/rt_paths.h (likewise absent from older builds)
    if hasattr(lib, "rt_indirect_paths"):
        lib.rt_paths_version.restype = i
        lib.rt_indirect_paths.argtypes = [vp, C.POINTER(RtPathsParams), i, vp, vp, vp]
        lib.rt_indirect_paths_device.argtypes = [vp, C.POINTER(RtPathsParams), i, vp, vp, vp, vp]
        lib.rt_get_paths_info.argtypes = [vp, C.POINTER(RtPathsInfo)]
        for name in ("rt_indirect_paths", "rt_indirect_paths_device", "rt_get_paths_info"):
            getattr(lib, name).restype = i
    # include/rt_paths_compact.h (likewise)
    if hasattr(lib, "rt_indirect_paths_compact"):
        lib.rt_paths_compact_version.restype = i
        lib.rt_indirect_paths_compact.argtypes = [vp, C.POINTER(RtPathsParams), i, vp, vp, vp]
        lib.rt_indirect_paths_compact_device.argtypes = [vp, C.POINTER(RtPathsParams), i, vp, vp, vp, vp]
        lib.rt_get_paths_compact_info.argtypes = [vp, C.POINTER(RtPathsCompactInfo)]
        for name in ("rt_indirect_paths_compact", "rt_indirect_paths_compact_device", "rt_get_paths_compact_info"):
            getattr(lib, name).restype = i
    # include/rt_mirror.h (likewise absent from older builds)
    if hasattr(lib, "rt_mirror_records"):
        lib.rt_mirror_version.restype = i
        lib.rt_mirror_records.argtypes = [vp, C.POINTER(RtMirrorParams), i, i, vp, vp, vp, vp, vp]
        lib.rt_mirror_records_device.argtypes = [vp, C.POINTER(RtMirrorParams), i, i, vp, vp, vp, vp, vp, vp]
        lib.rt_get_mirror_info.argtypes = [vp, C.POINTER(RtMirrorInfo)]
        lib.rt_mirror_records.restype = lib.rt_mirror_records_device.restype = lib.rt_get_mirror_info.restype = i
    # include/rt_glass.h (likewise)
    if hasattr(lib, "rt_glass_records"):
        lib.rt_glass_version.restype = i
        lib.rt_glass_records.argtypes = [vp, C.POINTER(RtGlassParams), i, i, vp, vp, vp, vp, vp]
        lib.rt_glass_records_device.argtypes = [vp, C.POINTER(RtGlassParams), i, i, vp, vp, vp, vp, vp, vp]
        lib.rt_get_glass_info.argtypes = [vp, C.POINTER(RtGlassInfo)]
        lib.rt_glass_records.restype = lib.rt_glass_records_device.restype = lib.rt_get_glass_info.restype = i
    # include/rt_mirror_compact.h (likewise)
    if hasattr(lib, "rt_mirror_records_compact"):
        lib.rt_mirror_compact_version.restype = i
        lib.rt_mirror_records_compact.argtypes = [vp, C.POINTER(RtMirrorParams), i, i, vp, vp, vp, vp, vp]
        lib.rt_mirror_records_compact_device.argtypes = [vp, C.POINTER(RtMirrorParams), i, i, vp, vp, vp, vp, vp, vp]
        lib.rt_get_mirror_compact_info.argtypes = [vp, C.POINTER(RtMirrorCompactInfo)]
        lib.rt_mirror_records_compact.restype = lib.rt_mirror_records_compact_device.restype = i
        lib.rt_get_mirror_compact_info.restype = i
    # include/rt_glass_compact.h (likewise)
    if hasattr(lib, "rt_glass_records_compact"):
        lib.rt_glass_compact_version.restype = i
        lib.rt_glass_records_compact.argtypes = [vp, C.POINTER(RtGlassParams), i, i, vp, vp, vp, vp, vp]
        lib.rt_glass_records_compact_device.argtypes = [vp, C.POINTER(RtGlassParams), i, i, vp, vp, vp, vp, vp, vp]
        lib.rt_get_glass_compact_info.argtypes = [vp, C.POINTER(RtGlassCompactInfo)]
        lib.rt_glass_records_compact.restype = lib.rt_glass_records_compact_device.restype = i
        lib.rt_get_glass_compact_info.restype = i
    # include/rt_capi_upsample.h (likewise absent from older builds)
    if hasattr(lib, "rt_upsample_guided"):
        lib.rt_capi_upsample_version.restype = i
        lib.rt_subsample_hits.argtypes = [i, i, i, i, i, vp, vp]
        lib.rt_subsample_hits_device.argtypes = [i, i, i, i, i, vp, vp, vp]
        lib.rt_upsample_guided.argtypes = [i, C.POINTER(RtUpsampleParams), i, i, vp, vp, vp, vp, vp, C.POINTER(C.c_double)]
        lib.rt_upsample_guided_device.argtypes = [i, C.POINTER(RtUpsampleParams), i, i, vp, vp, vp, vp, vp, vp]
        for name in ("rt_subsample_hits", "rt_subsample_hits_device", "rt_upsample_guided", "rt_upsample_guided_device"):
            getattr(lib, name).restype = i
    # include/rt_temporal.h (likewise absent from older builds)
    if hasattr(lib, "rt_temporal_accumulate"):
        lib.rt_capi_temporal_version.restype = i
        head = [i, C.POINTER(RtTemporalParams), C.POINTER(RtCameraDesc), C.POINTER(RtCameraDesc), i, i, i, i] + [vp] * 11
        lib.rt_temporal_accumulate.argtypes = head + [C.POINTER(C.c_double)]
        lib.rt_temporal_accumulate_device.argtypes = head + [vp]
        lib.rt_temporal_accumulate.restype = lib.rt_temporal_accumulate_device.restype = i
    # include/rt_motion.h (likewise absent from older builds)
    if hasattr(lib, "rt_motion_accumulate"):
        lib.rt_capi_motion_version.restype = i
        head = [i, C.POINTER(RtTemporalParams), C.POINTER(RtCameraDesc), C.POINTER(RtCameraDesc), i, i, i, i, vp, i] + [vp] * 11
        lib.rt_motion_accumulate.argtypes = head + [C.POINTER(C.c_double)]
        lib.rt_motion_accumulate_device.argtypes = head + [vp]
        lib.rt_motion_accumulate.restype = lib.rt_motion_accumulate_device.restype = i
    # include/rt_svgf.h (likewise absent from older builds)
    if hasattr(lib, "rt_svgf_filter"):
        lib.rt_capi_svgf_version.restype = i
        lib.rt_svgf_filter.argtypes = [i, C.POINTER(RtSvgfParams), i, i] + [vp] * 7 + [C.POINTER(C.c_double)]
        lib.rt_svgf_filter_device.argtypes = [i, C.POINTER(RtSvgfParams), i, i] + [vp] * 9
        lib.rt_svgf_filter.restype = lib.rt_svgf_filter_device.restype = i
        lib.rt_svgf_scratch_bytes.argtypes = [C.POINTER(RtSvgfParams), i, i]
        lib.rt_svgf_scratch_bytes.restype = C.c_uint64
    # include/rt_clamp.h (likewise absent from older builds)
    if hasattr(lib, "rt_history_clamp"):
        lib.rt_capi_clamp_version.restype = i
        lib.rt_history_clamp.argtypes = [i, C.POINTER(RtClampParams), i, i] + [vp] * 10 + [C.POINTER(C.c_double)]
        lib.rt_history_clamp_device.argtypes = [i, C.POINTER(RtClampParams), i, i] + [vp] * 11
        lib.rt_history_clamp.restype = lib.rt_history_clamp_device.restype = i
    # include/rt_gradient.h (likewise absent from older builds)
    if hasattr(lib, "rt_gradient_reweight"):
        lib.rt_capi_gradient_version.restype = i
        lib.rt_gradient_reweight.argtypes = [i, C.POINTER(RtGradientParams), i, i] + [vp] * 15 + [C.POINTER(C.c_double)]
        lib.rt_gradient_reweight_device.argtypes = [i, C.POINTER(RtGradientParams), i, i] + [vp] * 16
        lib.rt_gradient_reweight.restype = lib.rt_gradient_reweight_device.restype = i
    # include/rt_capi_launch.h (likewise absent from older builds)
    if hasattr(lib, "rt_get_launch_kernel"):
        lib.rt_capi_launch_version.restype = i
        lib.rt_get_launch_kernel.argtypes = [vp, C.c_char_p, i]
        lib.rt_get_launch_kernel.restype = i
    for name in ("rt_device_count", "rt_scene_create", "rt_scene_destroy", "rt_render",
                 "rt_render_device", "rt_render_multi", "rt_render_stats", "rt_learn_tile_order", "rt_get_timing", "rt_reset_timing",
                 "rt_get_launch_info", "rt_set_option", "rt_chunk_bounds", "rt_multi_create", "rt_multi_render",
                 "rt_multi_set_option", "rt_multi_destroy", "rt_multi_set_bounds", "rt_multi_get_info", "rt_balance_strips",
                 "rt_suggest_chunks", "rt_shared_image_create", "rt_shared_image_open", "rt_shared_image_close",
                 "rt_shared_image_destroy"):
        getattr(lib, name).restype = i
    _lib = lib
    return lib


def primary_rectangles(desc, camera, W, H):
    """rt_primary_rectangles (include/rt_capi_tuning.h, no device needed): the PRIMARY table a W x H launch of the scene
    description under the camera would get, as a list of RtPrimaryItem; empty when the launch would get none"""
    items = (RtPrimaryItem * RT_PRIMARY_ITEMS_MAX)()
    n = C.c_int(0)
    check(load_library().rt_primary_rectangles(desc, camera, W, H, items, RT_PRIMARY_ITEMS_MAX, C.byref(n)))
    return list(items[:n.value])


def check(rc):
    if rc != RT_OK:
        msg = load_library().rt_last_error()
        raise RtError(rc, msg.decode("utf-8", "replace") if msg else "")
