"""The kernel matrix: one case per render kernel of the catalogue (csrc/rt_tables.h, RENDER KERNELS), table mode times family --
the scene and options that select the mode, the shading that selects the family, and the call that launches it.
test_kernel_matrix_gpu.py runs every case against the references; test_capi_library.py checks, without a device, that the
cases are exactly the catalogue.  Plain data: neither torch nor a device is needed to read it."""
from collections import namedtuple

# mode -> (scene, options): the built-in scene (FAST tables and a PRIMARY table; "fast" = 0 for the item tables) or a field of
# clustered spheres (the same field with its tables in global memory for _large, whose leaf items are then read from there)
MODES = {
    "": ("builtin", {}),
    "_items": ("builtin", {"fast": 0}),
    "_large": ("field", {"tables": 2}),
    "_clusters": ("field", {"wide": 0}),
    "_clusters_wide": ("field", {"wide": 1}),
}

# the colour families: call suffix -> call; shading suffix -> what the scene carries (rt_capi.hip, family())
CALLS = {"": "render", "_ssaa": "ssaa", "_rays": "rays", "_gbuffer": "gbuffer"}
SHADINGS = ("", "_image", "_refract", "_soft", "_refract_soft")

DEPTH = 3            # every case
DEEP = 8             # the _refract cases also render at this depth with the bounce stack in HBM (option "stack" = 2)

Case = namedtuple("Case", "mode family scene options call shading deep")


def _query_shading(mode, family):
    """The queries answer geometry: a nearest-hit query of any shaded scene runs *_hits_image, an occlusion query *_occluded.
    So _hits_image runs on the image scene, and on the clustered fields on the scene with glass and area lights; _occluded on the
    plain scenes, and once on a clustered field packed as an image scene (glass and area lights)."""
    clustered = mode.startswith("_clusters")
    if family == "_hits":
        return ""
    if family == "_hits_image":
        return "_refract_soft" if clustered else "_image"
    if family == "_occluded":
        return "_refract_soft" if mode == "_clusters" else ""
    raise KeyError(family)


def families():
    """every family suffix with its call and its shading (None: a query, _query_shading())"""
    out = [(c + s, call, s) for s in SHADINGS for c, call in CALLS.items()]
    out += [("_hits", "hits", None), ("_occluded", "occluded", None), ("_hits_image", "hits", None)]
    return out


def cases():
    out = []
    for mode, (scene, options) in MODES.items():
        for family, call, shading in families():
            if shading is None:
                shading = _query_shading(mode, family)
            out.append(Case(mode, family, scene, dict(options), call, shading, family == "_refract"))
    return out


CASES = cases()


def kernel_name(case):
    return "rt_render_kernel" + case.mode + case.family


def case_id(case):
    return (case.mode or "fast") + ":" + (case.family or "plain")
