"""Ray queries (include/rt_capi_query.h) without a GPU: the header, the exported symbols, the check that comes before any device
is touched, and the reference the GPU tests lean on -- query_ref's restatement pinned to the oracle's frames through the object
and colour identities."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib
import query_ref
import scene_gen
from rays_ref import camera_rays, oracle_trace, positive_zeros
from tilecoderaytracer_amd import capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rt_capi_query.h")
FUNCTIONS = ["rt_capi_query_version", "rt_intersect_rays", "rt_intersect_rays_device", "rt_occluded_rays",
             "rt_occluded_rays_device"]


def declared_functions(path):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|const char \*)\s*(rt_\w+)\s*\(", text, flags=re.M)))


def test_header_declares_exactly_its_functions():
    assert declared_functions(HEADER) == FUNCTIONS
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert text.count("(") == 5                              # five prototypes, one parenthesis each


def test_header_is_plain_c99(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "query.c"
    src.write_text('#include "rt_capi_query.h"\n'
                   "#include <stddef.h>\n"
                   "static int (*const f)(rt_scene *, int, int, const float *, rt_hit *) = rt_intersect_rays;\n"
                   "static int (*const g)(rt_scene *, int, int, const void *, void *, void *) = rt_intersect_rays_device;\n"
                   "static int (*const h)(rt_scene *, int, int, const float *, uint8_t *) = rt_occluded_rays;\n"
                   "static int (*const k)(rt_scene *, int, int, const void *, void *, void *) = rt_occluded_rays_device;\n"
                   "typedef char size_ok[sizeof(rt_hit) == 48 && offsetof(rt_hit, normal) == 20 ? 1 : -1];\n"
                   "int main(void) { return (RT_CAPI_QUERY_VERSION == 1 && f && g && h && k) ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-Wno-unused-local-typedefs",
                        "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_hit_dtype_mirrors_rt_hit():
    assert HIT_DTYPE.itemsize == 48 and HIT_DTYPE == query_ref.HIT_DTYPE
    assert [HIT_DTYPE.fields[k][1] for k in ("object", "distance", "point", "normal", "color", "flags")] == [0, 4, 8, 20, 32, 44]


def test_library_exports_the_symbols_and_the_version():
    lib = capi.load_library()
    for name in FUNCTIONS:
        assert hasattr(lib, name), name
    macro = int(re.search(r"#define RT_CAPI_QUERY_VERSION (\d+)", open(HEADER).read()).group(1))
    assert lib.rt_capi_query_version() == macro == 1


def test_null_scene_is_invalid():
    lib = capi.load_library()
    rays = np.zeros((4, 6), dtype=np.float32)
    hits = np.zeros(4, dtype=HIT_DTYPE)
    blocked = np.zeros(4, dtype=np.uint8)
    for fn, out in ((lib.rt_intersect_rays, hits), (lib.rt_occluded_rays, blocked)):
        assert fn(None, 4, 4, rays.ctypes.data, out.ctypes.data) == capi.RT_ERR_INVALID
        assert b"scene" in lib.rt_last_error()
        assert fn(None, -1, 0, None, None) == capi.RT_ERR_INVALID           # the scene first
        assert b"scene" in lib.rt_last_error()
    for fn in (lib.rt_intersect_rays_device, lib.rt_occluded_rays_device):
        assert fn(None, 4, 4, None, None, None) == capi.RT_ERR_INVALID
        assert b"scene" in lib.rt_last_error()
    assert (hits["object"] == 0).all() and (blocked == 0).all()


# ---- query_ref pinned to the oracle ----------------------------------------------------------------------------------------

def builder(name):
    return lambda: oracle_lib.OracleScene.named(name)


def random_builder(seed):
    def build():
        return scene_gen.build_random(oracle_lib.OracleScene(), seed)
    return build


def incoherent_rays(build, n=600, seed=0):
    """Rays from inside spheres, from on planes, grazing the objects, and from far outside in random directions."""
    rng = np.random.RandomState(seed)
    o = build()
    objs = [o.get_object(i) for i in range(o.object_count)]
    spheres = [b for b in objs if b.kind == 0]
    planes = [b for b in objs if b.kind != 0]
    rays = []
    for k in range(n):
        kind = k % 4
        if kind == 0 and spheres:                                         # inside a sphere
            s = spheres[rng.randint(len(spheres))]
            E = np.array(s.origin.tuple()) + rng.uniform(-0.5, 0.5, 3) * s.radius
            T = E + rng.normal(size=3)
        elif kind == 1 and planes:                                        # on a plane
            p = planes[rng.randint(len(planes))]
            base = p.plane_origin if p.kind == 2 else p.origin
            E = np.array(base.tuple()) + rng.uniform(0, 2) * np.array(p.horizontal.tuple()) + \
                rng.uniform(0, 2) * np.array(p.vertical.tuple())
            T = E + rng.normal(size=3)
        elif kind == 2 and spheres:                                       # grazing a sphere
            s = spheres[rng.randint(len(spheres))]
            c = np.array(s.origin.tuple())
            E = c + rng.normal(size=3) * 20
            axis = c - E
            side = np.cross(axis, rng.normal(size=3))
            side /= np.linalg.norm(side)
            T = c + side * s.radius * rng.uniform(0.98, 1.02)
        else:                                                             # outside, anywhere
            E = rng.uniform(-30, 30, 3)
            T = E + rng.normal(size=3)
        rays.append(np.concatenate([E, T]))
    return np.array(rays, dtype=np.float32)


CASES = [("builtin", 24, 18), ("grid16", 20, 16), ("twomirrors", 24, 18)]


def check_identities(build, rays):
    scene = query_ref.Scene(build())
    got = query_ref.intersect(scene, rays)
    want_obj = query_ref.oracle_objects(build, rays)
    assert np.array_equal(got["object"], want_obj), np.argwhere(got["object"] != want_obj)[:5]
    want_rgb = query_ref.oracle_colours(build, rays)
    hit = got["object"] >= 0
    assert np.array_equal(got["color"][hit].view(np.uint32), want_rgb[hit].view(np.uint32))
    return got


@pytest.mark.parametrize("name,W,H", CASES)
def test_query_ref_matches_the_oracle_on_camera_rays(oracle, name, W, H):
    rays = camera_rays(oracle_lib.OracleScene.named(name).cam, W, H)
    got = check_identities(builder(name), rays)
    assert (got["object"] >= 0).any()


@pytest.mark.parametrize("name", ["builtin", "grid16", "twomirrors"])
def test_query_ref_matches_the_oracle_on_incoherent_rays(oracle, name):
    got = check_identities(builder(name), incoherent_rays(builder(name)))
    assert (got["flags"] & 1).any() or name == "twomirrors"        # some inside hits where there are spheres to be inside


@pytest.mark.parametrize("seed", [3, 11, 29])
def test_query_ref_matches_the_oracle_on_random_scenes(oracle, seed):
    build = random_builder(seed)
    rays = np.concatenate([camera_rays(build().cam, 16, 12).reshape(-1, 6), incoherent_rays(build, 200, seed)])
    check_identities(build, rays)


def test_occlusion_pin_lit_pixels_are_unblocked(oracle):
    """One light, plain diffuse materials: wherever the oracle's depth-0 pixel is lit (> 0), the segment from query_ref's hit
    point to the light is unblocked -- the shading saw the light from there."""
    o = oracle_lib.OracleScene()
    light = o.add_sphere((0.0, 10.0, 12.0), 0.2)
    o.set_light(light)
    o.add_infinite_plane((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    for k, (x, y, z, r) in enumerate([(-2.0, 12.0, 1.0, 1.0), (1.5, 9.0, 2.0, 0.8), (0.5, 14.0, 3.5, 1.4), (3.0, 11.0, 1.0, 0.6)]):
        i = o.add_sphere((x, y, z), r)
        o.set_specular(i, 0.0)
    o.set_object_indices(0, 1)
    o.camera_two_mirrors()
    W, H = 40, 30
    rays = camera_rays(o.cam, W, H)
    rgb = oracle_trace(o, positive_zeros(rays), 0)
    hits = query_ref.intersect(query_ref.Scene(o), rays)
    L = np.array(o.get_object(light).origin.tuple(), dtype=np.float32)
    lit = (rgb > 0).any(axis=-1) & (hits["object"] > light) & ((hits["flags"] & 2) == 0)
    segs = np.concatenate([hits["point"], np.broadcast_to(L, hits["point"].shape)], axis=-1).astype(np.float32)
    blocked = query_ref.occluded(query_ref.Scene(o), segs)
    assert lit.sum() > 50 and (~lit).sum() > 50
    assert not blocked[lit].any()
    # and the shadows are there: some unlit hit points face the light and are blocked
    assert blocked[(hits["object"] > light) & ~lit].any()
