"""The PRIMARY table (csrc/rt_capi.hip: primary_table()) under cameras the built-in scenes never have, without a GPU.

rt_primary_rectangles (include/rt_capi_tuning.h) returns the table a launch would get: per item of the FAST list its object, the
pixel rectangle outside which the camera rays' scan skips it, and its entry distance.  The reference is query_ref._collision --
the hit mask and distance of the reference's float tests, object by object -- on rays_ref.camera_rays: neither is the code under
test.  The property (CONSERVATIVE): every pixel whose ray the reference reports as hitting an item's object lies inside the item's
rectangle, and the item's entry distance is 0 or at most that hit's distance.  It is checked for every camera of
cameras.catalogue() on the built-in scene and on scene_gen.build_room(206), for 540 seeded random cameras, and for the frames of
2 x 2 and 4 x 4 supersampling; the catalogue is held to what its names promise, and the table to a bound on its slack."""
import ctypes as C
import functools

import numpy as np
import pytest

import cameras
import oracle_lib
import query_ref
from rays_ref import camera_rays
from scene_gen import build_random
from tilecoderaytracer_amd import HostScene, capi

SHAPES = [(61, 47), (200, 31), (17, 300), (128, 128)]     # no tile multiples but the last; a wide flat frame, a tall narrow one
W0, H0 = 90, 70                                           # the frame of the catalogue's own checks and of test_cameras_gpu.py
SCENES = ("builtin", "room206")


@functools.lru_cache(maxsize=None)
def scene(name):
    """(HostScene, query_ref.Scene) of a catalogue scene or of "random<seed>" (scene_gen.build_random)"""
    if name.startswith("random"):
        seed = int(name[6:])
        host, orc = build_random(HostScene.empty(), seed), build_random(oracle_lib.OracleScene(), seed)
    else:
        host, orc = cameras.scene_pair(name, HostScene, oracle_lib.OracleScene)
    return host, query_ref.Scene(orc)


def table(host, cam, W, H):
    """rt_primary_rectangles -> a record array (object, x_lo, x_hi, z_lo, z_hi, entry), one record per item"""
    items = capi.primary_rectangles(host.desc, C.byref(cam), W, H)
    return np.array([(t.object, t.x_lo, t.x_hi, t.z_lo, t.z_hi, t.entry) for t in items],
                    dtype=[("object", "i4"), ("x_lo", "i4"), ("x_hi", "i4"), ("z_lo", "i4"), ("z_hi", "i4"), ("entry", "f4")])


def reference_hits(qs, cam, W, H, objects):
    """per object of `objects`: (hit mask, distance), both (W, H), of the frame's camera rays"""
    rays = camera_rays(cam, W, H).reshape(-1, 6)
    E, d = rays[:, :3], query_ref.directions(rays)
    out = {}
    for k in objects:
        hit, dist = query_ref._collision(qs.objects[k], E, d, False)
        out[k] = (hit.reshape(W, H), dist.reshape(W, H))
    return out


def violations(t, hits, W, H):
    """pixels the reference hits an item's object at that the table would skip the item at -> a list of descriptions"""
    xs, zs = np.arange(W)[:, None], np.arange(H)[None, :]
    bad = []
    for it in t:
        hit, dist = hits[int(it["object"])]
        inside = (xs >= it["x_lo"]) & (xs <= it["x_hi"]) & (zs >= it["z_lo"]) & (zs <= it["z_hi"])
        with np.errstate(invalid="ignore"):
            ok = inside & ((it["entry"] == 0) | (dist >= it["entry"]))
        if (hit & ~ok).any():
            x, z = np.argwhere(hit & ~ok)[0]
            bad.append(f"object {it['object']}: rectangle x {it['x_lo']}..{it['x_hi']} z {it['z_lo']}..{it['z_hi']} entry "
                       f"{it['entry']}: {(hit & ~ok).sum()} hit pixels skipped, first ({x}, {z}) at distance {dist[x, z]}")
    return bad


def assert_conservative(name, cam, W, H, what):
    """-> the table (empty: none can be made)"""
    host, qs = scene(name)
    t = table(host, cam, W, H)
    if len(t):
        assert sorted(t["object"].tolist()) == sorted(set(t["object"].tolist())), what      # one item per object here
        bad = violations(t, reference_hits(qs, cam, W, H, t["object"].tolist()), W, H)
        assert not bad, f"{what}, {W} x {H}: " + "; ".join(bad)
    return t


CATALOGUE = [(s, c) for s in SCENES for c in cameras.catalogue(s)]


@pytest.mark.parametrize("name,camera", CATALOGUE, ids=[f"{s}-{c}" for s, c in CATALOGUE])
def test_catalogue_tables_are_conservative(name, camera):
    cam = cameras.catalogue(name)[camera]
    for W, H in SHAPES[:3] + [(W0, H0)]:
        t = assert_conservative(name, cam, W, H, f"{name} {camera}")
        assert (len(t) == 0) == (camera in cameras.DEGENERATE), f"{name} {camera}: {len(t)} items"


@pytest.mark.parametrize("name,camera", [(s, c) for s in SCENES for c in ("left_handed", "off_centre", "oblique", "behind_screen")])
@pytest.mark.parametrize("k", [2, 4])
def test_supersampled_frames_get_a_conservative_table(name, camera, k):
    """a k x k supersampled launch of a W x H frame makes its table for kW x kH: the rectangles of the frame of samples"""
    W, H = 37, 29
    t = assert_conservative(name, cameras.catalogue(name)[camera], k * W, k * H, f"{name} {camera} k {k}")
    assert len(t)


def random_camera(rng, qs):
    """a camera aimed at a random object from 0.002 to 2e4 units away: any roll, screens 1e-3 to 40 wide, 1e-3 to 100 before the
    eye, off-centre, skewed, scaled and mirrored ones"""
    o = qs.objects[int(rng.integers(len(qs.objects)))]
    p = o.origin if o.kind == query_ref.SPHERE else o.plane_origin
    target = np.array([p.x, p.y, p.z], dtype=np.float64)
    target = np.where(np.isfinite(target), target, 0.0)
    direction = rng.normal(size=3)
    eye = target + direction / np.linalg.norm(direction) * rng.choice([0.002, 0.05, 0.3, 1.5, 4.0, 9.0, 300.0, 2.0e4])
    return cameras.camera(eye, target, screen=(rng.choice([1e-3, 0.3, 1.0, 2.5, 40.0]), rng.choice([0.5, 1.0, 3.0])),
                          dist=rng.choice([1e-3, 0.2, 1.0, 4.0, 100.0]), roll=rng.uniform(-3.1, 3.1),
                          centre=(rng.choice([0.5, 0.5, 0.1, 1.3]), rng.choice([0.5, 0.5, -0.2, 0.9])),
                          skew=rng.choice([0.0, 0.0, 0.4]), hscale=rng.choice([1.0, 1.0, 0.5, 3.0]),
                          left_handed=bool(rng.integers(2)))


RANDOM_SCENES = ("room206", "random5", "random9")
RANDOM_PER_SCENE = 180


@functools.lru_cache(maxsize=None)
def sweep(name):
    """RANDOM_PER_SCENE seeded random cameras on a scene -> (the violations' descriptions, the cameras without a table)"""
    host, qs = scene(name)
    rng = np.random.default_rng(1000 + RANDOM_SCENES.index(name))
    bad, none = [], 0
    for i in range(RANDOM_PER_SCENE):
        cam = random_camera(rng, qs)
        W, H = SHAPES[i % 4]
        t = table(host, cam, W, H)
        none += len(t) == 0
        if len(t):
            bad += [f"camera {i}, {W} x {H}: {b}" for b in violations(t, reference_hits(qs, cam, W, H, t["object"].tolist()), W, H)]
    return bad, none


@pytest.mark.parametrize("name", RANDOM_SCENES)
def test_random_cameras_get_conservative_tables(name):
    bad, _ = sweep(name)
    assert not bad, f"{name}: {len(bad)} violations: " + "; ".join(bad[:5])


def test_few_random_cameras_are_refused():
    """the cameras primary_table() makes no table for (the kernel then culls by the bundle of rays) are at most 15 % of the
    random ones: a table that refused most cameras would be conservative too"""
    none = {name: sweep(name)[1] for name in RANDOM_SCENES}
    total = len(RANDOM_SCENES) * RANDOM_PER_SCENE
    print(f"no table for {none} of {RANDOM_PER_SCENE} cameras each")
    assert total >= 500 and sum(none.values()) <= 0.15 * total, none


# ---- the catalogue reaches what it names ------------------------------------------------------------------------------------

def _tables(name):
    return {c: table(scene(name)[0], cam, W0, H0) for c, cam in cameras.catalogue(name).items() if c not in cameras.DEGENERATE}


def _empty(t):
    return (t["x_lo"] > t["x_hi"]) | (t["z_lo"] > t["z_hi"])


def _whole(t):
    return (t["x_lo"] <= 0) & (t["x_hi"] >= W0 - 1) & (t["z_lo"] <= 0) & (t["z_hi"] >= H0 - 1)


def _eye_depths(qs, cam, k):
    """the least and greatest depth before the eye (along the viewing axis, in units of the eye's distance from the screen:
    primary_table()'s u0) of the corners of object k's bounding box (None: unbounded), and the least distance in world units"""
    o = qs.objects[k]
    if o.kind == query_ref.SPHERE:
        c, r = np.array(o.origin.tuple(), dtype=np.float64), float(o.radius)
        corners = c + r * np.array([[i, j, l] for i in (-1, 1) for j in (-1, 1) for l in (-1, 1)], dtype=np.float64)
    elif o.kind == query_ref.FINITE_PLANE:
        p, h, v = (np.array(x.tuple(), dtype=np.float64) for x in (o.plane_origin, o.horizontal, o.vertical))
        corners = np.array([p + i * h * o.h_distance + j * v * o.v_distance for i in (0, 1) for j in (0, 1)])
    else:
        return None
    eye, so = np.array(list(cam.eye_origin)), np.array(list(cam.screen_origin))
    m = np.array([so - eye, list(cam.vector_horizontal), list(cam.vector_vertical)], dtype=np.float64).T
    u0 = np.linalg.solve(m, (corners - eye).T)[0]
    axis = (so - eye) / np.linalg.norm(so - eye)
    return u0.min(), u0.max(), ((corners - eye) @ axis).min()


@pytest.mark.parametrize("name", SCENES)
def test_the_catalogue_reaches_what_it_names(name):
    """From the function's output, so that a later change of a scene cannot quietly empty a case."""
    host, qs = scene(name)
    cams, tables = cameras.catalogue(name), _tables(name)
    every = np.concatenate(list(tables.values()))
    # wholly behind the eye: no pixel
    assert any(_empty(t).any() for c, t in tables.items()), "no item with an empty rectangle"
    assert _empty(tables["among"]).sum() >= 3, "the eye among the objects has few of them behind it"
    # straddling the eye plane, and still a proper sub-rectangle
    straddling = 0
    for c, t in tables.items():
        for it in t:
            depths = _eye_depths(qs, cams[c], int(it["object"]))
            if depths and depths[0] < 0.0 < depths[1] and not _empty(t[t["object"] == it["object"]])[0] \
                    and not _whole(t[t["object"] == it["object"]])[0] and it["entry"] > 0:
                straddling += 1
    assert straddling >= 3, f"{straddling} items across the eye plane with a proper sub-rectangle"
    # rectangles that leave the image on every side
    proper = every[~_empty(every)]
    assert (proper["x_lo"] < 0).any() and (proper["x_hi"] >= W0).any() and (proper["z_lo"] < 0).any() and (proper["z_hi"] >= H0).any()
    partly = proper[~_whole(proper)]
    assert (partly["x_lo"] < 0).any() and (partly["x_hi"] >= W0).any() and (partly["z_lo"] < 0).any() and (partly["z_hi"] >= H0).any()
    # the eye inside an item's grown box: the whole image, always tested
    for c in cameras.EYE_INSIDE:
        t = tables[c]
        assert (_whole(t) & (t["entry"] == 0)).any(), f"{c}: no whole-image item with entry distance 0"
        assert not (_whole(t) & (t["entry"] == 0)).all(), f"{c}: every item is a whole-image item"
        kinds = {qs.objects[int(k)].kind for k in t["object"][_whole(t) & (t["entry"] == 0)]}
        assert query_ref.FINITE_PLANE in kinds, f"{c}: the eye is in no finite rectangle's grown box"
        if name == "builtin":                   # (the room of build_room(206) has no infinite plane)
            assert query_ref.INFINITE_PLANE in kinds, f"{c}: the eye is not within the slack of the infinite floor's slab"
    # a positive entry distance on everything wholly more than a unit before the eye
    ahead = 0
    for c, t in tables.items():
        for it in t:
            depths = _eye_depths(qs, cams[c], int(it["object"]))
            if depths and depths[0] > 0.0 and depths[2] > 1.0:
                ahead += 1
                assert it["entry"] > 0, f"{c}: object {it['object']} is {depths[2]} before the eye and has entry distance 0"
    assert ahead >= 50, ahead
    # the off-centre screen: the eye's axis (pixel 0.1 W, 1.3 H) is outside the image
    assert float(cams["off_centre"].screen_halfheight) > float(cams["off_centre"].screen_height)
    # the far eye: the float error of a pixel's screen point is more than a pixel (primary_table()'s err, restated)
    cam = cams["far"]
    mag = sum(abs(cam.screen_origin[k]) + abs(cam.eye_origin[k]) + abs(cam.vector_horizontal[k]) * (abs(cam.screen_halfwidth) + cam.screen_width) +
              abs(cam.vector_vertical[k]) * (abs(cam.screen_halfheight) + cam.screen_height) for k in range(3))
    assert 16.0 * 1.2e-7 * mag * W0 / cam.screen_width > 1.0


# ---- not trivially conservative -----------------------------------------------------------------------------------------------

# Total area of the rectangles, clipped to the 90 x 70 image, over the total area of the bounding rectangles of the items'
# reference hit pixels (items the reference hits nowhere add to the first sum only).  Measured on the table of commit 068d5f8
# ("Share the per-ray steps of render_tile() and render_tile_twin()"), whose host arithmetic is double and deterministic; the test
# allows 1.25 times these: a change of slack or margin moves them by a few per cent, a table that answers "the whole image" for
# everything by far more (the second figure: what that table would give).
TIGHTNESS = {
    "builtin": {
        "pitched_down": (1.524, 9.1), "pitched_up": (1.576, 6.8), "rolled_pi": (1.683, 11.3), "rolled_1p45": (1.764, 11.0),
        "left_handed": (1.677, 11.3), "off_centre": (1.229, 15.8), "oblique": (1.657, 11.9), "wide": (1.792, 12.3),
        "narrow": (2.514, 16.0), "behind_screen": (1.541, 10.4), "among": (1.901, 17.0), "far": (2.120, 17.5),
        "inside_box": (3.139, 15.8),
    },
    "room206": {
        "pitched_down": (1.816, 19.6), "pitched_up": (1.270, 10.9), "rolled_pi": (1.711, 18.3), "rolled_1p45": (1.568, 14.6),
        "left_handed": (1.725, 18.7), "off_centre": (1.618, 29.8), "oblique": (1.835, 18.1), "wide": (1.520, 20.2),
        "narrow": (1.000, 11.0), "behind_screen": (1.287, 9.8), "among": (1.385, 9.3), "far": (21.084, 39.8),
        "inside_box": (2.252, 20.5), "coarse_pixels": (12.082, 12.1),     # (whole images: the margins are wider than the image)
    },
}


def tightness(name, camera):
    """-> (the ratio, the ratio of a table of whole images)"""
    host, qs = scene(name)
    cam = cameras.catalogue(name)[camera]
    t = table(host, cam, W0, H0)
    hits = reference_hits(qs, cam, W0, H0, t["object"].tolist())
    area = bound = 0
    for it in t:
        x0, x1 = max(int(it["x_lo"]), 0), min(int(it["x_hi"]), W0 - 1)
        z0, z1 = max(int(it["z_lo"]), 0), min(int(it["z_hi"]), H0 - 1)
        area += max(x1 - x0 + 1, 0) * max(z1 - z0 + 1, 0)
        xz = np.argwhere(hits[int(it["object"])][0])
        if len(xz):
            bound += (xz[:, 0].max() - xz[:, 0].min() + 1) * (xz[:, 1].max() - xz[:, 1].min() + 1)
    return area / max(bound, 1), len(t) * W0 * H0 / max(bound, 1)


TIGHT_CASES = [(s, c) for s, c in CATALOGUE if c not in cameras.DEGENERATE]


@pytest.mark.parametrize("name,camera", TIGHT_CASES, ids=[f"{s}-{c}" for s, c in TIGHT_CASES])
def test_rectangles_are_not_much_larger_than_what_is_hit(name, camera):
    ratio, whole = tightness(name, camera)
    measured = TIGHTNESS[name][camera][0]
    print(f"{name} {camera}: ratio {ratio:.4f} (recorded {measured}, whole images {whole:.3f})")
    assert ratio <= 1.25 * measured, (ratio, measured)


def test_the_count_comes_whatever_the_capacity():
    """rt_primary_rectangles: *n_items is the table's size, out[] receives the first `cap` items and nothing beyond them"""
    host, _ = scene("builtin")
    cam = cameras.catalogue("builtin")["oblique"]
    whole = capi.primary_rectangles(host.desc, C.byref(cam), W0, H0)
    lib, n = capi.load_library(), C.c_int(-1)
    assert lib.rt_primary_rectangles(host.desc, C.byref(cam), W0, H0, None, 0, C.byref(n)) == capi.RT_OK and n.value == len(whole) == 32
    few = (capi.RtPrimaryItem * 6)()
    few[5].object = -7
    assert lib.rt_primary_rectangles(host.desc, C.byref(cam), W0, H0, few, 5, C.byref(n)) == capi.RT_OK and n.value == 32
    assert few[5].object == -7
    assert [(t.object, t.x_lo, t.x_hi, t.z_lo, t.z_hi, t.entry) for t in few[:5]] == \
           [(t.object, t.x_lo, t.x_hi, t.z_lo, t.z_hi, t.entry) for t in whole[:5]]
    assert lib.rt_primary_rectangles(host.desc, C.byref(cam), W0, H0, None, 5, C.byref(n)) == capi.RT_ERR_INVALID
    assert lib.rt_primary_rectangles(host.desc, C.byref(cam), 0, H0, few, 5, C.byref(n)) == capi.RT_ERR_INVALID and n.value == 0
