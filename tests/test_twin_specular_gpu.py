"""SPECULAR GATE of the twin tiles (csrc/rt_kernel.hip, render_tile_twin()): a (ray, light) region of rt_render_kernel skips the
specular term where every lane that runs it has specular factor +-0 and the scene's light colours are finite.

Every case asserts that the launch's kernel is rt_render_kernel and compares every pixel with two references, as
test_twin_tiles_gpu.py does: the CPU oracle, and the same handle with option "fast" = 0 (rt_render_kernel_items, one tile per
wavefront, no gate).  Bits, except that a NaN equals a NaN (the scene with an infinite light colour makes them).  The frames:
exactly one twin, an odd number of tile rows (the last twin's second tile does not exist) and partial tiles on both axes --
16 x 8, 48 x 20 and 33 x 9 under tiles of 16 columns by 4 rows (option "tile_z" 4), and the same three situations under the
shape the launches choose themselves, 4 columns by 16 rows: 4 x 32, 12 x 80 and 9 x 33; depths 0, 1 and 4.  The scenes are
the ones a gate can get wrong: regions that are all factor 0, all live and mixed lane by lane; a live side without a diffuse
term (a gate keyed on the wrong factor skips it); zeros of either sign and the smallest factor that is not one; light colours
whose products with +-0 are +0, -0 and +-0 of a huge number -- and one that is infinite, where nothing may be skipped."""
import numpy as np
import pytest

from tilecoderaytracer_amd import HostScene, Renderer

pytestmark = pytest.mark.gpu

TWIN, SINGLE = b"rt_render_kernel", b"rt_render_kernel_items"
SIZES = [(16, 8, 4), (48, 20, 4), (33, 9, 4), (4, 32, 16), (12, 80, 16), (9, 33, 16)]      # W, H, tile_z
DEPTHS = [0, 1, 4]


def assert_same(got, want, what):
    assert got.shape == want.shape, what
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        bad = np.argwhere(~same.all(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at {bad[0].tolist()}: "
                             f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def check(r, want, W, H, tile_z, depth, what):
    r.set_option("tile_z", tile_z)
    got = r.render(W, H, depth)
    li = r.launch_info()
    assert li.kernel == TWIN and (li.tile_x, li.tile_z) == (64 // tile_z, tile_z)
    assert_same(got, want, what + ": oracle")
    r.set_option("fast", 0)
    try:
        items = r.render(W, H, depth)
        assert r.launch_info().kernel == SINGLE
    finally:
        r.set_option("fast", 1)
    assert_same(got, items, what + ": item tables")
    return got


def _lights(s):
    return [i for i in range(s.object_count) if s.get_object(i).is_light]


def museum(s):
    return s


def museum_no_specular(s):
    for i in range(s.object_count):
        s.set_specular(i, 0.0)
    return s


def museum_tiny_factors(s):
    """-0.0, the smallest denormal, and the museum's own factor, object by object"""
    for i in range(s.object_count):
        if i % 3 != 2:
            s.set_specular(i, (-0.0, 1e-45)[i % 3])
    return s


def museum_light_colours(s, lights):
    for n, i in enumerate(lights):
        s.set_color(i, ((0.0, -1.0, 1e30), (1e30, 0.0, -1.0))[n % 2])
    return s


def museum_infinite_light(s, lights):
    s.set_color(lights[-1], (1.0, float("inf"), 0.5))
    return s


def _unit(v):
    return v / np.linalg.norm(v)


def wall(s, eye_ray, seam):
    """Seen by the default camera: a wall of two finite planes square to the central ray, five units away, factor 0 on one side
    of the seam and 0.5 on the other, a little mirror-like; a light just behind the eye, so that V.R is near 1 all over the wall,
    and a second one to the side.  seam ("x" | "z", position as a fraction of the frame): x = 7.5 / 16 runs through the middle of
    both tiles of a 16 x 8 frame (tiles of 16 x 4) -- every region has lanes of both factors -- z = 3.5 / 8 between the twin's
    two tiles, z = 1.5 / 8 through the middle of the first."""
    axis, at = seam
    o = np.array(eye_ray(0.5, 0.5)[0], dtype=np.float64)
    dc = _unit(np.array(eye_ray(0.5, 0.5)[1], dtype=np.float64))

    def on_wall(dx, dz):
        d = _unit(np.array(eye_ray(dx, dz)[1], dtype=np.float64))
        return o + d * (5.0 / d.dot(dc))

    for centre in (o - 1.0 * dc, on_wall(-0.5, 0.5) - 3.0 * dc):
        s.set_light(s.add_sphere(tuple(centre), 0.15))
    lo, hi = -1.0, 2.0                       # the wall reaches a frame's width beyond the frame on every side
    for factor, (a, b) in ((0.0, (lo, at)), (0.5, (at, hi))):                # (the live side has NO diffuse term)
        if axis == "x":
            corner, vcorner, hcorner = on_wall(a, lo), on_wall(a, hi), on_wall(b, lo)
        else:
            corner, vcorner, hcorner = on_wall(lo, a), on_wall(lo, b), on_wall(hi, a)
        i = s.add_finite_plane_corners(tuple(corner), tuple(vcorner), tuple(hcorner))
        s.set_specular(i, factor)
        s.set_diffuse(i, 0.0 if factor else 0.7)
        s.set_reflective(i, 0.25)
        s.set_color(i, (0.4, 0.5, 0.6))
    s.set_object_indices(0, 1)
    return s


SEAMS = {"through both tiles": ("x", 7.5 / 16), "between the tiles": ("z", 3.5 / 8), "through the first tile": ("z", 1.5 / 8)}


def _pair(oracle, name):
    """the scene as (HostScene, OracleScene)"""
    host, orc = HostScene.builtin(), oracle.OracleScene.builtin()
    if name in SEAMS:
        host, orc = HostScene.empty(), oracle.OracleScene()
        return wall(host, orc.eye_ray, SEAMS[name]), wall(orc, orc.eye_ray, SEAMS[name])
    lights = _lights(orc)
    assert len(lights) >= 1
    build = {"museum": museum, "no specular": museum_no_specular, "tiny factors": museum_tiny_factors,
             "light colours": lambda s: museum_light_colours(s, lights), "infinite light": lambda s: museum_infinite_light(s, lights)}[name]
    return build(host), build(orc)


SCENES = ["museum", "no specular", "tiny factors", "light colours", "infinite light"] + list(SEAMS)


@pytest.fixture(scope="module", params=SCENES)
def scene(request, oracle):
    host, orc = _pair(oracle, request.param)
    r = Renderer(host)
    yield request.param, r, orc
    r.close()


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("W,H,tile_z", SIZES)
def test_gate(scene, W, H, tile_z, depth):
    name, r, orc = scene
    want = orc.render(W, H, depth)
    check(r, want, W, H, tile_z, depth, f"{name} {W}x{H} depth {depth}")


def test_scenes_are_what_they_are_meant_to_be(oracle):
    """The museum has regions of either kind; the seams lie where the docstrings say: the wall with factor 0.5 on both sides
    differs from the mixed one exactly on the far side of the seam, in all of its pixels; the infinite colour reaches pixels as
    NaN (0 x inf) -- the frame the gate must leave alone."""
    orc = oracle.OracleScene.builtin()
    factors = [orc.get_object(i).specular for i in range(orc.object_count)]
    assert any(f == 0.0 for f in factors) and any(f != 0.0 for f in factors)
    for name, (axis, at) in SEAMS.items():
        mixed, live = wall(oracle.OracleScene(), orc.eye_ray, (axis, at)), wall(oracle.OracleScene(), orc.eye_ray, (axis, at))
        for i in range(live.object_count):
            if not live.get_object(i).is_light:
                live.set_specular(i, 0.5)
        differ = (mixed.render(16, 8, 0) != live.render(16, 8, 0)).any(axis=-1)
        x, z = np.meshgrid(np.arange(16) / 16, np.arange(8) / 8, indexing="ij")
        assert (differ == ((x if axis == "x" else z) < at)).all(), name
    _, inf_scene = _pair(oracle, "infinite light")
    assert np.isnan(inf_scene.render(16, 8, 1)).any()
