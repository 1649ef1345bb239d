"""DEAD REFLECTIONS of the twin tiles (csrc/rt_kernel.hip, render_tile_twin(), RT_TWIN_DEAD_REFLECTIONS): a shaded ray of
rt_render_kernel whose reflection would be folded with a colour of +-0 in all three components -- final = local + (f * C_next) *
oc, oc the three floats fold_child() receives -- ends instead of reflecting, where the host found the scene tame (every colour
component, factor and intensity finite and at most 1 in magnitude: RT_SCENE_VALUES_WILD unset).

Every case asserts that the launch's kernel is rt_render_kernel and compares every pixel with two references, as
test_twin_specular_gpu.py does: the CPU oracle, and the same handle with option "fast" = 0 (rt_render_kernel_items, one tile per
wavefront, no exit).  Bits, except that a NaN equals a NaN.  The frames: exactly one twin, an odd number of tile rows and partial
tiles on both axes -- 16 x 8, 48 x 20 and 33 x 9 under tiles of 16 columns by 4 rows (option "tile_z" 4), and 4 x 32, 12 x 80 and
9 x 33 under the shape the launches choose themselves, 4 columns by 16 rows; one 64 x 64 frame per scene, whose squares'
boundaries cross twins, and one strip of it; depths 0, 1 and 4, and 2 and 3 for the 64 x 64 frame.

The scenes are the museum with HostScene's setters applied.  Counted on the CPU with a copy of the oracle that counts, per
frame, the reflective hits below the last level whose colour is +-0 in every component ("dead"), the ones AT the last level
("last"), and the pixels that change when the dead ones are not traced ("changed"); frames 16x8 / 48x20 / 33x9 / 4x32 / 12x80 /
9x33 / 64x64, depth 4 (last: depth 1):
  tame scenes: the exit fires, and changes no pixel (changed = 0 in every frame of every scene, also at depths 0 to 3)
    museum                 dead  23 / 180 /  57 /  21 / 159 /  54 /  718    last (64 x 64, depth 1 / 2 / 3)  94 /  67 / 25
    dark (-0, 0, -0)       the museum's counts: still a zero colour
    dark (0, 0, 1e-45)     dead 0 in every frame: not a zero colour (and the pixels are the museum's, bit for bit)
    dark (0, 0, 0.5)       dead 0 in every frame: one live component
    black floor            dead  47 / 362 / 115 /  40 / 331 / 110 / 1484    last 192 / 141 / 69
    black sphere           dead  37 / 265 /  85 /  30 / 231 /  76 / 1061    last 122 /  79 / 29   (object 2, reflective factor 1)
    black matte            the museum's counts: black walls and pedestal with reflective factor 0 do not reflect at all
  the last level: "last" counts the black mirrors hit AT the last level -- at depth 1 the floor seen in the ceiling or a sphere,
    at depth 2 floor -> ceiling -> floor, at depth 3 one bounce more -- which the kernel folds with the null colour as before.
  wild scenes: the exit must not fire
    infinite light         dead as the museum; changed   3 /  32 /   7 /   2 /  26 /   8 /  117   (NaN = 0 x inf in the reference)
    nan light              dead as the museum; changed   5 /  35 /  14 /   5 /  29 /   7 /  134
    intensity 2            dead as the museum; changed 0: every value is finite here, the flag is conservative
    specular 1.5           dead as the museum; changed 0: likewise
  one wild scene for each kind of value the host looks at, so that each of its checks is held by pixels (dead as the museum;
  the changed pixels are NaN in the reference, 0 x inf under a black square, and `local` if the ray is ended):
    intensity inf          (light 1)             changed   0 /   9 /   2 /   0 /   6 /   2 /   17
    diffuse inf            (object 4)            changed   0 /   7 /   5 /   0 /   5 /   2 /   23   (depth 1: 0 / 2 / 3 / 0 / 3 / 1 / 10)
    specular inf           (the ceiling slab)    changed   0 /   4 /   0 /   0 /   0 /   0 /    9
    reflective inf         (object 5)            changed   4 /  31 /  10 /   2 /  30 /  10 /  127   (depth 1: ... / 124)
    colour inf             (the ceiling slab)    changed   0 /  30 /   4 /   0 /  24 /   5 /   80
    checker light inf      (the floor's WHITE)   changed   0 /  11 /   2 /   0 /   8 /   4 /   40
    (a wild DARK checkerboard colour cannot be shown by pixels: a square that is not zero is not ended either way)
  the null colour (test_infinite_null_colour): the museum's description with null colour (inf, inf, inf), made through
    Renderer.from_desc().  The oracle's null colour is a constant, so the reference is the fast = 0 render alone.  At depth 1 the
    cut-off colour lands under black squares: dead  20 / 134 /  43 /  19 / 118 /  39 /  532, changed   4 /  31 /  10 /   2 /  30 /
    10 /  124; at depth 4 changed   1 /  12 /   2 /   0 /   5 /   0 /   34 (counted with the copy's null colour set to inf)."""
import ctypes as C

import numpy as np
import pytest

from tilecoderaytracer_amd import HostScene, Renderer, capi

pytestmark = pytest.mark.gpu

TWIN, SINGLE = b"rt_render_kernel", b"rt_render_kernel_items"
SIZES = [(16, 8, 4), (48, 20, 4), (33, 9, 4), (4, 32, 16), (12, 80, 16), (9, 33, 16)]      # W, H, tile_z
DEPTHS = [0, 1, 4]
FLOOR, MIRROR_SPHERE, MATTE = 7, 2, tuple(range(8, 14)) + tuple(range(20, 26))
WHITE, BLACK = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)


def assert_same(got, want, what):
    assert got.shape == want.shape, what
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        bad = np.argwhere(~same.all(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at {bad[0].tolist()}: "
                             f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def check(r, want, W, H, tile_z, depth, what, x0=0, x1=None):
    r.set_option("tile_z", tile_z)
    got = r.render(W, H, depth, x0, x1)
    li = r.launch_info()
    assert li.kernel == TWIN and (li.tile_x, li.tile_z) == (64 // tile_z, tile_z)
    assert_same(got, want, what + ": oracle")
    r.set_option("fast", 0)
    try:
        items = r.render(W, H, depth, x0, x1)
        assert r.launch_info().kernel == SINGLE
    finally:
        r.set_option("fast", 1)
    assert_same(got, items, what + ": item tables")
    return got


def _lights(s):
    return [i for i in range(s.object_count) if s.get_object(i).is_light]


def _dark(colour):
    def build(s, lights):
        s.set_checkerboard(FLOOR, WHITE, colour, 3.0, 3.0)
        return s
    return build


def black_floor(s, lights):
    s.set_checkerboard(FLOOR, BLACK, BLACK, 3.0, 3.0)
    return s


def black_sphere(s, lights):
    s.set_color(MIRROR_SPHERE, BLACK)
    return s


def black_matte(s, lights):
    """the room's walls and the pedestal: reflective factor 0, now black"""
    for i in MATTE:
        s.set_color(i, BLACK)
    return s


def infinite_light(s, lights):
    s.set_color(lights[-1], (1.0, float("inf"), 0.5))
    return s


def nan_light(s, lights):
    s.set_color(lights[0], (1.0, float("nan"), 0.5))
    return s


def intensity_2(s, lights):
    s.set_intensity(lights[-1], 2.0)
    return s


def specular_1_5(s, lights):
    s.set_specular(4, 1.5)
    return s


INF, CEILING = float("inf"), range(26, 32)


def _each(setter, objects, value):
    def build(s, lights):
        for i in objects:
            getattr(s, setter)(i, value)
        return s
    return build


def checker_light_inf(s, lights):
    s.set_checkerboard(FLOOR, (INF, INF, INF), BLACK, 3.0, 3.0)
    return s


WILD = {"infinite light": infinite_light, "nan light": nan_light, "intensity 2": intensity_2, "specular 1.5": specular_1_5,
        "intensity inf": _each("set_intensity", (1,), INF), "diffuse inf": _each("set_diffuse", (4,), INF),
        "specular inf": _each("set_specular", CEILING, INF), "reflective inf": _each("set_reflective", (5,), INF),
        "colour inf": _each("set_color", CEILING, (INF, INF, INF)), "checker light inf": checker_light_inf}
BUILD = {"museum": lambda s, lights: s, "dark -0": _dark((-0.0, 0.0, -0.0)), "dark 1e-45": _dark((0.0, 0.0, 1e-45)),
         "dark 0.5": _dark((0.0, 0.0, 0.5)), "black floor": black_floor, "black sphere": black_sphere, "black matte": black_matte,
         **WILD}
SCENES = list(BUILD)


def pair(oracle, name):
    """the scene as (HostScene, OracleScene)"""
    host, orc = HostScene.builtin(), oracle.OracleScene.builtin()
    lights = _lights(orc)
    assert len(lights) == 2
    return BUILD[name](host, lights), BUILD[name](orc, lights)


@pytest.fixture(scope="module", params=SCENES)
def scene(request, oracle):
    host, orc = pair(oracle, request.param)
    r = Renderer(host)
    cache = {}

    def want(W, H, depth):
        if (W, H, depth) not in cache:
            cache[W, H, depth] = orc.render(W, H, depth)
            cache[W, H, depth].setflags(write=False)
        return cache[W, H, depth]

    yield request.param, r, want
    r.close()


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("W,H,tile_z", SIZES)
def test_exit(scene, W, H, tile_z, depth):
    name, r, want = scene
    check(r, want(W, H, depth), W, H, tile_z, depth, f"{name} {W}x{H} depth {depth}")


@pytest.mark.parametrize("depth", [0, 1, 2, 3, 4])
def test_squares_across_twins(scene, depth):
    """64 x 64 under the automatic shape: 16 x 2 twins; depths 1, 2 and 3 end floor / ceiling chains on the floor"""
    name, r, want = scene
    check(r, want(64, 64, depth), 64, 64, 16, depth, f"{name} 64x64 depth {depth}")


def test_strip(scene):
    name, r, want = scene
    check(r, want(64, 64, 4)[21:46], 64, 64, 16, 4, f"{name} strip 21:46 of 64x64", 21, 46)


def test_scenes_are_what_they_are_meant_to_be(oracle):
    """What the oracle alone can show of the table in the module's docstring: the zero colours render what the museum renders
    and the colours that are not zero do not; the wild lights reach pixels as NaN; the museum's values are all tame and each
    wild scene has one that is not."""
    museum = oracle.OracleScene.builtin().render(64, 64, 4)
    for name, same in (("dark -0", True), ("dark 1e-45", True), ("dark 0.5", False), ("black floor", False),
                       ("black sphere", False), ("black matte", False)):
        got = pair(oracle, name)[1].render(64, 64, 4)
        assert (got.view(np.uint32) == museum.view(np.uint32)).all() == same, name
    for name in WILD:
        if name not in ("intensity 2", "specular 1.5"):
            assert np.isnan(pair(oracle, name)[1].render(48, 20, 4)).any(), name

    def wild(s):
        objs = [s.get_object(i) for i in range(s.object_count)]
        v = [x for o in objs for x in o.color.tuple() + (o.diffuse, o.specular, o.reflective, o.intensity)]
        v += [x for o in objs if o.has_texture for x in o.tex_light.tuple() + o.tex_dark.tuple()]
        return any(not abs(x) <= 1.0 for x in v)

    for name in SCENES:
        assert wild(pair(oracle, name)[1]) == (name in WILD), name


class NullColourScene:
    """the museum's description and camera, copied, with another null colour: rt_scene_desc.null_color is part of the public
    description, and no setter of HostScene reaches it"""

    def __init__(self, null):
        self.host = host = HostScene.builtin()
        d = host.desc.contents
        self.objs = (capi.RtObjectDesc * d.n_objects)(*[d.objects[i] for i in range(d.n_objects)])
        self.texs = (capi.RtTextureDesc * max(d.n_textures, 1))(*[d.textures[i] for i in range(d.n_textures)])
        self.cam = capi.RtCameraDesc()
        C.memmove(C.byref(self.cam), host.camera, C.sizeof(capi.RtCameraDesc))
        self.desc = capi.RtSceneDesc(d.n_objects, self.objs, d.n_textures, self.texs, d.shadow_begin, d.shadow_end,
                                     (C.c_float * 3)(*null))
        self.r = Renderer.from_desc(self.desc, self.cam, keepalive=self)


@pytest.fixture(scope="module")
def null_scenes():
    inf, museum = NullColourScene((INF, INF, INF)), NullColourScene((0.75, 0.75, 0.75))
    yield inf.r, museum.r
    inf.r.close()
    museum.r.close()


@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("W,H,tile_z", SIZES + [(64, 64, 16)])
def test_infinite_null_colour(null_scenes, oracle, W, H, tile_z, depth):
    """The cut-off colour under a black square: inf x 0.5 x 0 is a NaN in the reference, and `local` if the ray is ended.  The
    reference is the item tables' kernel alone (the oracle's null colour is a constant); that the copied description is the
    museum's, and the two kernels' common ground, is checked with the null colour the oracle has."""
    r, museum = null_scenes
    check(museum, oracle.OracleScene.builtin().render(W, H, depth), W, H, tile_z, depth, f"copied museum {W}x{H} depth {depth}")
    r.set_option("fast", 0)
    try:
        want = r.render(W, H, depth)
        assert r.launch_info().kernel == SINGLE
    finally:
        r.set_option("fast", 1)
    if (W, H, depth) != (4, 32, 4) and (W, H, depth) != (9, 33, 4):          # (the two frames with no changed pixel: docstring)
        assert np.isnan(want).any()
    check(r, want, W, H, tile_z, depth, f"infinite null colour {W}x{H} depth {depth}")
