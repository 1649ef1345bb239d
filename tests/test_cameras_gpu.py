"""The kernels under the cameras of cameras.catalogue(): every pixel's bits against the references.

The PRIMARY table (csrc/rt_capi.hip: primary_table(); rt_kernel.hip: fast_primary_key()) decides which items the camera rays'
scan of rt_render_kernel and of every FAST family skips; the horizon line (horizon_dz(), heavy_band(), start_row()) decides which
tiles the clustered-scene kernels render as HEAVY tiles and where their queues start.  tests/test_primary_table_cpu.py holds
the table itself to the reference's hits; here the kernels read such tables: items behind the eye, across the eye plane, left
of column 0, left-handed, oblique, off-centre, wide and narrow screens, eyes inside boxes, cameras no table can be made for --
and horizon lines that leave the image, run upside down, nearly vertical, or so steep that the HEAVY line's Q16 arithmetic
leaves 32 bits on the way."""
import ctypes as C
import functools

import numpy as np
import pytest

import cameras
import oracle_lib
import soft_ref
from rays_ref import camera_rays
from test_kernel_matrix_gpu import World, field, kernel
from test_query_gpu import assert_hits_same
from test_texture_gpu import assert_same_bits
from test_twin_tiles_gpu import assert_same, check
from tilecoderaytracer_amd import HostScene, Renderer, capi

pytestmark = pytest.mark.gpu

FAST_SCENES = ("builtin", "room206")
W, H, DEPTH = 90, 70, 4
# items wholly behind the eye; det of the other sign; the eye's axis outside the image; a screen 40 wide 0.2 before the eye
FOUR = ("among", "left_handed", "off_centre", "wide")


def fast_pair(name, camera):
    """the scene on a HostScene and an OracleScene, both under the catalogue's camera -> (host, orc, cam)"""
    host, orc = cameras.scene_pair(name, HostScene, oracle_lib.OracleScene)
    cam = cameras.put(cameras.catalogue(name)[camera], host, orc)
    return host, orc, cam


@functools.lru_cache(maxsize=None)
def fast_frame(name, camera, w, h):
    return fast_pair(name, camera)[1].render(w, h, DEPTH)


FAST_CASES = [(s, c) for s in FAST_SCENES for c in cameras.catalogue(s)]


@pytest.mark.parametrize("name,camera", FAST_CASES, ids=[f"{s}-{c}" for s, c in FAST_CASES])
def test_fast_scenes_under_every_camera(name, camera):
    """rt_render_kernel with the PRIMARY table and with the bundle cull, whole frames and a strip, against the oracle and
    against rt_render_kernel_items.  The degenerate cameras get no table (the general cull renders them), and the pixel whose
    direction the reference makes NaN is compared like any other."""
    host, _, cam = fast_pair(name, camera)
    want = fast_frame(name, camera, W, H)
    table = capi.primary_rectangles(host.desc, C.byref(cam), W, H)
    assert (len(table) == 0) == (camera in cameras.DEGENERATE), (camera, len(table))
    if camera == "eye_on_screen":
        rays = camera_rays(cam, W, H)
        assert ((rays[..., 3:] == rays[..., :3]).all(axis=-1)).sum() == 1          # one ray of length 0
    r = Renderer(host)
    for primary in (1, 0):
        r.set_option("primary", primary)
        check(r, want, W, H, DEPTH, f"{name} {camera} primary {primary}")
        check(r, want[13:W - 7], W, H, DEPTH, f"{name} {camera} primary {primary}, strip", 13, W - 7)


@pytest.mark.parametrize("camera", FOUR)
@pytest.mark.parametrize("name", FAST_SCENES)
def test_fast_scenes_tile_shapes_and_ragged_frames(name, camera):
    """every tile shape's rectangle test (tile_z 1, 8, 64), a twin without a partner (4 x 33) and a ragged macro row (9 x 130)"""
    host, _, _ = fast_pair(name, camera)
    for tile_z in (1, 8, 64):
        r = Renderer(host)
        r.set_option("tile_z", tile_z)
        check(r, fast_frame(name, camera, W, H), W, H, DEPTH, f"{name} {camera} tile_z {tile_z}")
        assert r.launch_info().tile_z == tile_z
    r = Renderer(host)
    for w, h in ((4, 33), (9, 130)):
        check(r, fast_frame(name, camera, w, h), w, h, DEPTH, f"{name} {camera} {w} x {h}")


# ---- the families that share the table --------------------------------------------------------------------------------------

FW, FH, FDEPTH = 37, 29, 3


@functools.lru_cache(maxsize=None)
def family_world(shading):
    """a World of this module's own (test_kernel_matrix_gpu.world()'s are shared, and this one's camera is replaced)"""
    return World("builtin", shading)


@pytest.mark.parametrize("camera", FOUR + ("oblique",))
@pytest.mark.parametrize("shading", ["", "_image", "_refract_soft"])
def test_families_under_other_cameras(shading, camera):
    """rt_render, rt_render_ssaa (k = 2, 4) and rt_render_gbuffer of the built-in scene -- plain, with image textures, with
    glass and area lights -- against soft_ref and query_ref's records; each launch's kernel by name"""
    w = family_world(shading)
    cam = cameras.put(cameras.catalogue("builtin")[camera], desc=w.desc)
    what = f"builtin{shading} {camera}"
    want = soft_ref.render(w.ref, cam, FW, FH, FDEPTH)
    r = w.renderer({})
    try:
        assert_same_bits(r.render(FW, FH, FDEPTH), want, f"{what}: render")
        assert kernel(r) == "rt_render_kernel" + shading
        for k in (2, 4):
            assert_same_bits(r.render_ssaa(FW, FH, FDEPTH, k), soft_ref.render_ssaa(w.ref, cam, FW, FH, FDEPTH, k), f"{what}: ssaa {k}")
            assert kernel(r) == "rt_render_kernel_ssaa" + shading
        rgb, hits = r.render_gbuffer(FW, FH, FDEPTH)
        assert_same_bits(rgb, want, f"{what}: gbuffer colours")
        assert_hits_same(hits, w.records(camera_rays(cam, FW, FH)), f"{what}: gbuffer records")
        assert kernel(r) == "rt_render_kernel_gbuffer" + shading
    finally:
        r.close()


# ---- clustered scenes: the horizon line -------------------------------------------------------------------------------------

CW, CH, CDEPTH = 144, 128, 3
CSTRIP = (40, 101)


def field_pair(camera):
    host, orc = field(HostScene.empty()), field(oracle_lib.OracleScene())
    cam = cameras.put(cameras.catalogue("field")[camera], host, orc)
    return host, orc, cam


@functools.lru_cache(maxsize=None)
def field_frame(camera, w, h):
    return field_pair(camera)[1].render(w, h, CDEPTH)


def horizon_dz(normal, cam, dx):
    """csrc/rt_capi.hip: horizon_dz(), restated: the height (fraction of the image) at which the column at dx looks along a
    plane of this normal"""
    a = b = 0.0
    for c in range(3):
        at_dx = (cam.screen_origin[c] + cam.vector_horizontal[c] * (dx * cam.screen_width - cam.screen_halfwidth) -
                 cam.vector_vertical[c] * cam.screen_halfheight - cam.eye_origin[c])
        a += at_dx * normal[c]
        b += cam.vector_vertical[c] * cam.screen_height * normal[c]
    return -a / b if b != 0.0 else None


def infinite_planes(orc):
    objs = [orc.get_object(i) for i in range(orc.object_count)]
    return [o.normal.tuple() for o in objs if o.kind == capi.RT_KIND_INFINITE_PLANE]


@pytest.mark.parametrize("camera", ["pitched_up", "pitched_down", "rolled_pi", "rolled_1p45", "two_horizons"])
def test_clustered_field_under_other_horizons(camera):
    """no horizon in the image (the queues start at row 0, no band), the image upside down, a line that crosses most tile rows
    within the frame's width, and two planes' lines in one image: a band of 1 and of 4 rows either side and the automatic
    one, whole frames and a strip narrow enough for the automatic band"""
    host, orc, cam = field_pair(camera)
    lines = [horizon_dz(n, cam, 0.5) for n in infinite_planes(orc)]
    inside = [dz for dz in lines if dz is not None and 0.0 < dz < 1.0]
    if camera.startswith("pitched"):
        assert not inside, lines
    elif camera == "two_horizons":
        assert len(inside) == 2 and abs(inside[0] - inside[1]) * CH > 4.0, lines
    else:
        assert inside, lines
    want = field_frame(camera, CW, CH)
    r = Renderer(host)
    r.set_option("help", 2)
    for heavy in (2, 5, -1):
        r.set_option("heavy", heavy)
        assert_same(r.render(CW, CH, CDEPTH), want, f"{camera}, heavy {heavy}")
        assert kernel(r).startswith("rt_render_kernel_clusters")
        x0, x1 = CSTRIP
        assert_same(r.render(CW, CH, CDEPTH, x0, x1), want[x0:x1], f"{camera}, heavy {heavy}, strip")


@pytest.mark.parametrize("options,name", [({"wide": 1}, "rt_render_kernel_clusters_wide"), ({"tables": 2}, "rt_render_kernel_large")])
def test_clustered_field_other_kernels(options, name):
    host, _, _ = field_pair("rolled_1p45")
    want = field_frame("rolled_1p45", CW, CH)
    r = Renderer(host)
    for key, value in {**options, "help": 2, "heavy": 2}.items():
        r.set_option(key, value)
    assert_same(r.render(CW, CH, CDEPTH), want, f"rolled_1p45 {options}")
    assert kernel(r) == name
    x0, x1 = CSTRIP
    assert_same(r.render(CW, CH, CDEPTH, x0, x1), want[x0:x1], f"rolled_1p45 {options}, strip")


def test_heavy_line_whose_q16_product_leaves_32_bits():
    """(heavy_row0_q16 + tile_col * heavy_slope_q16) >> 16 is evaluated in int at two places of rt_kernel.hip, and a tile is
    rendered exactly once only if both agree.  192 x 128 in tiles of 64 x 1 under the steep-horizon camera: heavy_band()'s row
    values (restated here in double) are below 30 000 at both ends, so the band is made, while slope * (tiles_x - 1) in Q16 is
    beyond 2^31; the line crosses the middle tile column inside the image."""
    w, h, tile_x, tile_z = 192, 128, 64, 1
    host, orc, cam = field_pair("steep_horizon")
    ground = infinite_planes(orc)[0]
    tiles_x = (w + tile_x - 1) // tile_x
    row = [horizon_dz(ground, cam, (c + 0.5) * tile_x / w) * h / tile_z for c in range(tiles_x)]
    row0, slope = row[0], (row[-1] - row[0]) / (tiles_x - 1)
    assert abs(row0) < 30000 and abs(row0 + slope * (tiles_x - 1)) < 30000
    assert abs(slope * (tiles_x - 1)) * 65536 > 2 ** 31
    assert 0 < horizon_dz(ground, cam, 0.5) < 1 and 0 <= row[1] < h
    want = field_frame("steep_horizon", w, h)
    r = Renderer(host)
    r.set_option("help", 2)
    r.set_option("tile_z", tile_z)
    for heavy in (2, 5):
        r.set_option("heavy", heavy)
        assert_same(r.render(w, h, CDEPTH), want, f"steep horizon, heavy {heavy}")
        assert r.launch_info().tile_z == tile_z and kernel(r).startswith("rt_render_kernel_clusters")
        assert_same(r.render(w, h, CDEPTH, 40, 101), want[40:101], f"steep horizon, heavy {heavy}, strip")


def test_learned_order_under_another_camera():
    """rt_learn_tile_order under the two-mirrors camera, then the same W, H and depth under the pitched-down one: the learned
    start row is keyed by the launch's shape, not by the camera, and changes no pixel"""
    host = field(HostScene.empty())
    r = Renderer(host)
    r.learn_tile_order(CW, CH, CDEPTH)
    assert_same(r.render(CW, CH, CDEPTH), field(oracle_lib.OracleScene()).render(CW, CH, CDEPTH), "two-mirrors camera, learned")
    cameras.put(cameras.catalogue("field")["pitched_down"], host)
    assert_same(r.render(CW, CH, CDEPTH), field_frame("pitched_down", CW, CH), "pitched down, learned under another camera")
