"""TWIN TILES (csrc/rt_tables.h): rt_render_kernel renders wavefront tiles in vertical pairs, two pixels per lane.

Every case asserts that the launch's kernel is rt_render_kernel and compares every pixel's bits with two references: the CPU
oracle, and the same handle with option "fast" = 0 (rt_render_kernel_items, one tile per wavefront).  The cases are the ones a
pair of tiles can get wrong: a partner that does not exist, every tile shape, strips, the queue-entry arithmetic around the
size of the grid, both homes of the two-rows-per-level bounce stack, partners whose rays end at different levels, and every
path of the culls the two tiles now share."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tilecoderaytracer_amd import HostScene, Renderer

pytestmark = pytest.mark.gpu

TWIN, SINGLE = b"rt_render_kernel", b"rt_render_kernel_items"


def assert_same(got, want, what):
    assert got.shape == want.shape, what
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        bad = np.argwhere(~same.all(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at {bad[0].tolist()}: "
                             f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def render_twin(r, W, H, depth, x0=0, x1=None):
    img = r.render(W, H, depth, x0, x1)
    if img.size:
        assert r.launch_info().kernel == TWIN
    return img


def check(r, want, W, H, depth, what, x0=0, x1=None):
    """the handle's frame (rt_render_kernel) against the oracle's and against the item tables' kernel"""
    got = render_twin(r, W, H, depth, x0, x1)
    assert_same(got, want, what + ": oracle")
    r.set_option("fast", 0)
    try:
        items = r.render(W, H, depth, x0, x1)
        if items.size:
            assert r.launch_info().kernel == SINGLE
    finally:
        r.set_option("fast", 1)
    assert_same(got, items, what + ": item tables")
    return got


@pytest.fixture(scope="module")
def builtin(oracle):
    return Renderer(HostScene.builtin()), oracle.OracleScene.builtin()


@pytest.mark.parametrize("W,H", [(1, 1), (4, 16), (4, 17), (4, 32), (4, 33), (4, 48), (5, 80), (9, 130)])
def test_missing_and_present_partners(builtin, W, H):
    """one tile without a partner, exactly one twin, three tile rows, a macro tile plus one row, ragged in both directions"""
    r, orc = builtin
    check(r, orc.render(W, H, 4), W, H, 4, f"{W}x{H}")


@pytest.mark.parametrize("tile_z", [1, 2, 4, 8, 16, 32, 64])
def test_tile_shapes(oracle, tile_z):
    W, H = 2 * (64 // tile_z) + 1, 3 * tile_z + 1
    r = Renderer(HostScene.builtin())
    r.set_option("tile_z", tile_z)
    check(r, oracle.OracleScene.builtin().render(W, H, 4), W, H, 4, f"tile_z {tile_z}")
    assert r.launch_info().tile_z == tile_z and r.launch_info().tile_x * tile_z == 64      # (still one tile's)


def test_strips(builtin):
    r, orc = builtin
    W, H = 64, 96
    want = orc.render(W, H, 4)
    parts = [check(r, want[x0:x1], W, H, 4, f"strip {x0}:{x1}", x0, x1) for x0, x1 in ((0, 3), (3, 4), (4, 37), (37, 64))]
    assert render_twin(r, W, H, 4, 20, 20).shape == (0, H, 3)
    assert_same(np.concatenate(parts), check(r, want, W, H, 4, "frame"), "strips against the frame")


def _tall_oracle(oracle, H):
    """the built-in scene, 4 columns x H rows, depth 4: one oracle scene and one thread per column"""
    with ThreadPoolExecutor(max_workers=4) as pool:
        cols = list(pool.map(lambda x: oracle.OracleScene.builtin().render(4, H, 4, x, x + 1), range(4)))
    return np.concatenate(cols)


def test_entry_arithmetic(oracle):
    """The wavefronts' first entries come by arithmetic and the queue heads count the ones beyond: frames of one twin per row
    pair, 4 columns wide, with one twin fewer than the grid has wavefronts, exactly as many, and one more; the same with a
    grid that covers every entry (grid_mult 0); each twice, and once after a frame of another shape (the re-zeroed heads)."""
    r = Renderer(HostScene.builtin())
    render_twin(r, 4, 32 * 20000, 4)                       # more twins than any grid holds wavefronts
    li = r.launch_info()
    n = li.grid_blocks * li.block_threads // 64
    assert 1 < n < 20000
    for twins in (n - 1, n, n + 1):
        H = 32 * twins
        want = _tall_oracle(oracle, H)
        for grid_mult in (1, 0):
            r.set_option("grid_mult", grid_mult)
            first = check(r, want, 4, H, 4, f"{twins} twins, grid of {n}, grid_mult {grid_mult}")
            li = r.launch_info()
            assert li.grid_blocks * li.block_threads // 64 >= (min(n, twins) if grid_mult else twins)
            assert_same(render_twin(r, 4, H, 4), first, "the same frame again")
            render_twin(r, 9, 130, 4)
            assert_same(render_twin(r, 4, H, 4), first, "after a frame of another shape")
        r.set_option("grid_mult", 1)


def _facing_mirrors(s):
    """the scene of test_parity_gpu.py::test_facing_mirrors_depth_400"""
    i = s.add_sphere((3.0, 5.0, 8.0), 0.15)
    s.set_light(i)
    a = s.add_finite_plane_axes((-4.0, 9.0, -1.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 8.0, 8.0)
    b = s.add_finite_plane_axes((4.0, -3.0, -1.0), (0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), 8.0, 8.0)
    for m in (a, b):
        s.set_reflective(m, 1.0)
        s.set_diffuse(m, 0.0)
    k = s.add_sphere((0.5, 3.0, 2.0), 0.7)
    s.set_color(k, (1, 0, 0))
    s.set_object_indices(0, 1)
    s.camera_two_mirrors()
    return s


@pytest.fixture(scope="module")
def facing_mirrors(oracle):
    orc = _facing_mirrors(oracle.OracleScene())
    return {depth: orc.render(40, 70, depth) for depth in (0, 1, 2, 3, 5, 8, 13)}


@pytest.mark.parametrize("stack", [0, 1, 2])
@pytest.mark.parametrize("depth", [0, 1, 2, 3, 5, 8, 13])
def test_both_stack_homes(facing_mirrors, depth, stack):
    """Two rows per level.  The options size the LDS rows as for every kernel, one per level: "stack" 1 plans max_depth rows
    (at most 13 x 4 KiB here: never refused), which hold the lower half of this kernel's levels, the upper half going to HBM;
    0 plans as many as keep seven workgroups per CU; 2 none.  So the depths cross the border between the two homes at a
    different level under each option, and no launch here may be refused."""
    r = Renderer(_facing_mirrors(HostScene.empty()))
    r.set_option("stack", stack)
    check(r, facing_mirrors[depth], 40, 70, depth, f"depth {depth}, stack {stack}")
    li = r.launch_info()
    rows = (li.lds_bytes - li.scene_lds_bytes) // (16 * li.block_threads)
    if stack == 1:
        assert rows == depth                               # (rows 2 level + ray: levels below depth / 2 are in LDS)
    if stack == 2:
        assert rows == 0


def _divergent(s, flip):
    """Seen by the two-mirrors camera at 8 x 64 (tile rows 0-3 of 16 pixels): a tinted mirror floor patch with a mirror sheet
    a little above it and a mirror sphere, all below the sight lines of tile row 1 -- tile row 0 sees nothing but them, and
    its lowest rows bounce between floor and sheet to any depth, while tile row 1 sees only background.  flip: the same hung
    from above, so that tile row 3 sees it and tile row 2 the background."""
    for centre in ((3.0, 5.0, 8.0), (-4.0, 2.0, -6.0)):
        s.set_light(s.add_sphere(centre, 0.15))
    z = (lambda v: 5.0 - v) if flip else (lambda v: v)
    up, h, x0 = ((0.0, 0.0, -1.0), (-1.0, 0.0, 0.0), 6.0) if flip else ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), -6.0)
    floor = s.add_finite_plane_axes((x0, 3.0, z(0.0)), up, h, 5.7, 12.0)
    sheet = s.add_finite_plane_axes((x0, 4.2, z(0.12)), up, h, 3.3, 12.0)
    ball = s.add_sphere((1.5, 4.0, z(0.35)), 0.3)
    for j in (floor, sheet, ball):
        s.set_reflective(j, 1.0)
        s.set_diffuse(j, 0.25)
        s.set_color(j, (0.9, 0.8, 0.7))
    s.set_object_indices(0, 1)
    s.camera_two_mirrors()
    return s


@pytest.mark.parametrize("flip", [False, True])
def test_divergent_partners(oracle, flip):
    """one ray of a lane ends at level 0 while the other goes on to the last level"""
    orc = _divergent(oracle.OracleScene(), flip)
    want, shallower = orc.render(8, 64, 6), orc.render(8, 64, 5)
    background = (want == np.float32(0.75)).all(axis=-1)
    busy, idle = (slice(48, 64), slice(32, 48)) if flip else (slice(0, 16), slice(16, 32))
    assert background[:, idle].all() and background[:, busy].sum() < 16            # the scene is what it is meant to be
    assert (want[:, busy] != shallower[:, busy]).any(axis=-1).sum() >= 16          # rays that reach the last level
    check(Renderer(_divergent(HostScene.empty(), flip)), want, 8, 64, 6, f"divergent partners, flip {flip}")


def _random_pair(oracle, seed, **kw):
    from scene_gen import build_random
    return build_random(HostScene.empty(), seed, **kw), build_random(oracle.OracleScene(), seed, **kw)


@pytest.mark.parametrize("n_lights", [0, 1, 2, 3])
def test_cull_paths_lights(oracle, n_lights):
    """no light loop, one scan per level, both lights' culls in one pass, a third light's own cull"""
    host, orc = _random_pair(oracle, 17, n_lights=n_lights)
    check(Renderer(host), orc.render(50, 70, 5), 50, 70, 5, f"{n_lights} lights")


@pytest.mark.parametrize("what,kw", [("more than 32 shadow items", dict(n_spheres=30, n_finite=8)),
                                     ("more than 64 items", dict(n_spheres=60, n_finite=12))])
def test_cull_paths_rounds(oracle, what, kw):
    """no two-light pass; several rounds of 64 items and no PRIMARY table"""
    host, orc = _random_pair(oracle, 18, **kw)
    assert orc.object_count > (64 if "64" in what else 32) + 2
    r = Renderer(host)
    r.set_option("cluster_leaf", 0)                        # (sphere runs stay plain items: the FAST tables' kernel)
    check(r, orc.render(50, 70, 5), 50, 70, 5, what)


@pytest.mark.parametrize("key,value", [("primary", 0), ("tile_prio", 1)])
def test_cull_paths_options(builtin, key, value):
    r, orc = builtin
    r.set_option(key, value)
    try:
        check(r, orc.render(50, 70, 4), 50, 70, 4, f"{key} {value}")
    finally:
        r.set_option(key, 1 if key == "primary" else -1)


@pytest.mark.parametrize("seed", range(1, 13))
def test_random_scenes(oracle, seed):
    host, orc = _random_pair(oracle, seed, shadows=(seed % 3 != 0))
    check(Renderer(host), orc.render(50, 70, 5), 50, 70, 5, f"random scene {seed}")


@pytest.mark.parametrize("seed", range(200, 206))
def test_rooms(oracle, seed):
    from scene_gen import build_room
    host, orc = build_room(HostScene.empty(), seed), build_room(oracle.OracleScene(), seed)
    check(Renderer(host), orc.render(50, 70, 5), 50, 70, 5, f"room {seed}")


def _degenerate(s):
    """the scene of test_parity_gpu.py::test_degenerate_geometry: rays with non-finite components"""
    i = s.add_sphere((3.0, 5.0, 8.0), 0.15)
    s.set_light(i)
    s.add_sphere((0.0, 6.0, 1.0), 0.0)
    s.add_sphere((1.0, 6.0, 1.0), -1.0)
    s.add_infinite_plane((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    s.add_finite_plane_axes((0.0, 8.0, 0.0), (0.0, -1.0, 0.0), (1.0, 0.0, 0.0), 0.0, 3.0)
    i = s.add_infinite_plane((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0))
    s.set_reflective(i, 0.5)
    i = s.add_sphere((0.0, -1.0, 2.5), 3.0)
    s.set_reflective(i, 1.0)
    s.set_object_indices(0, 1)
    s.camera_two_mirrors()
    return s


def test_non_finite_rays(oracle):
    check(Renderer(_degenerate(HostScene.empty())), _degenerate(oracle.OracleScene()).render(48, 40, 4), 48, 40, 4, "degenerate geometry")
