"""The kernels on scenes scaled, shifted and turned onto other axes (placement.py): every pixel's, record's and verdict's bits
against the oracle -- or the *_ref.py built on the oracle's scene -- of the SAME placed scene.

The culls' margins -- the leaf boxes, the plane boxes and slabs, the SHADOW VOXELS, the PRIMARY table, soft_reach() -- are
documented as relative to distance and magnitude and carry absolute terms as well; the generators put every scene into one
box around the origin, z up, the eye at (0, -1, 2.5).  Here each scene sits under every placement of placement.PLACEMENTS:
1e-3 to 1e5 times its size, up to 3e4 units from the origin, on other axes, mirrored, and rotated off every axis.

a. FAST and item-table scenes: the defaults, "fast" 0, "primary" 0, "cull" 0 and a strip; the kernel's name is the unplaced
   scene's, so that a placement routes a scene to no other table mode.
b. Clustered scenes (sphere fields of 120 and 333 spheres, lattices of 12^2 and 23^2 whose coordinates tie on every axis)
   under the options that choose among their structures, a frame and a strip of 1 024 rows with the horizon in its middle.
c. The SHADOW VOXELS are engaged: the counting build's shadow candidates drop when the table is on.
d. Soft shadows, ray queries, G-buffer records and ambient occlusion over the same culls.

When a frame under the defaults differs, the message says whether the plain scans ("cull" 0) of the same placed scene differ
as well: if they do the difference is in shading or intersection, if not it is in a cull.

tests/test_placement_cpu.py holds every frame compared here to at least 200 distinct colours."""
import functools

import numpy as np
import pytest

import ao_ref
import oracle_lib
import placement
import query_ref
import soft_ref
from placement import CLUSTERED_SCENES, FAST_SCENES, NAMES, Placed
from rays_ref import camera_rays
from test_kernel_matrix_gpu import World, kernel
from test_query_gpu import assert_hits_same, assert_verdicts_same
from test_twin_tiles_gpu import assert_same
from tilecoderaytracer_amd import HostScene, Renderer

pytestmark = pytest.mark.gpu
F = np.float32

FW, FH, FDEPTH = 88, 72, 5              # rooms, random and far-grazing scenes
CW, CH, CDEPTH = 96, 80, 4              # fields and lattices
TW, TH, TDEPTH = 16, 1024, 3            # ... and their tall strip: the horizon is in its middle rows


def case_id(case):
    return f"{case[0]}{case[1]}-{case[2]}"


def pair(generator, seed, name):
    """-> (HostScene, OracleScene) of the generator's scene under the catalogue's placement"""
    host, orc, _ = placement.placed_pair(placement.builder(generator, seed), name, generator, seed, HostScene, oracle_lib.OracleScene)
    return host, orc


def renderer(host, options):
    r = Renderer(host)
    for key, value in options.items():
        r.set_option(key, value)
    return r


@functools.lru_cache(maxsize=None)
def unplaced_kernel(generator, seed, options, W, H, depth, x0=0, x1=None):
    """the name of the kernel the unplaced scene launches under the options (a tuple of pairs) for this frame"""
    r = renderer(placement.builder(generator, seed)(HostScene.empty()), dict(options))
    try:
        r.render(W, H, depth, x0, x1)
        return kernel(r)
    finally:
        r.close()


def differs(got, want):
    return got.shape != want.shape or not np.array_equal(got.view(np.uint32), want.view(np.uint32))


def check_defaults(host, r, want, W, H, depth, what):
    """the frame under the handle's options against the oracle's; a difference is attributed with the plain scans' frame"""
    got = r.render(W, H, depth)
    if differs(got, want):
        plain = renderer(host, {"cull": 0})
        try:
            scans = differs(plain.render(W, H, depth), want)
        finally:
            plain.close()
        where = "the plain scans (cull 0) differ from the oracle too: shading or intersection" if scans else \
                "the plain scans (cull 0) equal the oracle: a cull loses or invents a hit"
        try:
            assert_same(got, want, what)
        except AssertionError as e:
            raise AssertionError(f"{e}; {where}") from None


# ---- a. FAST and item-table scenes --------------------------------------------------------------------------------------------

FAST_CASES = placement.gpu_cases(FAST_SCENES)


@pytest.mark.parametrize("case", FAST_CASES, ids=case_id)
def test_fast_scenes_under_every_placement(case):
    generator, seed, name = case
    host, orc = pair(*case)
    want = orc.render(FW, FH, FDEPTH)
    what = case_id(case)
    r = Renderer(host)
    try:
        check_defaults(host, r, want, FW, FH, FDEPTH, f"{what}: defaults")
        assert kernel(r) == unplaced_kernel(generator, seed, (), FW, FH, FDEPTH), what
        assert_same(r.render(FW, FH, FDEPTH, 13, FW - 7), want[13:FW - 7], f"{what}: strip")
        for option in ("fast", "primary", "cull"):
            r.set_option(option, 0)
            assert_same(r.render(FW, FH, FDEPTH), want, f"{what}: {option} 0")
            assert kernel(r) == unplaced_kernel(generator, seed, ((option, 0),), FW, FH, FDEPTH), (what, option)
            assert_same(r.render(FW, FH, FDEPTH, 13, FW - 7), want[13:FW - 7], f"{what}: {option} 0, strip")
            r.set_option(option, 1)
    finally:
        r.close()


# ---- b. clustered scenes ------------------------------------------------------------------------------------------------------

CLUSTERED_CASES = placement.gpu_cases(CLUSTERED_SCENES)
SETTINGS = [(), (("svox", 1500),), (("svox", -1),), (("svox", 0),), (("pairs", 0),), (("cluster_leaf", 4),), (("cluster_leaf", 32),),
            (("tables", 2),), (("heavy", 1),)]
QUARTER = (CW // 2, CW // 2 + CW // 4)


@pytest.mark.parametrize("case", CLUSTERED_CASES, ids=case_id)
def test_clustered_scenes_under_every_placement(case):
    generator, seed, name = case
    host, orc = pair(*case)
    want, tall = orc.render(CW, CH, CDEPTH), orc.render(TW, TH, TDEPTH)
    for options in SETTINGS:
        what = f"{case_id(case)} {dict(options)}"
        r = renderer(host, dict(options))
        try:
            if options:
                assert_same(r.render(CW, CH, CDEPTH), want, what)
            else:
                check_defaults(host, r, want, CW, CH, CDEPTH, what)
            assert kernel(r) == unplaced_kernel(generator, seed, options, CW, CH, CDEPTH), what
            assert_same(r.render(TW, TH, TDEPTH), tall, f"{what}: the strip of {TH} rows")
            assert kernel(r) == unplaced_kernel(generator, seed, options, TW, TH, TDEPTH), what
        finally:
            r.close()
    x0, x1 = QUARTER
    r = renderer(host, {"help": 2})
    try:
        assert_same(r.render(CW, CH, CDEPTH, x0, x1), want[x0:x1], f"{case_id(case)} help 2, columns {x0}:{x1}")
        assert kernel(r) == unplaced_kernel(generator, seed, (("help", 2),), CW, CH, CDEPTH, x0, x1)
    finally:
        r.close()
    cull = renderer(host, {"cull": 0})
    try:
        assert_same(cull.render(CW, CH, CDEPTH), want, f"{case_id(case)} cull 0")
    finally:
        cull.close()


def test_the_clustered_scenes_are_clustered():
    """what the names above are compared with: the unplaced fields and lattices launch the clustered-scene kernels, with their
    tables in global memory the _large one, and "cluster_leaf" 32 leaves the fields of 120 spheres no clustered run"""
    for generator, seed in CLUSTERED_SCENES + (("field", 10),):
        assert unplaced_kernel(generator, seed, (), CW, CH, CDEPTH).startswith("rt_render_kernel_clusters"), (generator, seed)
        assert unplaced_kernel(generator, seed, (("tables", 2),), CW, CH, CDEPTH) == "rt_render_kernel_large", (generator, seed)
        few = generator == "field" and placement.FIELD_SPHERES[seed] < 4 * 32
        assert unplaced_kernel(generator, seed, (("cluster_leaf", 32),), CW, CH, CDEPTH).startswith("rt_render_kernel_clusters") != few
    for generator, seed in FAST_SCENES:
        assert unplaced_kernel(generator, seed, (), FW, FH, FDEPTH) == "rt_render_kernel", (generator, seed)
        assert unplaced_kernel(generator, seed, (("fast", 0),), FW, FH, FDEPTH) == "rt_render_kernel_items", (generator, seed)


# ---- c. the structures are engaged --------------------------------------------------------------------------------------------

# The SHADOW VOXELS are automatic ("svox" -1) from RT_SVOX_MIN_LEAVES = 24 leaves on (csrc/rt_tables.h; a speed decision,
# csrc/rt_capi.hip: pack_shadow_voxels()), and field 4's 333 spheres make 21 leaves of 16: shadow_voxels() refuses it a table
# under "svox" -1 wherever it sits, the unplaced scene included, and makes one when the option names a budget ("svox" 1500: from
# four leaves on).  So field 4 is held to the forced table, field 11 (700 spheres, 35 leaves of 20) to the automatic one, and
# field 4 under "svox" -1 to having none -- under each of the four placements.  No placement makes shadow_voxels() refuse a table
# it makes for the unplaced scene (non-finite values, a grid beyond its budget).
ENGAGED = [(("field", 4), 1500), (("field", 11), -1)]
NO_AUTOMATIC_TABLE = {("field", 4): "21 leaves, fewer than RT_SVOX_MIN_LEAVES = 24"}
COUNTERS = ("nearest_rays", "shadow_rays", "wave_shadow_scans")                     # counters 0, 1 and 3


def counted(scene, name, svox):
    """the counting build's frames and counters with the table asked for by `svox`, and without -> (on, off)"""
    host, orc = pair(*scene, name)
    want = orc.render(CW, CH, CDEPTH)
    r = renderer(host, {"svox": svox})
    try:
        img_on, on = r.render_stats(CW, CH, CDEPTH)
        r.set_option("svox", 0)
        img_off, off = r.render_stats(CW, CH, CDEPTH)
    finally:
        r.close()
    assert_same(img_on, want, f"{scene} {name}: counting build, svox {svox}")
    assert_same(img_off, want, f"{scene} {name}: counting build, svox 0")
    print(f"{scene} {name}: shadow candidates {on['shadow_candidates']} with svox {svox}, {off['shadow_candidates']} with svox 0")
    for counter in COUNTERS:
        assert on[counter] == off[counter] and on[counter] > 0, (counter, on[counter], off[counter])
    return on, off


@pytest.mark.parametrize("name", placement.ENGAGED_PLACEMENTS)
@pytest.mark.parametrize("scene,svox", ENGAGED, ids=[f"{g}{s}-svox{v}" for (g, s), v in ENGAGED])
def test_shadow_voxels_are_engaged_on_placed_fields(scene, svox, name):
    """counting build: the shadow candidates the cull leaves (counter 14) are strictly fewer with the table than without, the
    rays and shadow scans (counters 0, 1, 3) the same, both images the oracle's"""
    on, off = counted(scene, name, svox)
    assert on["shadow_candidates"] < off["shadow_candidates"], (on["shadow_candidates"], off["shadow_candidates"])


@pytest.mark.parametrize("name", placement.ENGAGED_PLACEMENTS)
@pytest.mark.parametrize("scene", list(NO_AUTOMATIC_TABLE), ids=[f"{g}{s}" for g, s in NO_AUTOMATIC_TABLE])
def test_no_automatic_table_below_24_leaves_wherever_the_field_sits(scene, name):
    on, off = counted(scene, name, -1)
    assert on["shadow_candidates"] == off["shadow_candidates"], (NO_AUTOMATIC_TABLE[scene], on["shadow_candidates"], off["shadow_candidates"])


# ---- d. the other families over the same culls ----------------------------------------------------------------------------------

FAMILY_SCENES = {("field", 7): (CW, CH, CDEPTH), ("room", 206): (FW, FH, FDEPTH)}
FAMILY_PLACEMENTS = ("identity", "tiny", "shifted_far", "small_far", "y_up_moved", "oblique")
FAMILY_CASES = [(g, s, n) for g, s in FAMILY_SCENES for n in FAMILY_PLACEMENTS]
AREA_SAMPLES, AREA_RADIUS = 2, 1.5
AO_SAMPLES, AO_RADIUS, AO_SEED = 2, 3.0, 1


@functools.lru_cache(maxsize=None)
def family_world(generator, seed, name, shading):
    scale, shift, rotation = placement.placement(name, generator, seed)
    length = Placed(None, scale, shift, rotation).length

    def build(scene):
        p = Placed(scene, scale, shift, rotation)
        placement.builder(generator, seed)(p)
        return p.put().scene
    return World(f"{generator}{seed}", shading, build, (AREA_SAMPLES, length(AREA_RADIUS))), length


@pytest.mark.parametrize("case", FAMILY_CASES, ids=case_id)
def test_soft_shadows_on_placed_scenes(case):
    """every light an area light of radius length(1.5), 2 x 2 samples: soft_reach()'s 2^-22 max|C_k| with |C| up to 3e4"""
    generator, seed, name = case
    W, H, depth = FAMILY_SCENES[(generator, seed)]
    w, _ = family_world(*case, "_soft")
    assert len(w.area) >= 1
    want = soft_ref.render(w.ref, w.desc.cam, W, H, depth)
    for options in ({}, {"cull": 0}):
        r = w.renderer(options)
        try:
            assert_same(r.render(W, H, depth), want, f"{case_id(case)} soft {options}")
            assert kernel(r).endswith("_soft"), kernel(r)
        finally:
            r.close()


@functools.lru_cache(maxsize=None)
def camera_records(generator, seed, name):
    w, _ = family_world(generator, seed, name, "")
    W, H, _ = FAMILY_SCENES[(generator, seed)]
    return query_ref.intersect(w.query, camera_rays(w.desc.cam, W, H))


@pytest.mark.parametrize("case", FAMILY_CASES, ids=case_id)
def test_ray_queries_on_placed_scenes(case):
    """rt_intersect_rays of the placed camera's rays, rt_occluded_rays of the shadow segments from their hit points"""
    generator, seed, name = case
    W, H, _ = FAMILY_SCENES[(generator, seed)]
    w, _ = family_world(*case, "")
    rays = np.ascontiguousarray(camera_rays(w.desc.cam, W, H))
    hits = camera_records(*case)
    P = hits["point"][hits["object"] >= 0]
    assert len(P) > W * H // 10            # (room 206 under y_up_moved is a room of 10 000: most walls are beyond the rays' reach)
    lights = [np.array(w.orc.get_object(k).origin.tuple(), dtype=F) for k in range(w.orc.object_count) if w.orc.get_object(k).is_light]
    segs = np.ascontiguousarray(np.concatenate([np.concatenate([P, np.broadcast_to(L, P.shape)], axis=1) for L in lights]).astype(F))
    verdicts = query_ref.occluded(w.query, segs)
    for options in ({}, {"cull": 0}):
        r = w.renderer(options)
        try:
            assert_hits_same(r.intersect_rays(rays), hits, f"{case_id(case)} intersect_rays {options}")
            assert_verdicts_same(r.occluded_rays(segs), verdicts, f"{case_id(case)} occluded_rays {options}")
        finally:
            r.close()


@pytest.mark.parametrize("case", FAMILY_CASES, ids=case_id)
def test_gbuffer_and_ambient_occlusion_on_placed_scenes(case):
    """rt_render_gbuffer's colours and records; rt_ambient_occlusion, 2 x 2 samples of radius length(3.0), from those records"""
    generator, seed, name = case
    W, H, depth = FAMILY_SCENES[(generator, seed)]
    w, length = family_world(*case, "")
    want, records = w.orc.render(W, H, depth), camera_records(*case)
    ao = ao_ref.ambient_occlusion(w.query, records, AO_SAMPLES, length(AO_RADIUS), seed=AO_SEED)
    for options in ({}, {"cull": 0}):
        r = w.renderer(options)
        try:
            rgb, hits = r.render_gbuffer(W, H, depth)
            assert_same(rgb, want, f"{case_id(case)} gbuffer colours {options}")
            assert_hits_same(hits, records, f"{case_id(case)} gbuffer records {options}")
            got = r.ambient_occlusion(np.ascontiguousarray(hits), AO_SAMPLES, length(AO_RADIUS), seed=AO_SEED)
            assert got.shape == ao.shape and np.array_equal(got.view(np.uint32), ao.view(np.uint32)), \
                f"{case_id(case)} ambient occlusion {options}: {(got.view(np.uint32) != ao.view(np.uint32)).sum()} records differ"
        finally:
            r.close()
