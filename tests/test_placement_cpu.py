"""placement.py and what can be held to it without a GPU: the wrapper itself, the host model against the oracle on placed scenes,
that no frame the GPU tests compare is inert, and the PRIMARY table (csrc/rt_capi.hip: primary_table()) of placed scenes.

The table's margins are written "relative to distance and magnitude" and carry absolute terms as well (ex = ... + 1.0e-4); whether
those are right shows only when the same scene sits somewhere else, at another size or turned onto other axes.  The reference
is test_primary_table_cpu's: query_ref._collision on rays_ref.camera_rays of the placed camera."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib
import placement
import query_ref
from placement import CLUSTERED_SCENES, FAST_SCENES, NAMES, REPLACED, Placed
from test_host_model import compare
from test_primary_table_cpu import H0, W0, _whole, reference_hits, table, violations
from tilecoderaytracer_amd import HostScene, capi

GENERATORS = FAST_SCENES + CLUSTERED_SCENES
IDS = [f"{g}{s}" for g, s in GENERATORS]
W, H, DEPTH = 64, 48, 4
MIN_COLOURS = 200


def colours(frame):
    return len(np.unique(np.ascontiguousarray(frame).reshape(-1, 3).view(np.uint32), axis=0))


@functools.lru_cache(maxsize=None)
def pair(generator, seed, name):
    """-> (HostScene, OracleScene) of the generator's scene under the catalogue's placement"""
    host, orc, _ = placement.placed_pair(placement.builder(generator, seed), name, generator, seed, HostScene, oracle_lib.OracleScene)
    return host, orc


@functools.lru_cache(maxsize=None)
def oracle_frame(generator, seed, name):
    return pair(generator, seed, name)[1].render(W, H, DEPTH)


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------

def test_the_catalogue_is_what_it_says():
    perms = placement.proper_permutations()
    assert len(perms) == 24 and len({m.tobytes() for m in perms}) == 24
    for m in perms:
        assert np.linalg.det(m) == 1.0 and set(np.abs(m).sum(axis=0)) == {1.0} and set(np.abs(m).sum(axis=1)) == {1.0}
    z = np.array([0.0, 0.0, 1.0])
    assert (placement.PLACEMENTS["x_up"][2] @ z).tolist() == [1.0, 0.0, 0.0]
    assert (placement.PLACEMENTS["y_up_moved"][2] @ z).tolist() == [0.0, 1.0, 0.0]
    for name in ("x_up", "y_up_moved"):
        assert any(np.array_equal(placement.PLACEMENTS[name][2], m) for m in perms), name
    mirror = placement.PLACEMENTS["mirrored"][2]
    assert np.linalg.det(mirror) == -1.0 and (mirror @ np.array([1.0, 2.0, 3.0])).tolist() == [-1.0, 2.0, 3.0]
    r = placement.OBLIQUE
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    assert np.allclose(r @ r.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(r), 1.0)
    assert np.allclose(r @ axis, axis, atol=1e-15) and np.isclose(np.trace(r), 1.0 + 2.0 * np.cos(0.6))
    assert (np.abs(r) > 0.07).all()                      # no axis stays an axis, or in a coordinate plane
    assert [placement.large_scale(g, s) for g, s in (("field", 3), ("random", 5), ("lattice", 12), ("far", 2))] == [100.0, 100.0, 100.0, 1.0]
    assert [placement.large_scale("room", s) for s in (201, 203, 206, 210)] == [1.0e5, 100.0, 1.0, 1000.0]


def test_points_directions_and_lengths():
    """computed in double, rounded to fp32 once; a permutation is exact"""
    p = Placed(None, 3.0, (-90.0, 55.0, 20.0), placement.OBLIQUE)
    x = (1.25, -7.5, 0.3)
    want = 3.0 * (placement.OBLIQUE @ np.array(x, dtype=np.float64)) + np.array([-90.0, 55.0, 20.0])
    assert p.point(x) == tuple(float(np.float32(c)) for c in want)
    assert p.direction(x) == tuple(float(np.float32(c)) for c in placement.OBLIQUE @ np.array(x, dtype=np.float64))
    assert p.length(0.15) == float(np.float32(3.0 * 0.15))
    q = Placed(None, 1.0, (0.0, 0.0, 0.0), placement.PLACEMENTS["x_up"][2])
    assert q.point((1.0, 2.0, 3.0)) == (3.0, 1.0, 2.0) and q.direction((0.0, 0.0, 1.0)) == (1.0, 0.0, 0.0)
    i = Placed(None)
    assert i.identity and i.point(x) is not None and i.point(x) == x and i.length(0.15) == 0.15


def records(scene):
    """every object record of a HostScene's description or of an OracleScene, as bytes"""
    if hasattr(scene, "desc"):
        d = scene.desc.contents
        return [bytes(d.objects[i]) for i in range(d.n_objects)] + [bytes(d.textures[i]) for i in range(d.n_textures)] + \
               [bytes(scene.camera.contents)]
    return [bytes(scene.get_object(i)) for i in range(scene.object_count)] + [bytes(scene.cam)]


@pytest.mark.parametrize("generator,seed", GENERATORS, ids=IDS)
def test_the_identity_placement_changes_nothing(generator, seed):
    build = placement.builder(generator, seed)
    host, orc = pair(generator, seed, "identity")
    plain_host, plain_orc = build(HostScene.empty()), build(oracle_lib.OracleScene())
    assert records(host) == records(plain_host)
    assert records(orc) == records(plain_orc)
    assert oracle_frame(generator, seed, "identity").tobytes() == plain_orc.render(W, H, DEPTH).tobytes()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("generator,seed", GENERATORS, ids=IDS)
def test_placed_scenes_flatten_like_the_oracle(generator, seed, name):
    host, orc = pair(generator, seed, name)
    compare(host, orc, eye_rays=name == "identity")


def test_the_placed_camera_is_the_two_mirrors_camera_placed():
    """eye, look-at point and up through the map; screen and distance times the scale; and it survives later changes"""
    for name in NAMES:
        ph = Placed.named(HostScene.empty(), name, "field", 3)
        placement.builder("field", 3)(ph)
        ph.set_reflective(40, 0.3)                          # (the host model flattens its own camera anew after a change)
        ph.add_sphere((0.0, 3.0, 1.0), 0.5)
        cam = ph.scene.camera.contents
        s, eye, look = ph.scale, np.array(ph.point(Placed.EYE)), np.array(ph.point(Placed.LOOK))
        assert np.array_equal(np.array(list(cam.eye_origin)), np.float32(eye)), name
        assert np.allclose(list(cam.screen_origin), look, rtol=1e-6, atol=1e-6 * s), name
        assert cam.screen_width == cam.screen_height == np.float32(s) and cam.screen_halfwidth == np.float32(s / 2), name
        if name != "mirrored":
            assert np.allclose(list(cam.vector_horizontal), ph.rotation @ [1.0, 0.0, 0.0], atol=1e-6), name
        assert np.allclose(list(cam.vector_vertical), ph.rotation @ [0.0, 0.0, 1.0], atol=1e-6), name


# ---- no inert frames ------------------------------------------------------------------------------------------------------------

def test_no_frame_of_the_gpu_tests_is_inert():
    """every (generator, seed, placement) tests/test_placement_gpu.py renders: at least 200 distinct colours in the oracle's
    64 x 48 depth-4 frame.  (The least is 238, lattice 23 under small_far; among the others 318, room 206 under y_up_moved.)"""
    cases = placement.gpu_cases(GENERATORS) + placement.gpu_cases(placement.ENGAGED_SCENES, placement.ENGAGED_PLACEMENTS)
    counts = {case: colours(oracle_frame(*case)) for case in cases}
    low = min(counts, key=counts.get)
    print(f"least: {low} with {counts[low]} colours")
    assert not {case: n for case, n in counts.items() if n < MIN_COLOURS}
    assert len(counts) == len(GENERATORS) * len(NAMES) + len(placement.ENGAGED_PLACEMENTS)      # (field 4 is in both lists)


def test_the_replaced_cases_are_inert():
    """REPLACED names what it replaces for this reason alone"""
    for (generator, seed, name), other in REPLACED.items():
        assert colours(oracle_frame(generator, seed, name)) < MIN_COLOURS, (generator, seed, name)
        assert other != seed


# ---- the PRIMARY table ----------------------------------------------------------------------------------------------------------

TABLE_SCENES = (("room", 201), ("room", 203), ("room", 206), ("random", 5), ("random", 9), ("far", 2))
LIVE_SCENES = {("room", 203): 1, ("random", 5): 2, ("far", 2): 1}       # whole-image items of the unplaced scene, 90 x 70
# Where a placement changes the number of whole-image items, and why (found by this test's own run, written down here):
#   small_far: a screen 0.05 wide at 3e4 -- a pixel is a fifth of a float's last place there, primary_table()'s error term is
#              wider than the image, and every item gets the whole image;
#   oblique:   the room's walls are no longer axis-aligned, the eye is inside the grown boxes of two of them and the far walls'
#              rectangles cover the image; build_random's and build_far_grazing's axis-aligned infinite planes (slabs) become
#              general planes, which always get the whole image: the mirror wall y = far of far 2, and in random 5 one more
#              rectangle's box reaches round the image.
WHOLE = {
    (("room", 203), "small_far"): 33, (("random", 5), "small_far"): 22, (("far", 2), "small_far"): 11,
    (("room", 203), "oblique"): 7, (("random", 5), "oblique"): 3, (("far", 2), "oblique"): 2,
}
N_ITEMS = {("room", 201): 36, ("room", 203): 34, ("room", 206): 33, ("random", 5): 22, ("random", 9): 22, ("far", 2): 11}
# room 201 (a room of 0.01) degenerates wholly under these as well: every one of its 36 items gets the whole image
WHOLLY_DEGENERATE = {(("room", 201), "tiny"), (("room", 201), "shifted_far"), (("room", 201), "small_far")}


REACH = np.float32(65535.0)       # the reference's rays end there: getCollision takes a hit only at a distance below it


def reachable_hits(orc, cam, w, h, objects):
    """reference_hits() without the hits beyond the rays' reach, which no ray reports (y_up_moved takes room 206, a room of
    1 000, to 10 000: most of its walls are farther away than that)"""
    hits = reference_hits(query_ref.Scene(orc), cam, w, h, objects)
    with np.errstate(invalid="ignore"):
        return {k: (hit & (dist < REACH), dist) for k, (hit, dist) in hits.items()}


def placed_table(scene, name, w, h):
    host, orc = pair(*scene, name)
    return table(host, host.camera.contents, w, h), orc, host.camera.contents


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("scene", TABLE_SCENES, ids=[f"{g}{s}" for g, s in TABLE_SCENES])
def test_placed_tables_are_conservative(scene, name):
    """every pixel the reference hits an item at lies in the item's rectangle, and the entry distance is not beyond the hit"""
    for w, h in ((61, 47), (W0, H0)):
        t, orc, cam = placed_table(scene, name, w, h)
        assert len(t) == N_ITEMS[scene], f"{scene} {name}: {len(t)} items"           # (never empty: the unplaced scene has one)
        assert sorted(t["object"].tolist()) == sorted(set(t["object"].tolist()))
        bad = violations(t, reachable_hits(orc, cam, w, h, t["object"].tolist()), w, h)
        assert not bad, f"{scene} {name}, {w} x {h}: " + "; ".join(bad)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("scene", list(LIVE_SCENES), ids=[f"{g}{s}" for g, s in LIVE_SCENES])
def test_placed_tables_stay_live(scene, name):
    """as many whole-image items as the unplaced scene has, but where WHOLE says otherwise"""
    t, _, _ = placed_table(scene, name, W0, H0)
    whole = int(_whole(t).sum())
    print(f"{scene} {name}: {whole} of {len(t)} items cover the whole image")
    assert whole == WHOLE.get((scene, name), LIVE_SCENES[scene]), (scene, name, whole)
    if name != "small_far":
        assert whole <= len(t) // 4


def test_room_201_degenerates_where_it_is_listed_and_nowhere_else():
    for name in NAMES:
        t, _, _ = placed_table(("room", 201), name, W0, H0)
        whole = int(_whole(t).sum())
        print(f"room 201 {name}: {whole} of {len(t)}")
        assert (whole == len(t)) == ((("room", 201), name) in WHOLLY_DEGENERATE), (name, whole)
