"""Pin the oracle, query_ref and the host model to a build of the reference itself.

tests/golden/ref/ holds what oracle/_ref/ref_harness -- the reference's own sources, compiled by `make -C oracle ref` -- wrote
for committed scenes: whole frames, getCollision records, calculatePixel colours, inShadeCollisionDetection verdicts, and the
SHA-256 of its frame for every case of a sweep (golden/make_ref_pins.py wrote them; nothing of ours is stored there).

Always, with or without the binary: the oracle reproduces every frame, colour and digest; query_ref every record and verdict,
field by field; the host model rebuilt from each scene file describes the oracle's objects.  Where the binary exists: it
reproduces every fixture and digest byte for byte, twice (so the fixtures are the reference's, and it is deterministic), and
then a live sweep on seeds that are not in digests.json.  A difference is a finding, never a tolerance: bits, NaN-aware."""
import hashlib
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib
import query_ref
import rays_ref
import ref_lib as R
from test_host_model import compare as compare_host_with_oracle

F = np.float32
CASES = R.sweep_cases()
WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))


def assert_frames_same(got, want, what):
    same = R.same_bits(got, want)
    if not same.all():
        bad = np.argwhere(~same.all(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} pixels differ from the reference, first at {bad[0].tolist()}: "
                             f"ours={got[tuple(bad[0])]} reference={want[tuple(bad[0])]}")


def assert_records_same(got, want, what):
    same = R.records_same(got, want)
    if not same.all():
        i = int(np.argmin(same))
        raise AssertionError(f"{what}: {int((~same).sum())} records differ from the reference, first at {i}: "
                             f"ours={got.reshape(-1)[i]} reference={want.reshape(-1)[i]}")


def same_oracle_scenes(a, b):
    """object by object, every derived member, the shadow range and the camera"""
    assert a.object_count == b.object_count and a.shadow_range() == b.shadow_range()
    for i in range(a.object_count):
        assert bytes(a.get_object(i)) == bytes(b.get_object(i)), f"object {i}"
    assert bytes(a.cam) == bytes(b.cam)


# ---- always: the committed fixtures against our restatements ------------------------------------------------------------------

@pytest.mark.parametrize("key", list(R.FRAMES))
def test_oracle_reproduces_the_references_frame(key):
    _, W, H, depth, _ = R.FRAMES[key]
    want = np.fromfile(R.frame_path(key), dtype=F).reshape(W, H, 3)
    got = R.load_scene(R.scene_path(key)).render(W, H, depth)
    assert_frames_same(got, want, key)


@pytest.mark.parametrize("key", list(R.FRAMES))
def test_scene_file_is_its_builders_scene_in_all_three_models(key):
    """the committed scene file is what the builder records today; the host model and the oracle rebuilt from the file, and the
    pair the builder fed directly, describe the same objects, shadow range and camera"""
    rec = R.FRAMES[key][0](host=True)
    assert open(R.scene_path(key)).read() == rec.text(), f"{key}: the builder no longer records the committed scene"
    host, orc = R.load_scene(R.scene_path(key), host=True), R.load_scene(R.scene_path(key))
    compare_host_with_oracle(host, orc)
    compare_host_with_oracle(rec.host, rec.oracle)
    same_oracle_scenes(orc, rec.oracle)


@pytest.mark.parametrize("n,shadows", [(32, True), (16, True), (32, False), (16, False), (3, True), (1, False)])
def test_python_grid_equals_the_native_grids(n, shadows):
    """ref_lib.build_grid (what the reference is handed) against orc_scene_grid and the host model's grid"""
    from tilecoderaytracer_amd import HostScene
    name = f"grid{n}" + ("" if shadows else "-noshadow")
    built = R.build_grid(oracle_lib.OracleScene(), n, shadows)
    same_oracle_scenes(built, oracle_lib.OracleScene.named(name))
    compare_host_with_oracle(HostScene.named(name), built)
    compare_host_with_oracle(R.build_grid(HostScene.empty(), n, shadows), oracle_lib.OracleScene.named(name))


@pytest.mark.parametrize("name", list(R.BATCHES))
def test_records_verdicts_and_colours_of_the_committed_rays(name):
    """query_ref.intersect / occluded against getCollision's record, field by field, and inShadeCollisionDetection's verdict;
    the oracle's calculate_pixel against calculatePixel at depth 3; the oracle's own winner and colour (query_ref's two
    identities) against the reference's record"""
    rays, hits, colours, segs, verdicts = R.load_batch(name)
    path = R.scene_path(R.BATCHES[name])
    orc = R.load_scene(path)
    assert np.array_equal(rays, rays_ref.positive_zeros(rays))
    q = query_ref.Scene(orc)
    assert_records_same(query_ref.intersect(q, rays), hits, f"{name}: query_ref.intersect")
    got = query_ref.occluded(q, segs)
    assert np.array_equal(got, verdicts), f"{name}: {int((got != verdicts).sum())} verdicts differ, first at {int(np.argmax(got != verdicts))}"
    assert_frames_same(rays_ref.oracle_trace(orc, rays, R.BATCH_DEPTH), colours, f"{name}: oracle colours at depth {R.BATCH_DEPTH}")
    winners = query_ref.oracle_objects(lambda: R.load_scene(path), rays)
    assert np.array_equal(winners, hits["object"]), f"{name}: the oracle's winner differs at ray {int(np.argmax(winners != hits['object']))}"
    hit = hits["object"] >= 0
    own = query_ref.oracle_colours(lambda: R.load_scene(path), rays)
    assert_frames_same(own[hit], hits["color"][hit], f"{name}: the oracle's hit colour")
    assert (own[~hit] == F(0.75)).all()
    # the batch holds what it is meant to hold
    assert hit.sum() > 500 and (hits["flags"] & 1).sum() > 20 and (hits["flags"] & 2).sum() > 0
    assert 100 < verdicts.sum() < 900
    assert len(np.unique(hits["object"])) > 4
    if name == "edges":
        # the rectangle's t is the ray's height: the reference lets the float 1E-5 itself through (it is below the double 1E-5
        # the finite plane compares with) and stops the next float up
        winners = hits["object"][-136:].reshape(8, 17)
        assert (winners[:, :9] != 1).all() and (winners[:, 9:] == 1).all()
        assert np.array_equal(verdicts[-136:].reshape(8, 17), winners == 1)


def _entry_frame(entry):
    return np.fromfile(os.path.join(R.GOLDEN_REF, entry["frame"]), dtype=F).reshape(entry["W"], entry["H"], 3)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_oracle_reproduces_the_references_digest(case):
    cid, make, W, H, depth, _ = case
    doc = R.load_digests()
    if cid in doc["excluded"]:
        assert cid not in doc["cases"]
        return                                       # counted and capped by test_the_manifest_is_whole
    entry = doc["cases"][cid]
    got = make().oracle.render(entry["W"], entry["H"], entry["depth"])
    assert (entry["depth"], R.count_nans(got)) == (depth, entry["nans"]), cid
    if entry["sha256"] is None:                      # a frame with NaNs is stored whole
        assert_frames_same(got, _entry_frame(entry), cid)
    else:
        assert (entry["W"], entry["H"]) == (W, H)
        assert hashlib.sha256(got.tobytes()).hexdigest() == entry["sha256"], f"{cid}: the oracle's frame is not the reference's"


def test_the_manifest_is_whole():
    """no case dropped: digests.json holds every case of the sweep, at least the number the sweep was defined with; exclusions
    only among the fuzz seeds, each with its reason, at most 2 % of them; extra.json's digests are the reference's"""
    doc = R.load_digests()
    ids = [c[0] for c in CASES]
    assert len(ids) == len(set(ids)) >= R.SWEEP_MIN_CASES == 268
    assert set(doc["cases"]) | set(doc["excluded"]) == set(ids) and not set(doc["cases"]) & set(doc["excluded"])
    seeds = {c[0] for c in CASES if c[5]}
    assert len(seeds) == 240 and set(doc["excluded"]) <= seeds and len(doc["excluded"]) <= R.MAX_EXCLUDED_SEEDS == 4
    assert all(isinstance(reason, str) and reason for reason in doc["excluded"].values())
    for cid, e in doc["cases"].items():
        assert (e["sha256"] is None) == (e["nans"] > 0) == ("frame" in e), cid
    extra = json.load(open(os.path.join(R.GOLDEN, "extra.json")))
    shared = [k for k in extra if not k.startswith("_")]
    assert len(shared) == 6
    for k in shared:
        assert doc["cases"][k]["sha256"] == extra[k], k
    for key in ("b64d4", "g32_64d4", "g16_64d8"):
        raw = open(R.frame_path(key), "rb").read()
        assert hashlib.sha256(raw).hexdigest() == oracle_lib.SURVEY_PINS[key][4]
    for name in os.listdir(R.GOLDEN_REF):
        assert os.path.getsize(os.path.join(R.GOLDEN_REF, name)) <= R.MAX_FIXTURE_BYTES, name


# ---- where the binary exists: the fixtures are the reference's, and a live sweep ----------------------------------------------

@pytest.fixture(scope="module")
def binary():
    if R.have_binary():
        return R.REF_BINARY
    if R.have_reference():
        pytest.fail(f"the reference is at {R.REFERENCE_DIR} but {R.REF_BINARY} is missing: build() / `make -C oracle ref` must make it")
    pytest.skip(f"neither {R.REF_BINARY} nor the reference's sources ({R.REFERENCE_DIR}/src) exist on this machine: the committed "
                "fixtures were still checked against the oracle above")


def _twice(*args, **kw):
    a, fa = R.run_reference(*args, **kw)
    b, fb = R.run_reference(*args, **kw)
    assert a.tobytes() == b.tobytes() and fa == fb, f"the reference gave two answers: {args} {kw}"
    return a, fa


def test_binary_reproduces_every_frame_and_batch_twice(binary):
    for key, (_, W, H, depth, _) in R.FRAMES.items():
        frame, _ = _twice(R.scene_path(key), W, H, depth)
        assert frame.tobytes() == open(R.frame_path(key), "rb").read(), key
    for name, key in R.BATCHES.items():
        rays, hits, colours, segs, verdicts = R.load_batch(name)
        path = R.scene_path(key)
        assert _twice(path, mode="hits", rays=rays)[0].tobytes() == hits.tobytes(), name
        assert _twice(path, depth=R.BATCH_DEPTH, mode="trace", rays=rays)[0].tobytes() == colours.tobytes(), name
        assert np.array_equal(_twice(path, mode="occluded", rays=segs)[0], verdicts), name


def test_binary_reproduces_every_digest_twice(binary, tmp_path):
    doc = R.load_digests()

    def work(case):
        cid, make, _, _, _, _ = case
        if cid in doc["excluded"]:
            return None
        e = doc["cases"][cid]
        path = make().write(str(tmp_path / (cid + ".scene")))
        frame, failures = _twice(path, e["W"], e["H"], e["depth"])
        if (R.count_nans(frame), failures) != (e["nans"], e["failures"]):
            return f"{cid}: NaNs or FAILURE diagnostics changed"
        if e["sha256"] is None:
            return None if R.same_bits(frame, _entry_frame(e)).all() else f"{cid}: frame differs"
        return None if hashlib.sha256(frame.tobytes()).hexdigest() == e["sha256"] else f"{cid}: digest differs"

    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        wrong = [w for w in pool.map(work, CASES) if w]
    assert not wrong, wrong


@pytest.mark.parametrize("generator", list(R.GENERATORS))
def test_live_sweep_on_fresh_seeds(binary, tmp_path, generator):
    """40 seeds per generator that are not in digests.json: the frame (oracle), the records and verdicts (query_ref) and the ray
    colours (oracle) against the binary.  A seed on which the reference itself fails is counted against the 2 % cap."""
    build = R.GENERATORS[generator]
    assert not set(R.LIVE_SEEDS) & set(R.SWEEP_SEEDS)

    def reference(k_seed):
        k, seed = k_seed
        rec = R._built(build, seed)()
        path = rec.write(str(tmp_path / f"{generator}_{seed}.scene"))
        depth = R.SWEEP_DEPTHS[k % len(R.SWEEP_DEPTHS)]
        rays = R.ray_batch(rec.oracle, seed, n=736)
        try:
            frame, _ = _twice(path, *R.SWEEP_SIZE, depth)
            hits, _ = R.run_reference(path, mode="hits", rays=rays)
            colours, _ = R.run_reference(path, depth=R.BATCH_DEPTH, mode="trace", rays=rays)
            segs = R.segment_batch(rec.oracle, hits, seed, n=512)
            verdicts, _ = R.run_reference(path, mode="occluded", rays=segs)
        except (R.ReferenceFailed, AssertionError) as e:
            return seed, None, str(e)
        return seed, (rec, depth, rays, frame, hits, colours, segs, verdicts), None

    failed = []
    with ThreadPoolExecutor(max_workers=WORKERS) as pool:
        for seed, got, why in pool.map(reference, list(enumerate(R.LIVE_SEEDS))):
            if got is None:
                failed.append((seed, why))
                continue
            rec, depth, rays, frame, hits, colours, segs, verdicts = got
            what = f"{generator} seed {seed}"
            assert_frames_same(rec.oracle.render(*R.SWEEP_SIZE, depth), frame, f"{what}: frame at depth {depth}")
            q = query_ref.Scene(rec.oracle)
            assert_records_same(query_ref.intersect(q, rays), hits, f"{what}: records")
            assert np.array_equal(query_ref.occluded(q, segs), verdicts), f"{what}: verdicts"
            assert_frames_same(rays_ref.oracle_trace(rec.oracle, rays, R.BATCH_DEPTH), colours, f"{what}: ray colours")
    assert len(failed) <= int(0.02 * len(R.LIVE_SEEDS)), failed
