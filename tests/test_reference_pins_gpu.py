"""The kernels against bytes the reference itself wrote, with no oracle in between.

tests/golden/ref/ (golden/make_ref_pins.py) holds frames, getCollision records, calculatePixel colours and
inShadeCollisionDetection verdicts written by a build of the reference's own sources for committed scene files, and the SHA-256
of its frame for every case of a sweep.  Here every committed scene is rebuilt in the host model from its file and rendered:
rt_render (whole frame and a strip), rt_render_gbuffer (colours; records where the committed rays are a frame's camera rays),
rt_trace_rays, rt_intersect_rays and rt_occluded_rays on the committed rays, and the sweep rendered and hashed.  The five table
modes of kernel_matrix.py run on the two scenes that select them, and every launch's kernel name is asserted, so that each of
the 25 kernels of the plain, _rays, _hits, _occluded and _gbuffer families meets reference-written bytes.  Nothing here reads the
reference's sources or needs its binary.  Ordinary small launches."""
import hashlib
import os

import numpy as np
import pytest

import ref_lib as R
from test_query_gpu import assert_hits_same, assert_verdicts_same
from tilecoderaytracer_amd import Renderer

pytestmark = pytest.mark.gpu
F = np.float32
BASE = "rt_render_kernel"
FAMILIES = ("_rays", "_hits", "_occluded", "_gbuffer")
# table mode -> (the batch whose scene selects it, options), as in kernel_matrix.MODES
MODES = {
    "": ("builtin", {}),
    "_items": ("builtin", {"fast": 0}),
    "_large": ("field7", {"tables": 2}),
    "_clusters": ("field7", {"wide": 0}),
    "_clusters_wide": ("field7", {"wide": 1}),
}


def assert_same(got, want, what):
    same = R.same_bits(got, want)
    if not same.all():
        bad = np.argwhere(~same.all(axis=-1))
        raise AssertionError(f"{what}: {len(bad)} values differ from the reference, first at {bad[0].tolist()}: "
                             f"gpu={got[tuple(bad[0])]} reference={want[tuple(bad[0])]}")


def renderer(key, options=None):
    r = Renderer(R.load_scene(R.scene_path(key), host=True))
    for k, v in (options or {}).items():
        r.set_option(k, v)
    return r


def frame_of(key):
    _, W, H, depth, _ = R.FRAMES[key]
    return np.fromfile(R.frame_path(key), dtype=F).reshape(W, H, 3), W, H, depth


def launched(r, family, mode=None):
    """the last launch's kernel: of `family`, and of table mode `mode` if given -> the whole name"""
    name = r.kernel_name()
    assert name.startswith(BASE), name
    if mode is not None:
        assert name == BASE + mode + family, (name, BASE + mode + family)
    elif family:
        assert name.endswith(family), (name, family)
    else:
        assert not name.endswith(FAMILIES), name
    return name


def check_frame(r, key, mode, what):
    """rt_render, a strip of it, and rt_render_gbuffer's colours against the reference's frame"""
    want, W, H, depth = frame_of(key)
    assert_same(r.render(W, H, depth), want, f"{what}: rt_render")
    names = {launched(r, "", mode)}
    x0, x1 = W // 5, W - W // 3
    assert_same(r.render(W, H, depth, x0, x1), want[x0:x1], f"{what}: rt_render strip {x0}:{x1}")
    names.add(launched(r, "", mode))
    rgb, _ = r.render_gbuffer(W, H, depth)
    assert_same(rgb, want, f"{what}: rt_render_gbuffer colours")
    names.add(launched(r, "_gbuffer", mode))
    return names


def check_batch(r, name, mode, what):
    """the three ray calls on the committed rays, and a G-buffer frame of the rays that are a frame's camera rays"""
    rays, hits, colours, segs, verdicts = R.load_batch(name)
    assert_same(r.trace_rays(rays, R.BATCH_DEPTH), colours, f"{what}: rt_trace_rays")
    names = {launched(r, "_rays", mode)}
    assert_hits_same(r.intersect_rays(rays), hits, f"{what}: rt_intersect_rays")
    names.add(launched(r, "_hits", mode))
    assert_verdicts_same(r.occluded_rays(segs), verdicts, f"{what}: rt_occluded_rays")
    names.add(launched(r, "_occluded", mode))
    W, H = R.GRID
    rgb, records = r.render_gbuffer(W, H, R.BATCH_DEPTH)
    assert_same(rgb, colours[:W * H].reshape(W, H, 3), f"{what}: rt_render_gbuffer colours of the camera grid")
    assert_hits_same(records, hits[:W * H].reshape(W, H), f"{what}: rt_render_gbuffer records")
    names.add(launched(r, "_gbuffer", mode))
    return names


@pytest.mark.parametrize("key", list(R.FRAMES))
def test_every_committed_scene_renders_the_references_frame(key):
    r = renderer(key)
    try:
        check_frame(r, key, None, key)
    finally:
        r.close()


@pytest.mark.parametrize("mode", list(MODES), ids=[m or "fast" for m in MODES])
def test_every_table_mode_against_the_references_bytes(mode):
    """the 25 kernels: five table modes times {plain, _gbuffer, _rays, _hits, _occluded}, each mode's five names asserted whole"""
    name, options = MODES[mode]
    key = R.BATCHES[name]
    r = renderer(key, options)
    try:
        names = check_frame(r, key, mode, f"{name} {options}") | check_batch(r, name, mode, f"{name} {options}")
    finally:
        r.close()
    assert names == {BASE + mode + family for family in ("",) + FAMILIES}, names


@pytest.mark.parametrize("name", list(R.BATCHES))
def test_committed_rays_in_the_default_mode(name):
    r = renderer(R.BATCHES[name])
    try:
        check_batch(r, name, None, name)
    finally:
        r.close()


GROUPS = sorted({c[0].rsplit("_", 1)[0] if c[5] or c[0].startswith(("adversarial", "checkerboard")) else "named"
                 for c in R.sweep_cases()})


@pytest.mark.parametrize("group", GROUPS)
def test_sweep_digests_on_the_gpu(group):
    """every case of digests.json rendered and hashed (a frame with NaNs: compared whole, NaN-aware)"""
    doc = R.load_digests()
    done = 0
    for cid, make, W, H, depth, is_seed in R.sweep_cases():
        mine = cid.rsplit("_", 1)[0] if is_seed or cid.startswith(("adversarial", "checkerboard")) else "named"
        if mine != group or cid in doc["excluded"]:
            continue
        e = doc["cases"][cid]
        r = Renderer(make(host=True).host)
        try:
            got = r.render(e["W"], e["H"], e["depth"])
        finally:
            r.close()
        if e["sha256"] is None:
            want = np.fromfile(os.path.join(R.GOLDEN_REF, e["frame"]), dtype=F).reshape(e["W"], e["H"], 3)
            assert_same(got, want, cid)
        else:
            assert hashlib.sha256(got.tobytes()).hexdigest() == e["sha256"], f"{cid}: the frame is not the reference's"
        done += 1
    assert done >= (56 if group in R.GENERATORS else 6)
