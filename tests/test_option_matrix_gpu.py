"""The speed-only options under the shadings added after them -- image textures, refraction, area lights, both of the last --
and under the ambient-occlusion kernels: include/rt_capi_tuning.h says that every option is covered by a bit-exactness test, and
for these kernels it was so for "fast", "tables", "stack" = 2, "cull" and "svox" alone.

Every case of kernel_matrix.CASES with one of those shadings, at the matrix's own size (37 x 29, depth kernel_matrix.DEPTH) and
against its references (test_kernel_matrix_gpu's World, frame, ssaa_frame, ray_batch, segments, camera_records: one cache in the
process), under each setting of settings_of() on its own, on a fresh handle.  With "tile_z" = 1 the frame has 29 tile rows:
eight macro rows, the top one ragged.  Refraction keeps three stack quads a level, addressed by the thread's number with the
workgroup's size as the stride (refract_entry()): "block_threads" 64, 128 and 512 are other strides than the 256 it had only ever
run with, and the *_refract cases render depth kernel_matrix.DEEP with 64 and 128 threads under "stack" = 0 as well, the mixed
LDS/HBM layout.  The five rt_ao_kernel* modes run test_ao_gpu's records under AO_SETTINGS.

Every launch goes through poisoned.py: into sentinel-filled outputs, so that a cell a setting leaves unwritten shows.  The
launched kernel's name is asserted wherever the setting leaves the table mode alone ("cull" = 0 and "pairs" = 0 give the item
tables: the family is asserted).  "cluster_leaf" = 0 makes a field without clustered runs, which gets FAST tables, and so does
32: pack_runs_and_clusters() clusters a run from four leaves on, and the field's run is 120 spheres.  30, the largest leaf that
still clusters it, runs beside it.  A setting
that the library refuses for a case -- RT_ERR_CAPACITY or RT_ERR_INVALID, and only "stack" = 1 or a workgroup of 512 may be --
is asserted as that refusal and left out for that case."""
import numpy as np
import pytest

import kernel_matrix as km
import poisoned
from test_ao_gpu import H as AO_H, R as AO_R, SEED as AO_SEED, W as AO_W, records as ao_records, reference as ao_reference
from test_kernel_matrix_gpu import H, W, camera_records, frame, ray_batch, segments, ssaa_frame, world
from test_query_gpu import assert_hits_same, assert_verdicts_same
from test_texture_gpu import assert_same_bits
from tilecoderaytracer_amd import RtError, capi

pytestmark = pytest.mark.gpu

NEWER = ("_image", "_refract", "_soft", "_refract_soft")
RENDER_CASES = [c for c in km.CASES if c.shading in NEWER]
CLUSTERED = ("_clusters", "_clusters_wide")
BATCH_ROWS = 29                                   # the batches as a grid of this many rows (the last column is short)
MAY_BE_REFUSED = {("stack", 1), ("block_threads", 512)}

EVERY_MODE = [("tile_z", 1), ("tile_z", 2), ("tile_z", 64), ("block_threads", 64), ("block_threads", 128), ("grid_mult", 0),
              ("grid_mult", 3), ("first_row", 500), ("first_row", 999), ("tile_prio", 1), ("stack", 1), ("stack", 2), ("cull", 0)]
FAST_MODE = [("primary", 0), ("tight_planes", 0), ("aa_planes", 0)]
CLUSTERED_MODES = [("pairs", 0), ("cluster_leaf", 4), ("cluster_leaf", 30), ("cluster_leaf", 32), ("cluster_leaf", 0), ("svox", 0),
                   ("svox", 800), ("block_threads", 512)]
AO_SETTINGS = [("tile_z", 1), ("tile_z", 64), ("block_threads", 64), ("grid_mult", 0), ("first_row", 500), ("cull", 0)]
AO_CLUSTERED = [("pairs", 0), ("cluster_leaf", 4), ("cluster_leaf", 30), ("cluster_leaf", 32), ("svox", 0)]
FIELD_RUN = 120                                   # the field's run of consecutive spheres (scene_gen.build_sphere_field)


def settings_of(mode):
    return [None] + EVERY_MODE + (FAST_MODE if mode == "" else []) + (CLUSTERED_MODES if mode in CLUSTERED else [])


def mode_under(mode, setting):
    """the table mode a setting leaves a case of `mode` in; None: not asserted (the family is)"""
    if setting is None:
        return mode
    key, value = setting
    if key == "cluster_leaf" and (value == 0 or FIELD_RUN < 4 * value):
        return ""                                 # no clustered runs (a run is clustered from four leaves on): FAST tables
    if key in ("cull", "pairs"):
        return None
    return mode


def launch(r, case, depth):
    """the case's call through poisoned.py, compared with its reference"""
    what = km.case_id(case)
    if case.call == "render":
        want = frame(case.scene, case.shading, depth)
        assert_same_bits(poisoned.rt_render_device(r, W, H, depth, 0, W, want), want, what)
    elif case.call == "ssaa":
        want = ssaa_frame(case.scene, case.shading, depth)
        assert_same_bits(poisoned.rt_render_ssaa_device(r, W, H, depth, 2, 0, W, want), want, what)
    elif case.call == "rays":
        rays, want, _ = ray_batch(case.scene, case.shading)
        assert_same_bits(poisoned.rt_trace_rays_device(r, rays, BATCH_ROWS, depth, want), want, what)
    elif case.call == "hits":
        rays, _, want = ray_batch(case.scene, case.shading)
        assert_hits_same(poisoned.rt_intersect_rays_device(r, rays, BATCH_ROWS, want), want, what)
    elif case.call == "occluded":
        segs, want = segments(case.scene, case.shading)
        assert_verdicts_same(poisoned.rt_occluded_rays_device(r, segs, BATCH_ROWS, want), want, what)
    else:
        want, want_hits = frame(case.scene, case.shading, depth), camera_records(case.scene, case.shading)
        rgb, hits = poisoned.rt_render_gbuffer_device(r, W, H, depth, 0, W, (want, want_hits))
        assert_same_bits(rgb, want, f"{what}: colours")
        assert_hits_same(hits, want_hits, f"{what}: records")


def refused(e, setting, what):
    """an RtError of a launch under `setting`: the refusal of a setting that may be refused -> True; anything else is raised"""
    if e.code in (capi.RT_ERR_CAPACITY, capi.RT_ERR_INVALID) and setting in MAY_BE_REFUSED:
        print(f"[option matrix] {what}: refused with {e.code}: {e.message}")
        return True
    raise e


def check_launch(r, setting, what):
    li = r.launch_info()
    assert li.tile_x * li.tile_z == 64 and li.grid_blocks >= 1, (what, li.tile_x, li.tile_z, li.grid_blocks)
    if setting and setting[0] == "block_threads":
        assert li.block_threads == setting[1], (what, li.block_threads)


@pytest.mark.parametrize("case", RENDER_CASES, ids=km.case_id)
def test_options_under_the_newer_shadings(case):
    w = world(case.scene, case.shading)
    ran = 0
    for setting in settings_of(case.mode):
        what = f"{km.case_id(case)} {setting}"
        r = w.renderer({**case.options, **(dict([setting]) if setting else {})})
        try:
            try:
                launch(r, case, km.DEPTH)
            except RtError as e:
                if refused(e, setting, what):
                    continue
            ran += 1
            check_launch(r, setting, what)
            if setting and setting[0] == "tile_z":
                k = 2 if case.call == "ssaa" else 1           # (a supersampled frame's tile holds whole pixels)
                assert r.launch_info().tile_z == min(max(setting[1], k), 64 // k), (what, r.launch_info().tile_z)
            mode, name = mode_under(case.mode, setting), r.kernel_name()
            if mode is None:
                assert name.startswith("rt_render_kernel") and name.endswith(case.family), (what, name)
            else:
                assert name == "rt_render_kernel" + mode + case.family, (what, name)
        finally:
            r.close()
    assert ran >= len(settings_of(case.mode)) - len(MAY_BE_REFUSED)


@pytest.mark.parametrize("block", [64, 128])
@pytest.mark.parametrize("case", [c for c in RENDER_CASES if c.deep], ids=km.case_id)
def test_refraction_mixed_stack_layout_at_other_strides(case, block):
    """depth DEEP under "stack" = 0: the low levels in LDS, the others in HBM, three quads a level at a stride of `block`"""
    w = world(case.scene, case.shading)
    r = w.renderer({**case.options, "stack": 0, "block_threads": block})
    try:
        launch(r, case, km.DEEP)
        li = r.launch_info()
        assert li.block_threads == block and r.kernel_name() == km.kernel_name(case), (li.block_threads, r.kernel_name())
        print(f"[option matrix] {km.case_id(case)} block {block}: lds {li.lds_bytes} bytes, of which tables {li.scene_lds_bytes}")
    finally:
        r.close()


@pytest.mark.parametrize("mode", list(km.MODES))
def test_options_under_the_ao_kernels(mode):
    scene, options = km.MODES[mode]
    n = 4
    hits, want = ao_records(scene), ao_reference(scene, n)
    assert hits.shape == (AO_W, AO_H)
    for setting in [None, "three channels"] + AO_SETTINGS + (AO_CLUSTERED if mode in CLUSTERED else []):
        what = f"rt_ao_kernel{mode} {setting}"
        three = setting == "three channels"
        r = world(scene, "").renderer({**options, **(dict([setting]) if setting and not three else {})})
        try:
            got = poisoned.rt_ambient_occlusion_device(r, hits, AO_H, np.repeat(want[..., None], 3, axis=2) if three else want,
                                                       samples=n, radius=AO_R, seed=AO_SEED, channels=3 if three else 1)
            assert_same_bits(got, np.repeat(want[..., None], 3, axis=2) if three else want, what)
            check_launch(r, None if three else setting, what)
            name, under = r.kernel_name(), mode if three else mode_under(mode, setting)
            if under is not None:
                assert name == "rt_ao_kernel" + under, (what, name)
            else:
                assert name.startswith("rt_ao_kernel"), (what, name)
        finally:
            r.close()
