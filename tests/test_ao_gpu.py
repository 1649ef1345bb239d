"""Ambient occlusion (include/rt_capi_ao.h) on the GPU against its definition: ao_ref's numpy restatement (pinned to query_ref's
verdicts in test_ao_cpu.py) and, as a second reference that shares no new code, the GPU's own occlusion query over
ao_ref.segments().  Bar: BIT-EXACT over every record."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import ao_ref
import image_ref
import kernel_matrix as km
import query_ref
from rays_ref import camera_rays
from test_kernel_matrix_gpu import world
from tilecoderaytracer_amd import RtError, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H = 97, 61
R = 2.0
SEED = 1


def assert_same(got, want, what):
    assert got.dtype == F and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    g, w = got.reshape(-1).view(np.uint32), np.ascontiguousarray(want).reshape(-1).view(np.uint32)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        i = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(g)} values differ, first at {i}: gpu={got.reshape(-1)[i]!r} "
                             f"ref={np.ascontiguousarray(want).reshape(-1)[i]!r}")


@functools.lru_cache(maxsize=None)
def renderer(mode):
    scene, options = km.MODES[mode]
    return world(scene, "").renderer(dict(options))


@functools.lru_cache(maxsize=None)
def records(scene, w=W, h=H):
    """query_ref's records of the w x h frame's camera rays"""
    wd = world(scene, "")
    return query_ref.intersect(wd.query, camera_rays(wd.desc.cam, w, h))


@functools.lru_cache(maxsize=None)
def reference(scene, n, seed=SEED, w=W, h=H):
    return ao_ref.ambient_occlusion(world(scene, "").query, records(scene, w, h), n, R, seed=seed)


# ---- 1. all five modes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 3, 4, 8])
@pytest.mark.parametrize("mode", list(km.MODES))
def test_every_mode_equals_the_reference(mode, n):
    scene = km.MODES[mode][0]
    r, hits, want = renderer(mode), records(scene), reference(scene, n)
    got = r.ambient_occlusion(hits, n, R, seed=SEED)
    assert r.kernel_name() == "rt_ao_kernel" + mode == r.launch_info().kernel.decode()
    assert_same(got, want, f"{mode} n={n}")
    three = r.ambient_occlusion(hits, n, R, seed=SEED, channels=3)
    assert r.kernel_name() == "rt_ao_kernel" + mode
    assert three.shape == (W, H, 3)
    assert_same(three, np.repeat(want[..., None], 3, axis=2), f"{mode} n={n}, three channels")
    assert n == 1 or ((want > 0) & (want < 1)).mean() > 0.1        # (an estimate, not a flat field)


# ---- 2. against the occlusion query -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(km.MODES))
def test_every_mode_equals_the_occlusion_query_of_its_segments(mode):
    r, hits = renderer(mode), records(km.MODES[mode][0])
    for n in (1, 3, 4, 8):
        segs, live = ao_ref.segments(hits, n, R, seed=SEED)
        blocked = r.occluded_rays(np.ascontiguousarray(segs.reshape(-1, 6)), rows=H).reshape(segs.shape[:2])
        assert r.kernel_name().endswith("_occluded")
        got = r.ambient_occlusion(hits, n, R, seed=SEED)
        assert_same(got, ao_ref.from_verdicts(blocked, live, n).reshape(W, H), f"{mode} n={n} against rt_occluded_rays")


# ---- 3. small sizes, 4. rows -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (67, 3)])
@pytest.mark.parametrize("mode", ["", "_clusters"])
def test_small_sizes(mode, w, h):
    scene = km.MODES[mode][0]
    r, hits = renderer(mode), records(scene, w, h)
    for n in (1, 4):
        assert_same(r.ambient_occlusion(hits, n, R, seed=SEED), reference(scene, n, SEED, w, h), f"{mode} {w}x{h} n={n}")
    li = r.launch_info()
    assert li.tile_x * li.tile_z == 64


@pytest.mark.parametrize("mode", ["", "_items", "_clusters_wide"])
def test_rows_never_change_a_result(mode):
    scene = km.MODES[mode][0]
    r, hits, want = renderer(mode), records(scene).reshape(-1), reference(scene, 4).reshape(-1)
    for rows in (1, 7, 64, H + 1, len(hits), len(hits) + 5, 2 ** 31 - 1):
        assert_same(r.ambient_occlusion(hits, 4, R, seed=SEED, rows=rows), want, f"{mode} rows={rows}")
        assert_same(r.ambient_occlusion(hits, 4, R, seed=SEED, rows=rows, channels=3), np.repeat(want[:, None], 3, axis=1),
                    f"{mode} rows={rows}, three channels")


# ---- 5. strips, 6. seeds -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["", "_large"])
def test_strips_with_their_key0_equal_the_frames_columns(mode):
    scene = km.MODES[mode][0]
    r, hits, want = renderer(mode), records(scene), reference(scene, 4)
    for x0, x1 in ((0, 1), (1, 30), (30, 96), (96, 97)):
        strip = np.ascontiguousarray(hits[x0:x1])
        assert_same(r.ambient_occlusion(strip, 4, R, seed=SEED, key0=x0 * H), want[x0:x1], f"{mode} columns {x0}:{x1}")
    if mode == "":
        assert not np.array_equal(r.ambient_occlusion(np.ascontiguousarray(hits[30:96]), 4, R, seed=SEED), want[30:96])
        # the key wraps: key0 = 2^32 - 5 is the reference's, and key0 + 2^32 is key0
        top = r.ambient_occlusion(hits, 4, R, seed=SEED, key0=2 ** 32 - 5)
        assert_same(top, ao_ref.ambient_occlusion(world(scene, "").query, hits, 4, R, seed=SEED, key0=2 ** 32 - 5), "wrapping key")
        assert not np.array_equal(top, want)


@pytest.mark.parametrize("mode", ["", "_clusters"])
def test_two_seeds(mode):
    scene = km.MODES[mode][0]
    r, hits = renderer(mode), records(scene)
    a, b = reference(scene, 3, 1), reference(scene, 3, 0xDEADBEEF)
    assert not np.array_equal(a, b)
    assert_same(r.ambient_occlusion(hits, 3, R, seed=1), a, f"{mode} seed 1")
    assert_same(r.ambient_occlusion(hits, 3, R, seed=0xDEADBEEF), b, f"{mode} seed 0xdeadbeef")


# ---- 7. shading --------------------------------------------------------------------------------------------------------------------

def test_glass_and_area_lights_give_the_plain_geometrys_bits():
    """the field packed with glass (a pane added) and area lights, in _clusters: the same kernel and the same bits as the same
    objects created plain, both ao_ref's"""
    w = world("field", "_refract_soft")
    hits = query_ref.intersect(w.query, camera_rays(w.desc.cam, W, H))
    want = ao_ref.ambient_occlusion(w.query, hits, 4, R, seed=SEED)
    shaded, plain = w.renderer({"wide": 0}), w.desc.make(images=None, options={"wide": 0})
    shaded.set_shadow_seed(99)                                   # (the scene's own seed plays no part)
    for r, what in ((shaded, "glass and area lights"), (plain, "plain")):
        assert_same(r.ambient_occlusion(hits, 4, R, seed=SEED), want, what)
        assert r.kernel_name() == "rt_ao_kernel_clusters"
    assert ((want > 0) & (want < 1)).mean() > 0.1


# ---- 8. synthetic records ----------------------------------------------------------------------------------------------------------

def synthetic_records(scene):
    """real records of the frame with their fields replaced: misses and lights with unusable points, inside hits with the normal
    pointing out of a sphere of the scene, NaN and infinite points and normals, signed zeros, N.x at and around +-0.5"""
    wd = world(scene, "")
    base = records(scene).reshape(-1)
    base = base[ao_ref.live_records(base)][:1024].copy()
    rng = np.random.RandomState(11)
    out = []

    def take(k):
        return base[rng.randint(len(base), size=k)].copy()

    nan, inf = F(np.nan), F(np.inf)
    miss = take(40); miss["object"] = -1; miss["point"][::2] = nan; out.append(miss)
    miss2 = take(8); miss2["object"] = -(2 ** 31); out.append(miss2)
    light = take(40); light["flags"] |= 2; light["normal"][::2] = inf; out.append(light)
    both = take(8); both["flags"] = 3; out.append(both)
    spheres = [o for o in wd.query.objects if o.kind == 0 and not o.is_light][:12]
    for o in spheres:                                             # inside hits: a point inside the sphere, the normal outwards
        rec = take(16)
        d = rng.normal(size=(16, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
        c = np.array([o.origin.x, o.origin.y, o.origin.z])
        rec["point"] = (c + d * np.sqrt(o.radius_squared) * rng.uniform(0.2, 1.0, size=(16, 1))).astype(F)
        rec["normal"] = d.astype(F)
        rec["flags"] = 1
        out.append(rec)
        rec = rec.copy(); rec["flags"] = 0; out.append(rec)           # and the same records looking outwards
    for field in ("point", "normal"):
        for value in (nan, inf, -inf):
            for axis in range(3):
                rec = take(6); rec[field][:, axis] = value; out.append(rec)
        rec = take(6); rec[field] = nan; out.append(rec)
        rec = take(6); rec[field] = inf; out.append(rec)
    zero = take(12); zero["normal"] = F(0); zero["normal"][::2] = F(-0.0); out.append(zero)
    for axis in range(3):
        for z in (F(0.0), F(-0.0)):
            rec = take(8)
            n = rec["normal"].astype(np.float64) + 0.25; n[:, axis] = 0
            n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F); n[:, axis] = z
            rec["normal"] = n; out.append(rec)
            rec = take(8); rec["point"][:, axis] = z; out.append(rec)
    for half in (F(0.5), F(-0.5)):
        for x in (half, np.nextafter(half, F(0)), np.nextafter(half, F(2) * half)):
            rec = take(8)
            yz = rng.normal(size=(8, 2)); yz /= np.linalg.norm(yz, axis=1)[:, None]
            rec["normal"][:, 0] = x
            rec["normal"][:, 1:] = (yz * np.sqrt(1.0 - float(x) ** 2)).astype(F)
            out.append(rec)
            rec = rec.copy(); rec["flags"] = 1; out.append(rec)
    recs = np.concatenate(out)
    return recs[rng.permutation(len(recs))]


@pytest.mark.parametrize("mode", list(km.MODES))
def test_synthetic_records(mode):
    scene = km.MODES[mode][0]
    r, hits = renderer(mode), synthetic_records(scene)
    assert len(hits) > 64 * 8
    for n in (1, 4):
        want = ao_ref.ambient_occlusion(world(scene, "").query, hits, n, R, seed=SEED)
        got = r.ambient_occlusion(hits, n, R, seed=SEED)
        assert_same(got, want, f"{mode} synthetic n={n}")
        segs, live = ao_ref.segments(hits, n, R, seed=SEED)
        blocked = r.occluded_rays(np.ascontiguousarray(segs.reshape(-1, 6))).reshape(segs.shape[:2])
        assert_same(got, ao_ref.from_verdicts(blocked, live, n), f"{mode} synthetic n={n} against rt_occluded_rays")
        assert (got[~live] == 1.0).all() and (~live).sum() >= 96
    inside = (hits["flags"] == 1) & live
    assert (want[inside] < 1).any() and (want[(hits["flags"] == 0) & live] == 1).any()
    # a batch without one live record scans nothing and is all ones
    dead = hits[~live]
    assert (r.ambient_occlusion(dead, 4, R, channels=3) == 1.0).all()


# ---- 9. the device entry point ------------------------------------------------------------------------------------------------------

def test_device_path_behind_the_gbuffer_on_one_stream():
    import torch
    r = renderer("")
    w, h, n = 203, 131, 3
    fill = 7.25
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_rgb = torch.zeros((w, h, 3), dtype=torch.float32, device="cuda")
        d_hits = torch.zeros((w * h * 12,), dtype=torch.int32, device="cuda")
        d_ao = torch.full((w * h + 128,), fill, dtype=torch.float32, device="cuda")
        d_ao3 = torch.full((w * h * 3 + 128,), fill, dtype=torch.float32, device="cuda")
        assert stream.cuda_stream != 0 and d_hits.data_ptr() % 16 == 0
        r.render_gbuffer_device(w, h, 0, 0, w, d_rgb.data_ptr(), d_hits.data_ptr(), stream.cuda_stream)
        r.ambient_occlusion_device(w * h, h, d_hits.data_ptr(), d_ao.data_ptr() + 256, samples=n, radius=R, seed=SEED,
                                   stream=stream.cuda_stream)                      # (no host wait in between)
        assert r.kernel_name() == "rt_ao_kernel"
        r.ambient_occlusion_device(w * h, h, d_hits.data_ptr(), d_ao3.data_ptr() + 256, samples=n, radius=R, seed=SEED,
                                   channels=3, stream=stream.cuda_stream)
    stream.synchronize()
    hits = d_hits.cpu().numpy().view(HIT_DTYPE).reshape(w, h)
    want = ao_ref.ambient_occlusion(world("builtin", "").query, hits, n, R, seed=SEED)
    ao, ao3 = d_ao.cpu().numpy(), d_ao3.cpu().numpy()
    assert_same(ao[64:-64].reshape(w, h), want, "device path")
    assert_same(ao3[64:-64].reshape(w, h, 3), np.repeat(want[..., None], 3, axis=2), "device path, three channels")
    for a in (ao, ao3):
        assert (a[:64] == fill).all() and (a[-64:] == fill).all()                  # nothing before or behind the output
    assert np.array_equal(hits.view(np.uint32), records("builtin", w, h).view(np.uint32))   # the input is only read
    assert r.timing().last_kernel_ms > 0.0


# ---- 10. the argument checks, in the header's order ---------------------------------------------------------------------------------

def test_argument_checks_in_the_headers_order():
    lib = capi.load_library()
    r = renderer("")
    s = r._scene
    hits = np.ascontiguousarray(records("builtin").reshape(-1)[:8])
    out = np.full(8 * 3, 7.0, dtype=F)
    P = capi.RtAoParams
    h, o = hits.ctypes.data, out.ctypes.data
    launches = r.timing().launches

    def host(params, n, rows, hp, op):
        return lib.rt_ambient_occlusion(s, C.byref(params) if params is not None else None, n, rows, hp, op)

    def device(params, n, rows, hp, op):
        return lib.rt_ambient_occlusion_device(s, C.byref(params) if params is not None else None, n, rows, hp, op, None)

    nan, inf = float("nan"), float("inf")
    # each line breaks its own check and every later one it can; the text names the first
    cases = [(None, -1, 0, None, None, "params")]
    cases += [(P(k, nan, 0, 0, 2), -1, 0, None, None, "samples") for k in (0, 9, -4, 2 ** 31 - 1)]
    cases += [(P(k, x, 0, 0, 2), -1, 0, None, None, "radius") for k in (1, 8) for x in (0.0, -0.0, -1.0, nan, inf, -inf)]
    cases += [(P(4, R, 0, 0, c), -1, 0, None, None, "channels") for c in (0, 2, 4, -1)]
    cases += [(P(4, R, 0, 0, 1), -1, 0, None, None, "n < 0"),
              (P(4, R, 0, 0, 3), 8, 0, None, None, "rows"),
              (P(4, R, 0, 0, 3), 0, 0, None, None, "rows"),
              (P(4, R, 0, 0, 1), 8, 8, None, None, "hits"),
              (P(4, R, 0, 0, 1), 533333334, 8, None, None, "hits"),
              (P(4, R, 0, 0, 1), 8, 8, h, None, "output"),
              (P(4, R, 0, 0, 1), 533333334, 8, h, o, "533333333"),
              (P(4, R, 0, 0, 1), 2 ** 31 - 1, 2 ** 31 - 1, h, o, "533333333")]
    for params, n, rows, hp, op, text in cases:
        for call in (host, device):
            assert call(params, n, rows, hp, op) == capi.RT_ERR_INVALID, (text, call.__name__)
            assert text in lib.rt_last_error().decode(), (text, call.__name__, lib.rt_last_error())
    # the device call's alignments, the records' first, both behind the record limit
    good = P(4, R, 0, 0, 1)
    assert device(good, 533333334, 8, 24, 2) == capi.RT_ERR_INVALID and "533333333" in lib.rt_last_error().decode()
    for hp in (8, 4, 17):
        assert device(good, 8, 8, hp, 2) == capi.RT_ERR_INVALID and "d_hits" in lib.rt_last_error().decode()
    for op in (2, 1, 35):
        assert device(good, 8, 8, 32, op) == capi.RT_ERR_INVALID and "d_out_ao" in lib.rt_last_error().decode()
    assert (out == 7.0).all() and r.timing().launches == launches          # nothing ran
    # n = 0 is RT_OK and launches nothing, with or without buffers
    for call in (host, device):
        assert call(good, 0, 1, None, None) == capi.RT_OK
        assert call(P(8, 1e-30, 5, 7, 3), 0, 5, h, o) == capi.RT_OK
    assert (out == 7.0).all() and r.timing().launches == launches
    # and the limits' good sides: 1 and 8 samples, a tiny and a huge radius
    for params in (P(1, 1e-30, 0, 0, 1), P(8, 3e38, 0, 0, 3)):
        assert host(params, 8, 8, h, o) == capi.RT_OK
    assert r.timing().launches == launches + 2


# ---- 11. the wrappers and the executable --------------------------------------------------------------------------------------------

def test_python_wrappers():
    r = renderer("")
    hits, want = records("builtin"), reference("builtin", 4)
    _, gpu_hits = r.render_gbuffer(W, H, 0)
    assert np.array_equal(gpu_hits.view(np.uint32), hits.view(np.uint32))
    assert_same(r.render_ao(W, H, 4, R, seed=SEED), want, "render_ao")
    assert_same(r.render_ao(W, H, 4, R, seed=SEED, channels=3), np.repeat(want[..., None], 3, axis=2), "render_ao, three channels")
    # the defaults: 4 x 4 directions, radius 1.0, seed 0, key0 0, one channel
    assert_same(r.ambient_occlusion(hits), ao_ref.ambient_occlusion(world("builtin", "").query, hits, 4, 1.0), "defaults")
    assert r.ambient_occlusion(hits[:0].copy()).shape == (0, H)
    with pytest.raises(TypeError):
        r.ambient_occlusion(np.zeros((4, 12), dtype=F))
    with pytest.raises(RtError) as e:
        r.ambient_occlusion(hits, samples=9)
    assert e.value.code == capi.RT_ERR_INVALID and "samples" in e.value.message
    with pytest.raises(RtError):
        r.render_ao(W, H, 4, R, channels=2)


def test_raytracer_ao_ppm_is_the_reference_encode_of_the_reference_ao(tmp_path):
    exe = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
    w, h = 64, 48
    common = [exe, "--width", str(w), "--height", str(h), "--depth", "3", "--no-txt"]
    p = subprocess.run(common + ["--ao", "3:2.0", "--ao-ppm", "a.ppm", "--ppm", "f.ppm"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0 and "Ambient occlusion (ms)" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    wd = world("builtin", "")
    hits = records("builtin", w, h)
    ao = ao_ref.ambient_occlusion(wd.query, hits, 3, 2.0, channels=3)
    want = image_ref.encode(ao, image_ref.table("linear"))
    assert len(np.unique(want)) >= 8
    assert (tmp_path / "a.ppm").read_bytes() == b"P6\n64 48\n255\n" + want.tobytes()
    # the frame is the one rendered without the option
    q = subprocess.run(common + ["--ppm", "g.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert q.returncode == 0 and (tmp_path / "f.ppm").read_bytes() == (tmp_path / "g.ppm").read_bytes()
    # the default radius is 1.0; the two options come together
    p = subprocess.run(common + ["--ao", "2", "--ao-ppm", "b.ppm"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-500:])
    want = image_ref.encode(ao_ref.ambient_occlusion(wd.query, hits, 2, 1.0, channels=3), image_ref.table("linear"))
    assert (tmp_path / "b.ppm").read_bytes() == b"P6\n64 48\n255\n" + want.tobytes()
    for bad in (["--ao", "3"], ["--ao-ppm", "c.ppm"], ["--ao", "9", "--ao-ppm", "c.ppm"], ["--ao", "3:0", "--ao-ppm", "c.ppm"],
                ["--ao", "3:", "--ao-ppm", "c.ppm"], ["--ao", "3x", "--ao-ppm", "c.ppm"], ["--ao", "4abc", "--ao-ppm", "c.ppm"],
                ["--ao", "3:2x", "--ao-ppm", "c.ppm"], ["--ao", ":2", "--ao-ppm", "c.ppm"], ["--ao", "3", "--ao-ppm", "c.ppm", "--ssaa", "2"]):
        p = subprocess.run(common + bad, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert p.returncode == 1 and "usage" in p.stderr, (bad, p.returncode)
        assert not (tmp_path / "c.ppm").exists()
