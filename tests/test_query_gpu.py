"""Ray queries (include/rt_capi_query.h) against their definition: the records of getCollision and the verdicts of
inShadeCollisionDetection, restated in numpy by query_ref (pinned to the oracle in test_query_cpu.py).  Bar: BIT-EXACT; a NaN
equals a NaN only where the reference gives one."""
import threading

import numpy as np
import pytest

import query_ref
from rays_ref import camera_rays
from test_rays_gpu import incoherent_rays
from tilecoderaytracer_amd import HostScene, Renderer, RtError, capi
from tilecoderaytracer_amd.renderer import HIT_DTYPE

pytestmark = pytest.mark.gpu


def assert_hits_same(got, want, what):
    assert got.dtype == HIT_DTYPE and got.shape == want.shape, (what, got.shape, want.shape)
    g = np.ascontiguousarray(got).reshape(-1).view(np.uint32).reshape(-1, 12)
    w = np.ascontiguousarray(want).reshape(-1).view(np.uint32).reshape(-1, 12)
    gf, wf = g.view(np.float32), w.view(np.float32)
    nan = np.isnan(gf) & np.isnan(wf)
    nan[:, 0] = nan[:, 11] = False                                  # object and flags are integers
    same = ((g == w) | nan).all(axis=1)
    if not same.all():
        i = int(np.argmin(same))
        raise AssertionError(f"{what}: {int((~same).sum())} records differ, first at {i}: gpu={got.reshape(-1)[i]} "
                             f"ref={want.reshape(-1)[i]}")


def assert_verdicts_same(got, want, what):
    assert got.dtype == np.bool_ and got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got.reshape(-1) != want.reshape(-1))
        raise AssertionError(f"{what}: {len(bad)} verdicts differ, first at {bad[0][0]}")


def kernel_name(r):
    return r.launch_info().kernel.decode()


def tile(r):
    li = r.launch_info()
    return li.tile_x, li.tile_z


def lights_of(oscene):
    return [np.array(oscene.get_object(i).origin.tuple(), dtype=np.float32)
            for i in range(oscene.object_count) if oscene.get_object(i).is_light]


def segments_to(points, L):
    return np.ascontiguousarray(np.concatenate([points, np.broadcast_to(L, points.shape)], axis=-1), dtype=np.float32)


def unrelated_segments(rays, n, seed):
    """segments whose ends have nothing to do with each other: origins and ends drawn from different rays' points"""
    rng = np.random.default_rng(seed)
    pts = rays.reshape(-1, 6)
    a, b = pts[rng.integers(len(pts), size=n)], pts[rng.integers(len(pts), size=n)]
    s = np.empty((n, 6), dtype=np.float32)
    s[:, :3] = a[:, 3:] + rng.normal(scale=4.0, size=(n, 3)).astype(np.float32)
    s[:, 3:] = b[:, 3:] + rng.normal(scale=4.0, size=(n, 3)).astype(np.float32)
    return s


FAMILIES = [
    ("builtin", {}, 61, 37, "rt_render_kernel"),                                    # FAST tables
    ("builtin", {"fast": 0}, 45, 29, "rt_render_kernel_items"),                     # the item tables
    ("grid16", {}, 50, 43, "rt_render_kernel_clusters"),                            # clustered sphere runs
    ("grid32", {"wide": 0}, 40, 35, "rt_render_kernel_clusters"),
    ("grid32", {"wide": 1}, 40, 35, "rt_render_kernel_clusters_wide"),
    ("twomirrors", {"tables": 2}, 33, 27, "rt_render_kernel_large"),                # tables in global memory
]


def renderer(name, options):
    r = Renderer(HostScene.named(name))
    for k, v in options.items():
        r.set_option(k, v)
    return r


# ------------------------------------------------------------------------------------------------------------ hits, every family

@pytest.mark.parametrize("name,options,W,H,kernel", FAMILIES)
def test_hits_of_every_family(oracle, name, options, W, H, kernel):
    o = oracle.OracleScene.named(name)
    scene = query_ref.Scene(o)
    r = renderer(name, options)
    rays = camera_rays(r._cam, W, H)
    got = r.intersect_rays(rays)                                   # (W, H, 6): rows = H, the image's tiles
    assert kernel_name(r) == kernel + "_hits"
    want = query_ref.intersect(scene, rays)
    assert (want["object"] >= 0).any()
    assert_hits_same(got, want, f"{name} {options}")
    flat = rays.reshape(-1, 6)
    perm = np.random.default_rng(W).permutation(len(flat))
    shuffled = r.intersect_rays(np.ascontiguousarray(flat[perm]))
    assert kernel_name(r) == kernel + "_hits"
    assert_hits_same(shuffled, want.reshape(-1)[perm], f"{name} {options} shuffled")


def test_hits_of_the_whole_bench_frame():
    r = Renderer(HostScene.builtin())
    import oracle_lib
    rays = camera_rays(r._cam, 4096, 4096)
    got = r.intersect_rays(rays)
    assert kernel_name(r) == "rt_render_kernel_hits"
    assert_hits_same(got, query_ref.intersect(query_ref.Scene(oracle_lib.OracleScene.builtin()), rays), "4096^2")


@pytest.mark.parametrize("seed,case", enumerate(["fisheye", "in_spheres", "on_planes", "outside", "shuffled"]))
def test_hits_of_incoherent_rays(oracle, seed, case):
    o = oracle.OracleScene.builtin()
    r = Renderer(HostScene.builtin())
    rays = incoherent_rays(o, camera_rays(o.cam, 96, 80), case, 4000, seed)
    got = r.intersect_rays(rays)
    want = query_ref.intersect(query_ref.Scene(o), rays)
    assert_hits_same(got, want, case)
    if case == "in_spheres":
        assert (want["flags"] & 1).any()                           # inside hits, with their negative distances
        assert (want["distance"][(want["flags"] & 1) == 1] < 0).all()


@pytest.mark.parametrize("seed", range(1, 13))
def test_hits_and_verdicts_of_random_scenes(oracle, seed):
    from scene_gen import build_random
    host = build_random(HostScene.empty(), seed, shadows=(seed % 3 != 0))
    orc = build_random(oracle.OracleScene(), seed, shadows=(seed % 3 != 0))
    scene = query_ref.Scene(orc)
    r = Renderer(host)
    case = ("shuffled", "in_spheres", "on_planes", "outside")[seed % 4]
    rays = incoherent_rays(orc, camera_rays(orc.cam, 80, 60), case, 1000, seed)
    hits = r.intersect_rays(rays)
    assert_hits_same(hits, query_ref.intersect(scene, rays), f"seed {seed} {case}")
    segs = np.concatenate([segments_to(hits["point"], L) for L in lights_of(orc)] + [unrelated_segments(rays, 500, seed)])
    assert_verdicts_same(r.occluded_rays(segs), query_ref.occluded(scene, segs), f"seed {seed} segments")


# --------------------------------------------------------------------------------------------------------- occluded, every family

@pytest.mark.parametrize("name,options,W,H,kernel", FAMILIES)
def test_verdicts_of_every_family(oracle, name, options, W, H, kernel):
    o = oracle.OracleScene.named(name)
    scene = query_ref.Scene(o)
    r = renderer(name, options)
    rays = camera_rays(r._cam, W, H)
    hits = r.intersect_rays(rays)
    for k, L in enumerate(lights_of(o)):
        segs = segments_to(hits["point"], L)                       # (W, H, 6): the shading's shadow rays of level 0
        got = r.occluded_rays(segs)
        assert kernel_name(r) == kernel + "_occluded"
        want = query_ref.occluded(scene, segs)
        assert_verdicts_same(got, want, f"{name} {options} light {k}")
    segs = unrelated_segments(rays, 3000, W)                       # the generalised bundle cull
    want = query_ref.occluded(scene, segs)
    assert_verdicts_same(r.occluded_rays(segs), want, f"{name} {options} unrelated segments")
    assert_verdicts_same(r.occluded_rays(segs, rows=64), want, f"{name} {options} unrelated segments, rows 64")


@pytest.mark.parametrize("bad", ["target_is_origin", "huge", "inf_origin", "inf_target", "nan_origin", "nan_target",
                                 "huge_origin"])
@pytest.mark.parametrize("lane", [0, 37, 63])
def test_a_degenerate_lane_leaves_its_wavefront_exact(oracle, bad, lane):
    o = oracle.OracleScene.builtin()
    scene = query_ref.Scene(o)
    r = Renderer(HostScene.builtin())
    rays = incoherent_rays(o, camera_rays(o.cam, 96, 80), "shuffled", 64, seed=lane)     # one flat wavefront: a 1 x 64 tile
    segs = segments_to(query_ref.intersect(scene, rays)["point"], lights_of(o)[0])
    for batch in (rays, segs):
        e, t = batch[lane, :3], batch[lane, 3:]
        if bad == "target_is_origin":
            t[:] = e
        elif bad == "huge":
            t[1] = np.float32(1e30)
        elif bad == "huge_origin":
            e[0] = np.float32(-1e30)
        elif bad == "inf_origin":
            e[2] = np.float32(np.inf)
        elif bad == "inf_target":
            t[0] = np.float32(-np.inf)
        elif bad == "nan_origin":
            e[1] = np.float32(np.nan)
        elif bad == "nan_target":
            t[2] = np.float32(np.nan)
    assert_hits_same(r.intersect_rays(rays), query_ref.intersect(scene, rays), f"{bad} at lane {lane}")
    assert tile(r) == (1, 64)
    assert_verdicts_same(r.occluded_rays(segs), query_ref.occluded(scene, segs), f"{bad} at lane {lane}, segments")
    assert tile(r) == (1, 64)


# ---------------------------------------------------------------------------------------------------- layouts and options

@pytest.mark.parametrize("n", [1, 63, 65, 1009])
def test_rows_and_order_never_change_a_result(oracle, n):
    o = oracle.OracleScene.builtin()
    scene = query_ref.Scene(o)
    r = Renderer(HostScene.builtin())
    rays = incoherent_rays(o, camera_rays(o.cam, 64, 48), "shuffled", n, seed=n)
    segs = unrelated_segments(camera_rays(o.cam, 64, 48), n, seed=n)
    want_h, want_o = query_ref.intersect(scene, rays), query_ref.occluded(scene, segs)
    perm = np.random.default_rng(n).permutation(n)
    for rows in (None, 1, 7, 64, n, n + 5):
        assert_hits_same(r.intersect_rays(rays, rows=rows), want_h, f"n {n} rows {rows}")
        assert_verdicts_same(r.occluded_rays(segs, rows=rows), want_o, f"n {n} rows {rows}")
    assert_hits_same(r.intersect_rays(np.ascontiguousarray(rays[perm]), rows=7), want_h[perm], f"n {n} permuted")
    assert_verdicts_same(r.occluded_rays(np.ascontiguousarray(segs[perm]), rows=7), want_o[perm], f"n {n} permuted")


def test_an_empty_batch_writes_nothing():
    lib = capi.load_library()
    r = Renderer(HostScene.builtin())
    hits = np.full(4, 7, dtype=HIT_DTYPE)
    blocked = np.full(4, 7, dtype=np.uint8)
    z = np.zeros(6, np.float32).ctypes.data
    for fn, out in ((lib.rt_intersect_rays, hits), (lib.rt_occluded_rays, blocked)):
        assert fn(r._scene, 0, 1, None, None) == capi.RT_OK
        assert fn(r._scene, 0, 5, z, out.ctypes.data) == capi.RT_OK
    for fn in (lib.rt_intersect_rays_device, lib.rt_occluded_rays_device):
        assert fn(r._scene, 0, 1, None, None, None) == capi.RT_OK
    assert (hits["object"] == 7).all() and (blocked == 7).all()
    assert r.intersect_rays(np.zeros((0, 6), np.float32)).shape == (0,)
    assert r.occluded_rays(np.zeros((0, 6), np.float32)).shape == (0,)


def test_speed_options_give_the_same_bits(oracle):
    for name, W, H in (("grid16", 40, 36), ("builtin", 48, 40)):
        o = oracle.OracleScene.named(name)
        scene = query_ref.Scene(o)
        rays = camera_rays(o.cam, W, H)
        want_h = query_ref.intersect(scene, rays)
        segs = np.concatenate([segments_to(want_h["point"], lights_of(o)[0]).reshape(-1, 6),
                               unrelated_segments(rays, 1000, W)])
        want_o = query_ref.occluded(scene, segs)
        for key, value in (("cull", 0), ("fast", 0), ("tables", 2), ("tile_z", 1), ("tile_z", 16), ("tile_z", 64),
                           ("first_row", 500), ("tile_prio", 1), ("help", 1)):
            r = Renderer(HostScene.named(name))
            r.set_option(key, value)
            assert_hits_same(r.intersect_rays(rays), want_h, f"{name} {key} {value}")
            assert kernel_name(r).endswith("_hits")
            assert_verdicts_same(r.occluded_rays(segs), want_o, f"{name} {key} {value}")
            assert kernel_name(r).endswith("_occluded")


# -------------------------------------------------------------------------------------------- device entry points, one handle

def test_device_entry_points_on_a_stream(oracle):
    import torch
    o = oracle.OracleScene.builtin()
    r = Renderer(HostScene.builtin())
    W, H = 120, 72
    rays = camera_rays(r._cam, W, H)
    want_h = r.intersect_rays(rays)
    segs = segments_to(want_h["point"], lights_of(o)[0])
    want_o = r.occluded_rays(segs)
    d_rays = torch.from_numpy(rays).to("cuda:0")
    d_segs = torch.from_numpy(segs).to("cuda:0")
    hits = torch.full((W * H * 12,), -1.0, dtype=torch.float32, device="cuda:0")
    blocked = torch.full((W * H,), 7, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        r.intersect_rays_device(W * H, H, d_rays.data_ptr(), hits.data_ptr(), stream.cuda_stream)
        r.occluded_rays_device(W * H, H, d_segs.data_ptr(), blocked.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert kernel_name(r) == "rt_render_kernel_occluded"
    assert_hits_same(hits.cpu().numpy().view(HIT_DTYPE).reshape(W, H), want_h, "intersect_rays_device")
    assert_verdicts_same(blocked.cpu().numpy().view(np.bool_).reshape(W, H), want_o, "occluded_rays_device")
    assert r.timing().last_kernel_ms > 0


def test_one_handle_interleaved_with_trace_rays_and_four_threads(oracle):
    from rays_ref import oracle_trace
    name, W, H = "builtin", 48, 40
    o = oracle.OracleScene.named(name)
    scene = query_ref.Scene(o)
    rays = camera_rays(o.cam, W, H)
    want_rgb = o.render(W, H, 3)
    want_h = query_ref.intersect(scene, rays)
    segs = unrelated_segments(rays, 800, 5)
    want_o = query_ref.occluded(scene, segs)
    r = Renderer(HostScene.named(name))
    for _ in range(2):
        assert np.array_equal(r.trace_rays(rays, 3).view(np.uint32), want_rgb.view(np.uint32))
        assert_hits_same(r.intersect_rays(rays), want_h, "intersect")
        assert_verdicts_same(r.occluded_rays(segs), want_o, "occluded")
    errors = []

    def worker(k):
        try:
            for i in range(6):
                if (i + k) % 3 == 0:
                    assert np.array_equal(r.trace_rays(rays, 3).view(np.uint32), want_rgb.view(np.uint32))
                elif (i + k) % 3 == 1:
                    assert_hits_same(r.intersect_rays(rays), want_h, f"thread {k}, call {i}")
                else:
                    assert_verdicts_same(r.occluded_rays(segs), want_o, f"thread {k}, call {i}")
        except Exception as e:                                     # pragma: no cover - reported below
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]
    assert oracle_trace is not None


# --------------------------------------------------------------------------------------------------------- invalid arguments

def test_invalid_arguments_in_the_contracts_order(oracle):
    lib = capi.load_library()
    r = Renderer(HostScene.builtin())
    rays = np.zeros((8, 6), dtype=np.float32)
    rp = rays.ctypes.data
    hits = np.zeros(8, dtype=HIT_DTYPE)
    blocked = np.zeros(8, dtype=np.uint8)
    for fn, dev, op in ((lib.rt_intersect_rays, lib.rt_intersect_rays_device, hits.ctypes.data),
                        (lib.rt_occluded_rays, lib.rt_occluded_rays_device, blocked.ctypes.data)):
        cases = [
            ((None, 8, 8, rp, op), b"scene"),
            ((r._scene, -1, 0, None, None), b"n < 0"),
            ((r._scene, 8, 0, None, None), b"rows"),
            ((r._scene, 8, -3, rp, op), b"rows"),
            ((r._scene, 8, 8, None, None), b"rays"),
            ((r._scene, 8, 8, rp, None), b"output"),
            ((r._scene, 0x7fffffff, 0x40000001, rp, op), b"too large"),     # a grid of 2^31 + 2 cells (nothing is read)
            ((r._scene, 0x7fffffff, 0x7fffffff, rp, op), b"too large"),
        ]
        for args, text in cases:
            assert fn(*args) == capi.RT_ERR_INVALID, args
            assert text in lib.rt_last_error(), (args, lib.rt_last_error())
            assert dev(*args, None) == capi.RT_ERR_INVALID, args
            assert text in lib.rt_last_error(), (args, lib.rt_last_error())
    assert (hits["object"] == 0).all() and (blocked == 0).all()
    with pytest.raises(RtError):
        r.intersect_rays(rays, rows=0)
    with pytest.raises(RtError):
        r.occluded_rays(rays, rows=0)
    with pytest.raises(TypeError):
        r.intersect_rays(rays.astype(np.float64))
    with pytest.raises(ValueError):
        r.occluded_rays(np.zeros((8, 5), np.float32))
    o = oracle.OracleScene.builtin()                               # the scene still answers
    cam = camera_rays(o.cam, 20, 16)
    assert_hits_same(r.intersect_rays(cam), query_ref.intersect(query_ref.Scene(o), cam), "afterwards")
