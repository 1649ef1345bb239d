"""k x k supersampling averaged inside the render kernel (include/rt_capi_ssaa.h) against its definition: the oracle's
virtual kW x kH frame (or the GPU's own rt_render of it), box-filtered in numpy (ssaa_ref.box_filter).  Bar: BIT-EXACT."""
import os

import numpy as np
import pytest

from tilecoderaytracer_amd import HostScene, Renderer, RtError, capi
from ssaa_ref import box_filter

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assert_same(gpu, ref, what):
    assert gpu.shape == ref.shape, (what, gpu.shape, ref.shape)
    same = gpu.view(np.uint32) == ref.view(np.uint32)
    if not same.all():
        bad = np.argwhere(~same.all(axis=-1))
        diff = np.abs(gpu.astype(np.float64) - ref.astype(np.float64))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, max |d|={np.nanmax(diff):.3g}, "
                             f"first at {bad[0].tolist()}: gpu={gpu[tuple(bad[0])]} ref={ref[tuple(bad[0])]}")


def kernel_name(r):
    return r.launch_info().kernel.decode()


def check_against(r, want_virtual, W, H, depth, k, what, x0=0, x1=None):
    """rt_render_ssaa(W, H, k) == the box-filtered virtual frame; the kernel is the *_ssaa sibling of the one rt_render runs
    on the virtual frame, and rt_render of the virtual frame on the GPU filters to the same image."""
    x1 = W if x1 is None else x1
    plain = r.render(k * W, k * H, depth, k * x0, k * x1)
    plain_kernel = kernel_name(r)
    got = r.render_ssaa(W, H, depth, k, x0, x1)
    assert kernel_name(r) == plain_kernel + "_ssaa", (what, plain_kernel, kernel_name(r))
    want = box_filter(want_virtual, k)
    assert_same(got, want, what)
    assert_same(box_filter(plain, k), want, what + " (the GPU's own virtual frame)")
    return got


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("name,W,H,depth,family", [
    ("builtin", 250, 252, 3, "rt_render_kernel"),               # FAST tables
    ("builtin", 61, 37, 4, "rt_render_kernel"),                 # sizes that are not multiples of a tile
    ("grid16", 96, 96, 8, "rt_render_kernel_clusters"),         # clustered sphere runs
    ("grid32", 64, 64, 4, "rt_render_kernel_clusters"),
])
def test_against_the_oracle(oracle, name, W, H, depth, family, k):
    r = Renderer(HostScene.named(name))
    want = oracle.OracleScene.named(name).render(k * W, k * H, depth)
    check_against(r, want, W, H, depth, k, f"{name} {W}x{H} d{depth} k{k}")
    assert kernel_name(r).startswith(family) and kernel_name(r).endswith("_ssaa")


@pytest.mark.parametrize("k", [2, 4])
def test_tables_in_global_memory(oracle, k):
    """The reference's SCENE 2 (3 920 objects) with option tables = 2: rt_render_kernel_large_ssaa."""
    r = Renderer(HostScene.two_mirrors())
    r.set_option("tables", 2)
    W, H, depth = 40, 36, 6
    want = oracle.OracleScene.two_mirrors().render(k * W, k * H, depth)
    check_against(r, want, W, H, depth, k, f"twomirrors k{k}")
    assert kernel_name(r) == "rt_render_kernel_large_ssaa"


@pytest.mark.parametrize("k", [2, 4])
def test_plain_scans(oracle, k):
    """Option cull = 0: the item tables' kernel, rt_render_kernel_items_ssaa."""
    r = Renderer(HostScene.builtin())
    r.set_option("cull", 0)
    W, H, depth = 70, 50, 4
    want = oracle.OracleScene.builtin().render(k * W, k * H, depth)
    check_against(r, want, W, H, depth, k, f"cull 0 k{k}")
    assert kernel_name(r) == "rt_render_kernel_items_ssaa"


@pytest.mark.parametrize("seed", [1, 2, 3, 5, 8, 11])
def test_random_scenes(oracle, seed):
    from scene_gen import build_random
    k = 2 if seed % 2 else 4
    host = build_random(HostScene.empty(), seed, shadows=(seed % 3 != 0))
    orc = build_random(oracle.OracleScene(), seed, shadows=(seed % 3 != 0))
    W, H, depth = 36, 28, 5
    check_against(Renderer(host), orc.render(k * W, k * H, depth), W, H, depth, k, f"seed {seed} k{k}")


def test_large_frame_equals_the_gpus_own_virtual_frame():
    """2048^2 at k = 2: the 4096^2 frame of rt_render (itself pinned to the oracle by test_parity_gpu), box-filtered."""
    r = Renderer(HostScene.builtin())
    virtual = r.render(4096, 4096, 4)
    assert kernel_name(r) == "rt_render_kernel"
    got = r.render_ssaa(2048, 2048, 4, 2)
    assert kernel_name(r) == "rt_render_kernel_ssaa"
    assert_same(got, box_filter(virtual, 2), "builtin 2048^2 k2")


@pytest.mark.parametrize("name,k", [("builtin", 2), ("builtin", 4), ("grid16", 2), ("grid16", 4)])
def test_strips_equal_the_whole_frames_columns(name, k):
    r = Renderer(HostScene.named(name))
    W, H, depth = 150, 90, 5
    full = r.render_ssaa(W, H, depth, k)
    for x0, x1 in ((0, 24), (24, 61), (61, 150), (149, 150), (13, 14), (1, 149), (7, 7)):
        assert_same(r.render_ssaa(W, H, depth, k, x0, x1), full[x0:x1], f"{name} k{k} strip {x0}:{x1}")


def test_device_entry_point_on_a_stream():
    import torch
    r = Renderer(HostScene.builtin())
    W, H, depth = 120, 72, 4
    for k in (1, 2, 4):
        want = r.render_ssaa(W, H, depth, k, 20, 100)
        buf = torch.zeros((80, H, 3), dtype=torch.float32, device="cuda:0")
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            r.render_ssaa_device(W, H, depth, k, 20, 100, buf.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert_same(buf.cpu().numpy(), want, f"render_ssaa_device k{k}")
    assert r.timing().launches >= 6


@pytest.mark.parametrize("name", ["builtin", "grid16", "twomirrors"])
def test_one_sample_is_rt_render(name):
    r = Renderer(HostScene.named(name))
    W, H, depth = 64, 48, 4
    want = r.render(W, H, depth, 5, 60)
    plain_kernel = kernel_name(r)
    assert_same(r.render_ssaa(W, H, depth, 1, 5, 60), want, f"{name} k1")
    assert kernel_name(r) == plain_kernel and not plain_kernel.endswith("_ssaa")


@pytest.mark.parametrize("tile_z", [1, 2, 32, 64])
def test_tile_shapes_the_planner_must_override(oracle, tile_z):
    """Option tile_z asks for shapes that cannot hold whole k x k pixels: the SSAA launch takes the nearest that can."""
    r = Renderer(HostScene.builtin())
    r.set_option("tile_z", tile_z)
    W, H, depth = 75, 35, 4
    for k in (2, 4):
        want = box_filter(oracle.OracleScene.builtin().render(k * W, k * H, depth), k)
        assert_same(r.render_ssaa(W, H, depth, k), want, f"tile_z {tile_z} k{k}")
        li = r.launch_info()
        assert li.tile_z % k == 0 and li.tile_x % k == 0 and li.tile_x * li.tile_z == 64
        assert li.tile_z == min(max(tile_z, k), 64 // k)
        assert_same(r.render_ssaa(W, H, depth, k, 9, 58), want[9:58], f"tile_z {tile_z} k{k} strip")


def test_help_heavy_and_first_row(oracle):
    """Forced HELP (the desk from two wavefronts on), HEAVY tiles, and a start row: scheduling only."""
    name, W, H, depth, k = "grid16", 64, 80, 6, 2
    want = box_filter(oracle.OracleScene.named(name).render(k * W, k * H, depth), k)
    r = Renderer(HostScene.named(name))
    r.set_option("help", 2)
    assert_same(r.render_ssaa(W, H, depth, k), want, "help 2")
    assert_same(r.render_ssaa(W, H, depth, k, 10, 30), want[10:30], "help 2, strip")
    r.set_option("heavy", 3)
    assert_same(r.render_ssaa(W, H, depth, k, 3, 20), want[3:20], "help 2, heavy 3, strip")
    for first_row in (0, 333, 999):
        r.set_option("first_row", first_row)
        assert_same(r.render_ssaa(W, H, depth, k), want, f"first_row {first_row}")


def test_help_timeout_path_is_exact_and_reported(oracle):
    lib = capi.load_library()
    name, W, H, depth, k = "grid16", 48, 40, 8, 2
    want = box_filter(oracle.OracleScene.named(name).render(k * W, k * H, depth), k)
    r = Renderer(HostScene.named(name))
    r.set_option("help", 2)
    r.set_option("block_threads", 256)
    r.set_option("help_spin_limit", -1)
    out = np.zeros((W, H, 3), dtype=np.float32)
    rc = lib.rt_render_ssaa(r._scene, r._cam, W, H, 0, W, depth, k, out.ctypes.data)
    assert rc == capi.RT_ERR_HIP and b"HELP" in lib.rt_last_error()
    assert_same(out, want, "image of the launch whose HELP waits timed out")
    r.set_option("help_spin_limit", 1 << 22)
    assert_same(r.render_ssaa(W, H, depth, k), want, "the handle is usable afterwards")


@pytest.mark.parametrize("name,x0,x1", [("builtin", 0, 75), ("grid16", 10, 60)])
def test_learned_order_on_the_virtual_shape(oracle, name, x0, x1):
    W, H, depth, k = 75, 60, 5, 2
    want = box_filter(oracle.OracleScene.named(name).render(k * W, k * H, depth), k)[x0:x1]
    r = Renderer(HostScene.named(name))
    r.learn_tile_order(k * W, k * H, depth, k * x0, k * x1)
    for _ in range(2):
        assert_same(r.render_ssaa(W, H, depth, k, x0, x1), want, f"{name}, learned order")


@pytest.mark.parametrize("samples", [0, 3, 8, -1])
def test_bad_sample_counts_are_invalid(samples):
    lib = capi.load_library()
    r = Renderer(HostScene.builtin())
    out = np.zeros((16, 16, 3), dtype=np.float32)
    assert lib.rt_render_ssaa(r._scene, r._cam, 16, 16, 0, 16, 3, samples, out.ctypes.data) == capi.RT_ERR_INVALID
    assert b"samples" in lib.rt_last_error()
    assert lib.rt_render_ssaa_device(r._scene, r._cam, 16, 16, 0, 16, 3, samples, None, None) == capi.RT_ERR_INVALID
    assert b"samples" in lib.rt_last_error()
    with pytest.raises(RtError):
        r.render_ssaa(16, 16, 3, samples)


def test_bad_virtual_sizes_are_invalid():
    r = Renderer(HostScene.builtin())
    with pytest.raises(RtError):
        r.render_ssaa(1 << 30, 4, 3, 4, 0, 1)          # 4 W does not fit an int
    with pytest.raises(RtError):
        r.render_ssaa(16, 16, 3, 2, 10, 20)            # x1 > W
    with pytest.raises(RtError):
        r.render_ssaa(16, 16, -1, 2)


def test_executable_writes_the_supersampled_image(oracle, tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "tilecoderaytracer_amd", "bin", "tcrt_raytracer")
    out = tmp_path / "f.txt"
    run = subprocess.run([exe, "--width", "100", "--height", "100", "--ssaa", "2", "--out", str(out)],
                         check=True, stdout=subprocess.PIPE, cwd=tmp_path, timeout=300)
    assert b"Mrays/s" in run.stdout
    want = tmp_path / "want.txt"
    oracle.write_screen_txt(str(want), box_filter(oracle.OracleScene.builtin().render(200, 200, 50), 2), 0.0, 0.0)
    got_lines, want_lines = out.read_bytes().split(b"\n"), want.read_bytes().split(b"\n")
    got_pixels, want_pixels = [l for l in got_lines if l[:1] == b"("], [l for l in want_lines if l[:1] == b"("]
    assert len(want_pixels) == 100 * 100 and got_pixels == want_pixels
