"""bench.py --dump-outputs DIR: after the timed steps, what the last timed step computed lands in DIR/<name>.npy -- the
whole image, or a fixed seeded sample of a large one, 64 MB at most in all -- and --steps is exactly the number of timed
steps.  The helpers run without a GPU; the runs of bench.py itself are GPU tests."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_steps_and_dump_outputs_arguments():
    a = bench.parse_args(["--steps", "7", "--warmup", "0", "--dump-outputs", "some/dir"])
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == "some/dir"
    assert bench.parse_args([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_dump_image_writes_a_small_image_whole(tmp_path):
    img = np.random.default_rng(1).random((64, 48, 3), dtype=np.float32)
    path = bench.dump_image(str(tmp_path / "out"), "image", img)
    assert path == str(tmp_path / "out" / "image.npy")
    got = np.load(path)
    assert got.dtype == np.float32 and np.array_equal(got, img)


def test_dump_image_samples_a_large_image_with_a_fixed_seed(tmp_path):
    W, H = 1100, 1000                                  # 1.1 M pixels: more than DUMP_SAMPLE_PIXELS
    img = np.random.default_rng(2).random((W, H, 3), dtype=np.float32)
    got = np.load(bench.dump_image(str(tmp_path), "image", img))
    index = bench.dump_sample_index(W * H)
    assert got.shape == (bench.DUMP_SAMPLE_PIXELS, 3) and got.dtype == np.float32
    assert np.array_equal(got, img.reshape(-1, 3)[index])
    assert np.array_equal(index, bench.dump_sample_index(W * H))           # the same pixels on every run
    assert np.all(np.diff(index) > 0) and index[0] >= 0 and index[-1] < W * H
    # two such images (headline + sphere grid) stay under the 64 MB the dumps may take
    assert 2 * os.path.getsize(tmp_path / "image.npy") < 64e6
    assert bench.dump_sample_index(bench.DUMP_SAMPLE_PIXELS) is None


def test_read_screen_txt_reads_back_what_the_writer_wrote(tmp_path):
    from tilecoderaytracer_amd.host import write_screen_txt
    W, H = 5, 7
    img = ((np.arange(W * H * 3) % 97 - 40) / 64.0).astype(np.float32).reshape(W, H, 3)   # exact in six decimals
    p = str(tmp_path / "raytracer_screen.txt")
    write_screen_txt(p, img, 0.25, 1.0)
    got = bench.read_screen_txt(p, W, H)
    assert got.dtype == np.float64 and np.array_equal(got, img.astype(np.float64))
    with pytest.raises(ValueError):
        bench.read_screen_txt(p, W, H + 1)


def run_bench(args, env=None, timeout=900):
    out = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=timeout, cwd=ROOT,
                         env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dumps_the_last_frame_of_a_small_run(oracle, tmp_path):
    d = tmp_path / "dump"
    j = run_bench(["--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--no-extra", "--workload", "grid16d8", "--size", "128",
                   "--dump-outputs", str(d)])
    assert j["steps"] == 4
    assert sorted(os.listdir(d)) == ["image.npy"]
    got = np.load(d / "image.npy")
    want = oracle.OracleScene.named("grid16").render(128, 128, 8)
    assert got.dtype == np.float32 and got.shape == (128, 128, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_bench_dumps_a_seeded_sample_of_the_default_workload(tmp_path):
    from tilecoderaytracer_amd import HostScene, Renderer
    d = tmp_path / "dump"
    j = run_bench(["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", str(d)])
    assert j["steps"] == 2 and j["sphere_grid"]["steps"] >= 1
    assert sorted(os.listdir(d)) == ["image.npy", "sphere_grid_image.npy"]
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64e6
    index = bench.dump_sample_index(4096 * 4096)
    for name, scene, depth in (("image", "builtin", 4), ("sphere_grid_image", "grid32", 4)):
        got = np.load(d / f"{name}.npy")
        frame = Renderer(HostScene.named(scene)).render(4096, 4096, depth)
        assert got.dtype == np.float32 and got.shape == (bench.DUMP_SAMPLE_PIXELS, 3)
        assert np.array_equal(got.view(np.uint32), frame.reshape(-1, 3)[index].view(np.uint32)), name


@pytest.mark.gpu
def test_bench_two_ranks_dump_rank_0s_image(tmp_path):
    """N = 2 (both ranks on the one GPU, gloo control collectives, the direct transport): rank 0 writes the image the strips
    were stored into, and it is one GPU's frame."""
    from tilecoderaytracer_amd import HostScene, Renderer
    env = dict(os.environ, TCRT_BENCH_ONE_DEVICE="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    d = tmp_path / "dump"
    j = run_bench(["--gpus", "2", "--steps", "3", "--warmup", "3", "--backend", "gloo", "--size", "512", "--no-pipelined",
                   "--dump-outputs", str(d)], env=env)
    assert j["n_gpus"] == 2 and j["steps"] == 3
    assert sorted(os.listdir(d)) == ["image.npy"]
    got = np.load(d / "image.npy")
    want = Renderer(HostScene.named("builtin")).render(512, 512, 4)
    assert got.shape == (512, 512, 3) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_bench_shipped_workload_takes_every_step_and_dumps_its_text(oracle, tmp_path):
    from tilecoderaytracer_amd.host import write_screen_txt
    d = tmp_path / "dump"
    j = run_bench(["--workload", "shipped512", "--steps", "11", "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", str(d)])
    assert j["steps"] == 11 and len(j["config"]["runs_s"]) == 11
    got = np.load(d / "image.npy")
    p = str(tmp_path / "oracle_screen.txt")
    write_screen_txt(p, oracle.OracleScene.named("builtin").render(512, 512, 3))
    assert got.dtype == np.float64 and np.array_equal(got, bench.read_screen_txt(p, 512, 512))
