"""bench.py's own contract: a plain run prints the headline only and times exactly --steps steps, everything else is behind --full;
--dump-outputs writes the frame of the last timed step as float32 / float64 arrays, the same for every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_a_fixed_sample_and_every_row(tmp_path):
    import bench
    rng = np.random.default_rng(3)
    image = rng.integers(0, 256, (1100, 1024, 4), dtype=np.uint8)  # more pixels than the sample
    bench.dump_outputs(str(tmp_path / "a"), image)
    bench.dump_outputs(str(tmp_path / "b"), image)
    sample = np.load(tmp_path / "a" / "frame_sample.npy")
    rows = np.load(tmp_path / "a" / "frame_row_sums.npy")
    assert sample.dtype == np.float32 and sample.shape == (bench.DUMP_SAMPLE_PIXELS, 4)
    assert rows.dtype == np.float64 and rows.shape == (1100, 4)
    assert np.array_equal(rows, image.astype(np.float64).sum(axis=1))
    index = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(1100 * 1024, size=bench.DUMP_SAMPLE_PIXELS, replace=False))
    assert np.array_equal(sample, image.reshape(-1, 4)[index].astype(np.float32))
    for name in ("frame_sample.npy", "frame_row_sums.npy"):  # the same arguments give the same files
        assert (tmp_path / "a" / name).read_bytes() == (tmp_path / "b" / name).read_bytes()
    # the largest frame the benchmark draws (8192 x 8192) stays far below 64 MB
    assert bench.DUMP_SAMPLE_PIXELS * 4 * 4 + 8192 * 4 * 8 < 64 << 20


@pytest.mark.parametrize("argv, message", [(["--check"], "--check is part of --full"), (["--steps", "0"], "--steps must be at least 1")])
def test_bench_refuses_options_it_cannot_honour(argv, message):
    done = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert done.returncode == 2 and message in done.stderr, done.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_frame(oracle_lib, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` without --full: one line with the headline keys and none of the --full blocks; the dumped
    frame is the oracle's frame of the same scene (512 x 512: the sample is every pixel, in order)."""
    from contrast_renderer_amd import scenes
    out = tmp_path / "dump"
    done = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--paths", "400", "--size", "512",
                           "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert done.returncode == 0, done.stderr[-2000:]
    lines = [l for l in done.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, done.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["n_gpus"] == 1
    assert line["unit"] == "paths/s" and line["higher_is_better"] is True and line["dtype"] == "f32" and line["metric"].startswith("paths/sec")
    assert line["value"] > 0 and abs(line["value"] - 400 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert not {"kernels", "roofline", "spread", "latency_ms_per_step", "animated", "check", "reupload", "other_workloads", "cpu_baseline"} & set(line)
    sample = np.load(out / "frame_sample.npy")
    rows = np.load(out / "frame_row_sums.npy")
    assert sample.dtype == np.float32 and rows.dtype == np.float64
    sc = scenes.scene_cubic_fill(400, (512, 512), config_index=2)
    expect = oracle_lib.Oracle(sc["batch"]).render(512, 512, sc["msaa"], 4, sc["transforms"], sc["colors"])
    assert np.array_equal(sample, expect.reshape(-1, 4).astype(np.float32))
    assert np.array_equal(rows, expect.astype(np.float64).sum(axis=1))
    assert (expect[..., 3] > 0).any()
