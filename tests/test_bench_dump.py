"""bench.py --dump-outputs: the accumulators the timed region left, written as .npy files (float32 / float64, at most 64 MB,
a seeded pixel sample above DUMP_MAX_PIXELS), --steps as the exact number of timed samples, and what a plain run leaves to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("summed_image", "summed_sample_weights", "summed_sample_counts", "unidirectional_image")


class _FakeRenderer:
    """Stands in for Renderer.read_accumulators(): distinct values in every pixel and channel."""

    def __init__(self, W, H, samples=3):
        rng = np.random.default_rng(7)
        self.acc = (rng.random((H, W, 3), dtype=np.float32), rng.random((H, W, 1), dtype=np.float32),
                    np.full((H, W, 1), samples, np.int32), rng.random((H, W, 3), dtype=np.float32))

    def read_accumulators(self):
        return self.acc


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_whole_accumulators_of_a_small_frame(tmp_path):
    import bench
    r = _FakeRenderer(64, 48)
    shapes = bench.dump_outputs(str(tmp_path / "d"), r)
    got = _load(tmp_path / "d")
    assert sorted(got) == sorted(NAMES) and shapes == {k: list(v.shape) for k, v in got.items()}
    for name, ref in zip(NAMES, r.acc):
        assert got[name].dtype == np.float32 and got[name].shape == ref.shape
        assert np.array_equal(got[name], ref.astype(np.float32))


def test_dump_of_a_large_frame_is_a_fixed_seeded_sample_within_64_mb(tmp_path):
    import bench
    W, H = 1920, 1080
    r = _FakeRenderer(W, H)
    bench.dump_outputs(str(tmp_path / "a"), r)
    bench.dump_outputs(str(tmp_path / "b"), _FakeRenderer(W, H))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(NAMES + ("pixel_index",))
    assert sum(os.path.getsize(tmp_path / "a" / f"{k}.npy") for k in a) <= 64 * 10 ** 6
    idx = a["pixel_index"]
    assert idx.dtype == np.float64 and len(idx) == bench.DUMP_MAX_PIXELS
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < W * H and np.array_equal(idx, np.round(idx))
    rows = idx.astype(np.int64)
    for name, ref in zip(NAMES, r.acc):
        assert a[name].dtype == np.float32
        assert np.array_equal(a[name], ref.reshape(W * H, -1)[rows].astype(np.float32))
    for k in a:                                                     # same pixels, same values on every run
        assert np.array_equal(a[k], b[k])


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "3", "--sample-streams", "2"], ["--sample-streams", "0"],
                                  ["--full", "--steps", "0"]])
def test_bench_refuses_steps_it_would_not_time_exactly(argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and p.stdout == "" and "must be" in p.stderr


@pytest.mark.gpu
def test_bench_dumps_the_timed_samples_identically_from_run_to_run(tmp_path):
    """Two runs of the same command: the dumped accumulators hold exactly --steps samples in every pixel and agree to the
    tolerance smoke() holds the device to against the oracle (the light splat adds with float atomics)."""
    runs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--width", "64", "--height", "48", "--steps", "3",
                            "--warmup", "1", "--no-mesh", "--no-cpu-baseline", "--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads(p.stdout)
        assert line["steps"] == 3 and line["config"]["samples_rendered_all_ranks"] == 3
        runs.append(_load(d))
    a, b = runs
    assert sorted(a) == sorted(NAMES)
    assert a["summed_image"].shape == (48, 64, 3) and a["summed_sample_weights"].shape == (48, 64, 1)
    assert (a["summed_sample_counts"] == 3).all() and (b["summed_sample_counts"] == 3).all()
    for name in NAMES:
        assert a[name].dtype == np.float32 and np.isfinite(a[name]).all()
        assert np.allclose(a[name], b[name], rtol=1e-5, atol=1e-7), name
    assert a["summed_image"].any()


@pytest.mark.gpu
def test_plain_run_does_only_the_headline_and_full_adds_the_rest(tmp_path):
    """A plain run times the steps and prints the line, nothing else: no stage breakdown, serial loop, legs or CPU baseline.
    `--full` adds them after the clock and changes nothing before or inside it: both runs dump the same accumulators."""
    common = ["--width", "64", "--height", "48", "--steps", "3", "--warmup", "1"]
    extra = {"plain": [], "full": ["--full", "--no-mesh", "--cpu-width", "64", "--cpu-height", "48", "--cpu-samples", "1"]}
    lines, dumps = {}, {}
    for kind, argv in extra.items():
        d = tmp_path / kind
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + argv + ["--dump-outputs", str(d)],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        lines[kind] = json.loads(p.stdout)
        dumps[kind] = _load(d)
    plain, full = lines["plain"], lines["full"]
    for key in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup"):
        assert plain[key] == full[key], key
    assert plain["steps"] == 3 and plain["config"]["samples_rendered_all_ranks"] == 3
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["roofline"]["avg_launch_ms"] > 0
    assert not {"stage_ms", "serial_ms", "legs", "cpu_baseline", "strong_scaling"} & set(plain)
    assert "avg_launch_ms_alone" not in plain["roofline"]
    assert {"stage_ms", "cpu_baseline"} <= set(full) and full["roofline"]["avg_launch_ms_alone"] > 0
    assert "legs" not in full                                       # --no-mesh still trims --full
    assert (dumps["plain"]["summed_sample_counts"] == 3).all() and (dumps["full"]["summed_sample_counts"] == 3).all()
    for name in NAMES:
        assert np.allclose(dumps["plain"][name], dumps["full"][name], rtol=1e-5, atol=1e-7), name
