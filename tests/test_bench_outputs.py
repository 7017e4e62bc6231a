"""bench.py's plain run (the headline figure only) and --dump-outputs (what the last timed step returned, for comparing builds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, relerr


def test_dump_outputs_keeps_to_64_mb_with_a_fixed_sample(tmp_path):
    """A frame above the 64 MB budget (4K: 99.5 MB) is written as a seeded sample of its pixels, the same pixels every time;
    a 1080p frame is written whole."""
    sys.path.insert(0, ROOT)
    import bench
    big = np.repeat(np.arange(2160 * 3840, dtype=np.float32)[:, None], 3, axis=1).reshape(2160, 3840, 3)      # every value = its pixel's index
    big[..., 1] *= -1
    bench.dump_outputs(str(tmp_path / "a"), {"denoised": big})
    bench.dump_outputs(str(tmp_path / "b"), {"denoised": big})
    a = np.load(tmp_path / "a" / "denoised_sample.npy")
    assert os.path.getsize(tmp_path / "a" / "denoised_sample.npy") <= 64 * 1024 * 1024
    assert a.dtype == np.float32 and a.shape[1] == 3 and a.shape[0] > 2160 * 3840 // 2
    assert np.array_equal(a, np.load(tmp_path / "b" / "denoised_sample.npy"))
    assert np.all(np.diff(a[:, 0]) > 0) and np.array_equal(a, big.reshape(-1, 3)[a[:, 0].astype(np.int64)])      # whole pixels, in order
    small = np.random.default_rng(0).random((1080, 1920, 3), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "c"), {"denoised": small})
    assert np.array_equal(np.load(tmp_path / "c" / "denoised.npy"), small)


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "2",
                        "--min-warmup-seconds", "0.1", "--dump-outputs", str(out_dir)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_reports_the_headline_and_dumps_the_last_timed_frame(tmp_path):
    """Without --full the line holds the headline figure and nothing that needs runs of its own; --steps sets the timed steps;
    two runs with the same arguments dump the same frame (the timed steps inherit the same converged history)."""
    line = _plain_run(tmp_path / "a")
    assert line["metric"].startswith("SVGF Mpixels/s (full pipeline) at 1080p") and line["unit"] == "Mpixels/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["steps"] == 6 and line["full"] is False
    assert abs(line["value"] * 1e6 * line["ms_per_step"] * 1e-3 - 1920 * 1080) <= 0.01 * 1920 * 1080
    for k in ("roofline", "latency_ms_sync", "cadence", "cpu_baseline", "telemetry", "kernels_us"):
        assert k not in line, k
    a = np.load(tmp_path / "a" / "denoised.npy")
    assert a.dtype == np.float32 and a.shape == (1080, 1920, 3) and np.isfinite(a).all() and a.max() > 0
    _plain_run(tmp_path / "b")
    b = np.load(tmp_path / "b" / "denoised.npy")
    assert relerr(b, a).max() <= 1e-4      # measured: 1.2e-6 (the history converges to the same state up to rounding)
