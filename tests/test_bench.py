"""bench.py: a plain run times exactly --steps launches and reports only the headline figure; --dump-outputs writes what the
last timed launch produced, the same positions for the same arguments."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


class _HostBatch:
    """The geometry and download_frame of a DeviceBatch, over frames in host memory."""

    def __init__(self, frames):
        self.n, self.h, self.w = frames.shape
        self.frames = frames

    def download_frame(self, f):
        return self.frames[f]


def test_dump_outputs_is_a_fixed_seeded_sample_within_budget(tmp_path, monkeypatch):
    bench = _bench("bench_dump")
    assert bench.DUMP_FRAME_BYTES + 4 * bench.DUMP_SAMPLES <= 64e6
    frames = bench.make_frames(64, 48, 6, 10, seed=1)
    batch = _HostBatch(frames)
    monkeypatch.setattr(bench, "DUMP_SAMPLES", 5000)       # fewer samples than the batch holds
    bench.dump_outputs(batch, str(tmp_path / "a"))
    bench.dump_outputs(batch, str(tmp_path / "b"))
    f0 = np.load(tmp_path / "a" / "filtered_frame0.npy")
    assert f0.dtype == np.float32 and np.array_equal(f0, frames[0])
    s = np.load(tmp_path / "a" / "filtered_sample.npy")
    pos = np.unique(np.random.default_rng(0).integers(0, frames.size, 5000))
    assert s.dtype == np.float32 and s.size > 4000 and np.array_equal(s, frames.ravel()[pos])
    assert np.array_equal(s, np.load(tmp_path / "b" / "filtered_sample.npy"))
    monkeypatch.setattr(bench, "DUMP_SAMPLES", frames.size)  # a batch that fits: all of it, in order
    bench.dump_outputs(batch, str(tmp_path / "c"))
    assert np.array_equal(np.load(tmp_path / "c" / "filtered_sample.npy"), frames.ravel())


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_launch(tmp_path, oracle):
    out = tmp_path / "dump"
    w, h, F, steps = 256, 128, 8, 7
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--width", str(w),
           "--height", str(h), "--frames", str(F), "--settle-max-ms", "0", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert (res["metric"], res["unit"], res["higher_is_better"], res["dtype"]) == ("luma_frames_per_sec", "frames/s", True, "int16")
    assert res["steps"] == steps and res["ms_per_step"] > 0 and res["value"] == pytest.approx(F * 1e3 / res["ms_per_step"])
    assert not {"extra_configs", "cpu_baseline", "reference_table_352x288", "e2e_host_frame"} & set(res)
    assert res["bit_exact_vs_oracle"] is None and res["cross_rank"] is None    # checks belong to --full
    want = np.stack([oracle.filter_plane(fr, 32) for fr in _bench("bench_frames").make_frames(w, h, F, 8, seed=1)])
    assert np.array_equal(np.load(out / "filtered_frame0.npy"), want[0].astype(np.float32))
    assert np.array_equal(np.load(out / "filtered_sample.npy"), want.ravel().astype(np.float32))
