"""bench.py's plain run and --dump-outputs: a plain run reports the headline alone (the other
figures belong to --full), and the dumped array is the last timed step's host-readable frame,
float32, bit for bit the frame a one-process render gives; a frame above the size limit is
dumped as a fixed, seeded sample of its pixels."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

FULL_ONLY = ("device_resident", "frame_latency_ms", "trace_kernel_ms", "bvh_build_ms", "roofline", "copy_engine",
             "camera_path", "cpu_baseline", "queries_traced_per_frame", "query_occupancy", "issue_bound")


def _bench_module(monkeypatch):
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "16")            # bench.py sets it at import: restored afterwards
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_and_sampled(monkeypatch, tmp_path):
    bench = _bench_module(monkeypatch)
    rng = np.random.default_rng(1)
    frame = rng.integers(0, 2 ** 32, size=(37, 53), dtype=np.uint32)
    bench.dump_outputs(str(tmp_path / "a"), frame)
    a = np.load(tmp_path / "a" / "rgba.npy")
    assert a.dtype == np.float32 and a.shape == (37, 53, 4)
    assert np.array_equal(a.astype(np.uint8).reshape(37, 53 * 4).view(np.uint32), frame)
    # above the limit: the same sorted sample every time, within the limit
    monkeypatch.setattr(bench, "DUMP_LIMIT", 16 * 100)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), frame)
    b, c = np.load(tmp_path / "b" / "rgba.npy"), np.load(tmp_path / "c" / "rgba.npy")
    assert b.dtype == np.float32 and b.shape == (100, 4) and b.nbytes <= 16 * 100
    assert np.array_equal(b, c)
    idx = np.sort(np.random.default_rng(0).choice(37 * 53, 100, replace=False))
    assert np.array_equal(b, a.reshape(-1, 4)[idx])


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_its_frame(gpu, tmp_path):
    W, H, spp, steps = 320, 180, 2, 3
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--width", str(W), "--height", str(H), "--spp", str(spp), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 2 and d["full"] is False
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and d["value"] > 0
    # value = rays per frame over the step time (ms_per_step is printed rounded to 1e-4 ms)
    rel = 1e-4 / d["ms_per_step"] + 1e-6
    assert abs(d["value"] - d["rays_per_frame"] / (d["ms_per_step"] * 1e-3) / 1e6) <= rel * d["value"]
    assert not [k for k in FULL_ONLY if k in d], d.keys()
    assert sorted(os.listdir(out_dir)) == ["rgba.npy"]
    a = np.load(out_dir / "rgba.npy")
    assert a.dtype == np.float32 and a.shape == (H, W, 4)
    ref = gpu.Scene.load_json(scene_path("world8_stress"), W, H).render(spp=spp, want=("rgba",), stats=True)
    assert np.array_equal(a.astype(np.uint8).reshape(H, W * 4).view(np.uint32), ref["rgba"])
    assert d["rays_per_frame"] == ref["stats"]["rays"]
