"""The trace launch plan (csrc/rt_plan.h) on the host: which trace kernel a frame gets, its lane
mapping and group geometry, its grid and its scheduling history mode are pure arithmetic, so
tests/plan_host.cpp prints them without a GPU (host pass of the kernels' compiler and float rules).

Kernel choice: golden/trace_variants.npz is the table `ns_bucket lds mode shm part_k sky sky_brute`
of plan_host.cpp's grid, recorded from the commit before trace_variant_key existed: that commit's
rt_kernels.hip compiled whole, linked to a throwaway program that ran choose_trace_variant over the
same grid and printed the kernel handle's address (named trace_kernel<NS, LDS, MODE> by nm -C),
shm and the flags.  The grid regenerates the inputs; the table holds outputs only.

Geometry, grid and history cases: derived from launch_trace's text at that commit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NG = 9  # MAX_FRAMES - 1
# the 47 trace kernels of the build, <NS, LDS, MODE>
KERNELS = (
    {(0, 1, m) for m in (0, 4, 16, 20, 52, 116, 180, 420, 692, 700)} | {(0, 0, 0)}
    | {(2, 1, m) for m in (0, 4, 16, 20, 24, 52, 56, 116, 180, 420)} | {(2, 0, 0)}
    | {(NG, 1, m) for m in (0, 1, 2, 3, 8, 9, 10, 11, 4, 16, 20, 24, 52, 56, 116, 180, 420)}
    | {(NG, 0, m) for m in (0, 1, 2, 3, 8, 9, 10, 11)})


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math",
                    "-fno-slp-vectorize", "-I", os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "plan_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)

    def run(*args):
        return subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
    return run


def fields(out):
    t = out.split()
    return {k: int(v) for k, v in zip(t[::2], t[1::2])}


def test_recorded_table_covers_the_kernels():
    t = np.load(os.path.join(GOLDEN, "trace_variants.npz"))["table"]
    assert len(KERNELS) == 47
    assert {tuple(int(v) for v in r[:3]) for r in t} == KERNELS           # every trace kernel, and no other
    assert {tuple(int(v) for v in r[4:]) for r in t} == {(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 1, 0)}   # part_k, sky, sky_brute


def test_trace_variant_key_matches_recorded_table(plan):
    want = np.load(os.path.join(GOLDEN, "trace_variants.npz"))["table"]
    got = np.array([[int(v) for v in line.split()] for line in plan("variants").splitlines()], dtype=np.int64)
    assert got.shape == want.shape
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "case %d: got %s, recorded %s" % (bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("row_step,spp,want", [
    (1, 8, dict(lanes_per_px=8, px_per_wave=8, gw=4, gh=2, n_gx=480, n_groups=259200, l_shift=3, gw_shift=2, n_rows=1080)),
    (8, 8, dict(lanes_per_px=8, px_per_wave=8, gw=8, gh=1, n_gx=240, n_groups=32400, n_rows=135)),
    (1, 1, dict(lanes_per_px=1, px_per_wave=64, gw=8, gh=8)),
    (1, 16, dict(lanes_per_px=16, px_per_wave=4, gw=2, gh=2)),
    (1, 32, dict(lanes_per_px=32, px_per_wave=2, gw=2, gh=1)),
    (1, 64, dict(lanes_per_px=64, px_per_wave=1, gw=1, gh=1)),
    (1, 200, dict(lanes_per_px=64, px_per_wave=1, gw=1, gh=1)),
    (1, 3, dict(lanes_per_px=3, px_per_wave=21, gw=21, gh=1, l_shift=-1, gw_shift=-1)),
])
def test_frame_geometry(plan, row_step, spp, want):
    g = fields(plan("geometry", 1920, 1080, 0, row_step, spp))
    assert {k: g[k] for k in want} == want
    # the ticket permutation: a factor coprime with the queue length; the divisors are the launch constants
    per_q = (g["n_groups"] + 7) // 8
    assert g["div_ngx_d"] == g["n_gx"] and g["div_perq_d"] == per_q
    assert np.gcd(g["scramble"], per_q) == 1 and 0 < g["scramble"] < per_q
    assert g["scramble_small"] == int((per_q + 3) * g["scramble"] < 2 ** 32)   # (+ RT_TPC tickets past the end)


def test_frame_geometry_no_rows(plan):
    assert fields(plan("geometry", 1920, 1080, 1080, 1, 8))["n_rows"] <= 0
    assert fields(plan("geometry", 1920, 1080, 1085, 8, 8))["n_rows"] <= 0


HALF, FULL, STREAM = 0, 1, 2   # RT_OVERLAP_* (rt_amd.h)


def test_overlap_constants():
    txt = open(os.path.join(ROOT, "include", "rt_amd.h")).read()
    for name, v in (("RT_OVERLAP_HALF", HALF), ("RT_OVERLAP_FULL", FULL), ("RT_OVERLAP_STREAM", STREAM)):
        assert "%s = %d" % (name, v) in txt


# n_cu = 256, per_cu = 1, blocks of 16 waves: (n_groups, n_slots, overlap, other_running, ranks_per_device) -> plan
@pytest.mark.parametrize("args,want", [
    ((259200, 1, HALF, 0, 1), dict(blocks=256, grid_waves=4096, heavy_static=1, heavy_cap=64800)),
    ((259200, 8, HALF, 1, 1), dict(blocks=128, grid_waves=2048, heavy_static=0, heavy_cap=64800)),
    ((32400, 8, HALF, 1, 1), dict(blocks=64)),       # 32400 < 48 * 2048: a quarter of the CUs
    ((32400, 8, HALF, 1, 8), dict(blocks=128)),      # not with virtual ranks
    ((259200, 8, FULL, 1, 1), dict(blocks=256, heavy_static=0)),
    ((259200, 3, HALF, 1, 1), dict(blocks=256, heavy_static=0)),
    ((259200, 8, HALF, 0, 1), dict(blocks=256, heavy_static=1)),
    ((259200, 4, STREAM, 0, 1), dict(blocks=128, heavy_static=0)),
    ((10, 1, HALF, 0, 1), dict(blocks=1, grid_waves=16, heavy_static=0, heavy_cap=32)),
])
def test_grid_policy(plan, args, want):
    n_groups, n_slots, overlap, other, ranks = args
    g = fields(plan("grid", 256, 1, n_groups, n_slots, overlap, other, ranks))
    assert {k: g[k] for k in want} == want


# (want_stats, dbg, sky, prof, heavy_q, n_groups, full_waves) -> hist
@pytest.mark.parametrize("args,want", [
    ((1, 0, 1, 0, 6, 100, 4096), 0), ((0, 1, 1, 0, 6, 100, 4096), 0), ((1, 0, 0, 1, 6, 100, 4096), 0),
    ((0, 0, 1, 0, 6, 259200, 4096), 2), ((0, 0, 1, 0, 6, 100, 4096), 2),
    ((0, 0, 1, 0, 0, 12 * 4096, 4096), 1), ((0, 0, 1, 0, 0, 12 * 4096 + 1, 4096), 0),
    ((0, 0, 0, 1, 6, 259200, 4096), 1), ((0, 0, 0, 0, 6, 259200, 4096), 0), ((0, 0, 0, 0, 6, 32400, 4096), 1),
])
def test_history_mode(plan, args, want):
    assert fields(plan("history", *args))["hist"] == want
