"""The axis-specialised leaf step of cast_local (rt_math.h: axis_plane_pass<AX>, axis_inplane_reject<AX>),
compiled for the host with the kernels' float rules (tests/leaf_loop_host.cpp): for all three axes
and a million random (ray, record) pairs each, the plane time's bits, the window test and the
in-plane reject equal the form they replaced (every component picked through a run-time axis
index), and the window's edge values behave as the reference's comparisons do (a NaN reciprocal
never passes, tt == lo passes, tt == t_best does not).  The GPU twin is tests/test_gpu_leaf_loop.py."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "leaf_loop_host.cpp")
INC = os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", INC]


def check(out, n):
    pairs, passes, rejects, nan_inv, mismatch, edge_err = (int(v) for v in out.split())
    assert pairs > 2.9 * n                     # (a few zero directions are dropped)
    assert mismatch == 0
    assert edge_err == 0
    # both outcomes of both tests occur, and so does the NaN reciprocal
    assert 0.2 * pairs < passes < 0.8 * pairs
    assert 0.2 * passes < rejects < 0.9 * passes
    assert 0.02 * pairs < nan_inv < 0.2 * pairs


def test_axis_step_host(tmp_path):
    exe = str(tmp_path / "leaf_loop_host")
    subprocess.run(["g++", "-O2", *FLAGS, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "1000000"], capture_output=True, text=True)
    check(r.stdout, 1000000)
    assert r.returncode == 0


def test_axis_step_host_sanitized(tmp_path):
    """The same program under AddressSanitizer and UBSan, stand-alone."""
    exe = str(tmp_path / "leaf_loop_host_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", *FLAGS, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "200000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    check(r.stdout, 200000)
