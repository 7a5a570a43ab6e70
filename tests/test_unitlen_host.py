"""The unit-length fast path of the direction and normal chains (rt_math.h: unit_window, unit_head,
unit_len_rcp and the two chain stages built on them), compiled for the host with the kernels'
float rules (tests/unitlen_host.cpp): the closed forms equal sqrtf and 1.0f / sqrtf bit for bit
on every float of the window, the window tests are false for everything else, and for a million
random directions the chain's head passes its vote, every later stage stays inside the window
and the unit chain returns the generic chain's bits (the fast path is the common path).  The GPU
twin is tests/test_gpu_unitlen.py."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "unitlen_host.cpp")
INC = os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", INC]


def check(out):
    swept, in_window, window_err, value_err, special_err, dirs, outside, mismatch = (int(v) for v in out.split())
    assert swept == 2048 + 1024 + 1           # 2^-24 apart below 1, 2^-23 apart above, and 1 itself
    assert in_window == 1024 + 512 + 1        # |s - 1| <= 2^-14
    assert window_err == 0
    assert value_err == 0
    assert special_err == 0
    assert outside == 0                       # 100%: a failure here is a finding about the windows
    assert mismatch == 0
    return dirs


def test_unit_len_rcp_host(tmp_path):
    exe = str(tmp_path / "unitlen_host")
    subprocess.run(["g++", "-O2", *FLAGS, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "1000000"], capture_output=True, text=True)
    assert check(r.stdout) > 990_000
    assert r.returncode == 0


def test_unit_len_rcp_host_sanitized(tmp_path):
    """The same program under AddressSanitizer and UBSan, stand-alone."""
    exe = str(tmp_path / "unitlen_host_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", *FLAGS, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "200000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert check(r.stdout) > 198_000
