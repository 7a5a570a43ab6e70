"""The unit-length closed forms of the shading steps' chains (rt_math.h: reflect_unit,
reflect_pre_unit; rt_kernels.hip trace_sample: the hit's unit normal, the light step's three
chains, the reflection step), compiled for the host with the kernels' float rules
(tests/unitlen_shade_host.cpp): for a million random (unit normal, unit incoming direction, point
light) triples every chain's head passes its vote in at least 99% of them, every squared length
met after a passed head lies inside unit_window, and the closed forms return the generic chains'
bits; on adversarial inputs (window edges, zero and near-zero vectors, a directional light's
sqrt(2)) the vote fails exactly where the head is outside unit_head, and the result is the
generic one.  The GPU twin is tests/test_gpu_shade_chains.py."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "unitlen_shade_host.cpp")
INC = os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", INC]


def check(out, n):
    triples, head_pass, outside, mismatch, adversarial, vote_err = (int(v) for v in out.split())
    print("triples %d head_pass %d outside %d mismatch %d adversarial %d vote_err %d"
          % (triples, head_pass, outside, mismatch, adversarial, vote_err))
    assert triples > 0.99 * n
    assert outside == 0                       # a stage outside the window after a passed head: a finding
    assert mismatch == 0                      # closed form != generic chain: a finding
    assert vote_err == 0                      # adversarial inputs: the vote fails where it must
    assert adversarial > 12000
    assert head_pass >= 0.99 * triples        # the fast path is the common path


def test_shade_chains_host(tmp_path):
    exe = str(tmp_path / "unitlen_shade_host")
    subprocess.run(["g++", "-O2", *FLAGS, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "1000000"], capture_output=True, text=True)
    check(r.stdout, 1000000)
    assert r.returncode == 0


def test_shade_chains_host_sanitized(tmp_path):
    """The same program under AddressSanitizer and UBSan, stand-alone."""
    exe = str(tmp_path / "unitlen_shade_host_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", *FLAGS, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, "200000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    check(r.stdout, 200000)
