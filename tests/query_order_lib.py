"""Shared pieces of the query-order tests (tests/test_query_order_host.py, tests/test_gpu_query_order.py):
tests/query_order_host.cpp compiled with the flags tests/test_query_host.py uses, its keys for numpy
arrays, and the edge rays both tests feed it.  TEST INFRASTRUCTURE."""
import os
import shutil
import subprocess

import numpy as np

import query_cases as qc
from conftest import ROOT

REJECTED_BIT = np.uint64(1) << np.uint64(63)


class HostProgram:
    def __init__(self, tmp_dir):
        hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
        self.dir = str(tmp_dir)
        self.exe = os.path.join(self.dir, "query_order_host")
        subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math",
                        "-fno-slp-vectorize", "-I", os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "query_order_host.cpp"), "-o", self.exe],
                       check=True, capture_output=True, text=True)
        self.info = self._fields("info")

    def _fields(self, *args):
        t = subprocess.run([self.exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.split()
        return {k: int(v) for k, v in zip(t[::2], t[1::2])}

    def plan(self, n_rays, mode, counted):
        return self._fields("plan", n_rays, mode, int(counted))

    def keys(self, rays, box):
        """uint64 keys of (n, 6) rays as traced in `box` (6 floats, or one box per ray)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        rows = np.concatenate([rays, np.broadcast_to(np.asarray(box, np.float32).reshape(-1, 6), rays.shape)], axis=1)
        a, b = os.path.join(self.dir, "keys_in.bin"), os.path.join(self.dir, "keys_out.bin")
        np.ascontiguousarray(rows, np.float32).tofile(a)
        subprocess.run([self.exe, "keys", a, b], check=True)
        out = np.fromfile(b, np.uint64)
        assert len(out) == len(rays)
        return out


def as_traced(origins, dirs):
    """(n, 6) float32: the rays rt_query traces for caller origins / directions (rmath::Ray's normalisation)."""
    with np.errstate(all="ignore"):
        return np.concatenate([np.asarray(origins, np.float32).reshape(-1, 3), qc.normalized32(dirs)], axis=1).astype(np.float32)


# caller rays the kernel rejects: NaN / inf components, the zero direction, a 1e-6-long direction
REJECTED_RAYS = np.float32([
    [np.nan, 0, 0, 0, 0, 1], [0, np.inf, 0, 0, 0, 1], [0, 0, -np.inf, 0, 1, 0], [0, 0, 0, np.nan, 0, 1],
    [0, 0, 0, np.inf, 0, 0], [0, 0, 0, 0, -np.inf, 1], [1, 2, 3, 0, 0, 0], [1, 2, 3, 1e-6, 0, 0],
    [0, 0, 0, 6e-7, 6e-7, -6e-7], [0, 0, 0, 3e38, 3e38, 3e38]])
OCTANTS = np.float32([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
AXES = np.float32([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])


def edge_rays(box):
    """Caller rays (origins, dirs) at the key's edges for `box`: the rejected rays, the octant and axis
    directions from the box centre, and origins on, beyond and far beyond every face."""
    box = np.asarray(box, np.float32)
    mn, mx = box[0:3], box[3:6]
    c, e = 0.5 * (mn + mx), mx - mn
    o, d = [REJECTED_RAYS[:, 0:3]], [REJECTED_RAYS[:, 3:6]]
    dirs = np.concatenate([OCTANTS, AXES, np.float32([[0.3, -0.2, 0.9], [1e-30, 1, 0], [-0.0, 0.0, -2.5]])])
    o.append(np.tile(c, (len(dirs), 1))); d.append(dirs)
    for ax in range(3):
        for f in (-1e6, -1.0, -1e-3, 0.0, 1e-3, 0.25, 0.5, 0.999, 1.0, 1.001, 2.0, 1e6, 1e30):
            p = c.copy()
            p[ax] = mn[ax] + np.float32(f) * e[ax]
            o.append(p[None, :]); d.append(np.float32([[0.1, -0.7, 0.4]]))
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)


def scene_box(arrays):
    """A conservative world box of a scene from Scene.arrays(): every instance position +- the
    farthest vertex's distance from its mesh origin (a rotation keeps it inside)."""
    pos = arrays["instances"][:, 4:7].astype(np.float64)
    r = float(np.linalg.norm(arrays["vertices"].astype(np.float64), axis=1).max())
    return np.concatenate([pos.min(axis=0) - r, pos.max(axis=0) + r]).astype(np.float32)
