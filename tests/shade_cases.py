"""Shared pieces of the rt_shade tests (tests/test_shade_host.py, tests/test_gpu_shade.py): the
frames and cameras of the cases, the bit-for-bit comparison, rt_accum.h's fold restated in numpy
float32 (tests/test_accumulate_host.py proves the restatement against the header) and the six
axis orientations of the probe.  TEST INFRASTRUCTURE (may use the oracle)."""
import numpy as np

import query_cases as qc

SCENE = "world8_stress"
SIZES = ((96, 64), (50, 37))                 # whole waves; a ragged frame (1850 rays: 28 waves and 58 lanes)
MOVED_CAMERA = qc.VALUES_CAMERA              # above the near edge, 45 degrees down: 94% of the pixels hit
PLAN_N = (1, 63, 64, 65, 257, 2073600)       # one lane; a wave's edges; more than one block; a 1080p frame
BATCHES = (1, 63, 64, 65, 257)
ORDERED, HEAP, BRUTE = 0, 1, 2
NG = 9                                       # MAX_FRAMES - 1: the generic frame-stack depth
OUT = ("radiance", "rgba", "rays_out")
PERM_SEED = 20241021

# The probe: a camera inside world8_stress turned to +z, +x, -z, -x (about y), up and down (about x);
# quaternions (x, y, z, w), half angles of 0, 90, 180, 270 degrees and -+ 90 degrees.
R = 0.70710678
PROBE_SIZE = (32, 24)
PROBE_POS = (-0.45, 4.0, -3.9)               # in the pit at the field's near edge: walls on three sides, sky behind and above
PROBE_QUATS = ((0.0, 0.0, 0.0, 1.0), (0.0, R, 0.0, R), (0.0, 1.0, 0.0, 0.0), (0.0, -R, 0.0, R),
               (-R, 0.0, 0.0, R), (R, 0.0, 0.0, R))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def differing(got, want):
    """Rays whose value differs in any bit."""
    g, w = bits(got), bits(want)
    return int((g != w).reshape(len(w), -1).any(axis=1).sum())


def assert_same(got, want, keys=OUT, ctx=""):
    for k in keys:
        assert np.array_equal(bits(got[k]), bits(want[k])), (ctx, k, differing(got[k], want[k]))


def take(res, idx, keys=OUT):
    return {k: res[k][idx] for k in keys}


def frame_of(fr, keys=("radiance", "rgba")):
    """A frame of Scene.render as per-ray arrays in pixel order."""
    return {k: (fr[k].reshape(-1, 4) if k == "radiance" else fr[k].ravel()) for k in keys}


def pack(c):
    """rt_accum.h's pack of (n, 4) float32 colours in [0, 1]: Color's truncation to bytes, RGBA from the top."""
    b = (np.float32(255) * c.astype(np.float32)).astype(np.uint8).astype(np.uint32)
    return ((b[:, 0] << 24) + (b[:, 1] << 16) + (b[:, 2] << 8) + b[:, 3]).astype(np.uint32)


def fold(samples):
    """The frame of the samples (each (n_px, 4) float32 radiance) by rt_accum.h's arithmetic: in-order
    sums from 0, raw and clamped per sample, the mean as x * 2^-k for n = 2^k and x / n otherwise,
    then pack.  (radiance, rgba)."""
    n = len(samples)
    sum_r = np.zeros(samples[0].shape, np.float32)
    sum_c = np.zeros(samples[0].shape, np.float32)
    for r in samples:
        r = r.astype(np.float32)
        sum_r = sum_r + r
        sum_c = sum_c + np.where(r > np.float32(1), np.float32(1), r)
    assert sum_r.dtype == np.float32 and sum_c.dtype == np.float32
    if n & (n - 1) == 0:
        recip = np.float32(1) / np.float32(n)
        mc, mr = sum_c * recip, sum_r * recip
    else:
        mc, mr = sum_c / np.float32(n), sum_r / np.float32(n)
    return mr.astype(np.float32), pack(mc)


ZERO_RGBA = 0                                # pack of (0, 0, 0, 0)
