"""Progressive refinement on the host.

The per-pixel arithmetic rt_accumulate's fold kernel and the trace kernel's resolve share
(csrc/rt_accum.h: fold, mean, pack), compiled for the host with the kernels' float rules
(tests/accum_host.cpp), against a numpy float32 restatement: in-order sums from 0, clamp per
sample, the mean as x * 2^-k for n = 2^k and x / n otherwise, Color's truncation.  Every RGBA word
and every float is equal bit for bit, for n = 1..9, 16, 17 and 64 (both forms of the mean), over
random samples with values above 1, exact 0, -0.0 and values in the denormal range.

And rt_accumulate's argument checks, which come before any device work, on a machine without a
device.  The GPU twin is tests/test_gpu_accumulate.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, scene_path

SRC = os.path.join(ROOT, "tests", "accum_host.cpp")
INC = os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I", INC]
NS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 64)
N_MAX = 64


def samples(n_px, seed=7):
    """(N_MAX, n_px, 4) float32, non-negative (a negative channel's byte is outside what the
    reference's Color defines): mostly in [0, 1.6), with exact 0, -0.0, values around 1, large
    values and values in and just above the denormal range mixed in per element."""
    rng = np.random.default_rng(seed)
    s = (rng.random((N_MAX, n_px, 4), np.float32) * np.float32(1.6)).astype(np.float32)
    pick = rng.integers(0, 16, s.shape)
    s[pick == 0] = 0.0
    s[pick == 1] = -0.0
    s[pick == 2] = rng.choice(np.array([1e-45, 3e-42, 1e-39, 1.1754942e-38, 1.1754944e-38, 2e-38], np.float32), int((pick == 2).sum()))
    s[pick == 3] = rng.choice(np.array([1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0)),
                                        37.5, 1e6], np.float32), int((pick == 3).sum()))
    # whole pixels of special values: all zero, all -0.0, all denormal, all above 1, exactly 1
    s[:, 0] = 0.0
    s[:, 1] = -0.0
    s[:, 2] = np.float32(3e-42)
    s[:, 3] = np.float32(1.25)
    s[:, 4] = np.float32(1.0)
    return s


def numpy_frames(s):
    """{n: (sum_r, sum_c, rgba, radiance)}: the frame of the first n samples, in float32."""
    out = {}
    sum_r = np.zeros(s.shape[1:], np.float32)
    sum_c = np.zeros(s.shape[1:], np.float32)
    for k in range(s.shape[0]):
        r = s[k]
        sum_r = sum_r + r                                          # float32 + float32: one rounding
        sum_c = sum_c + np.where(r > np.float32(1), np.float32(1), r)
        assert sum_r.dtype == np.float32 and sum_c.dtype == np.float32
        n = k + 1
        if n in NS:
            if n & (n - 1) == 0:
                recip = np.float32(1) / np.float32(n)
                mc, mr = sum_c * recip, sum_r * recip
            else:
                mc, mr = sum_c / np.float32(n), sum_r / np.float32(n)
            b = (np.float32(255) * mc).astype(np.uint8).astype(np.uint32)   # truncation; values are in [0, 255]
            rgba = (b[:, 0] << 24) + (b[:, 1] << 16) + (b[:, 2] << 8) + b[:, 3]
            out[n] = (sum_r.copy(), sum_c.copy(), rgba.astype(np.uint32), mr.astype(np.float32))
    return out


def run_and_check(exe, tmp_path, n_px):
    s = samples(n_px)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    s.tofile(fin)
    r = subprocess.run([exe, fin, fout, str(n_px), str(N_MAX)] + [str(n) for n in NS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout) == len(NS)
    raw = np.fromfile(fout, np.uint32)
    rec = 13 * n_px                                                # words per record: 4 + 4 + 1 + 4 per pixel
    assert raw.size == rec * len(NS)
    want = numpy_frames(s)
    for i, n in enumerate(NS):
        w = raw[i * rec:(i + 1) * rec]
        got = (w[:4 * n_px], w[4 * n_px:8 * n_px], w[8 * n_px:9 * n_px], w[9 * n_px:])
        for name, g, e in zip(("sum_r", "sum_c", "rgba", "radiance"), got, want[n]):
            e = np.ascontiguousarray(e).view(np.uint32).ravel()
            assert np.array_equal(g, e), (n, name, int((g != e).sum()))
    # the special pixels say what they should: -0.0 sums to +0.0, a pixel of 1.25 is white
    assert want[3][0][1].view(np.uint32).max() == 0 and want[3][2][3] == 0xFFFFFFFF and want[3][2][4] == 0xFFFFFFFF
    assert want[3][2][0] == 0 and want[3][2][2] == 0
    assert np.all(want[5][3][3] == np.float32(1.25))


def test_fold_and_resolve_match_numpy(tmp_path):
    exe = str(tmp_path / "accum_host")
    subprocess.run(["g++", "-O2", *FLAGS, SRC, "-o", exe], check=True, capture_output=True, text=True)
    run_and_check(exe, tmp_path, 1531)


def test_fold_and_resolve_sanitized(tmp_path):
    """The same program under AddressSanitizer and UBSan, stand-alone."""
    exe = str(tmp_path / "accum_host_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", *FLAGS, SRC, "-o", exe], check=True, capture_output=True, text=True)
    run_and_check(exe, tmp_path, 257)


def test_opts_default(rt):
    o = rt.AccumOpts()
    ctypes.memset(ctypes.byref(o), 0xff, ctypes.sizeof(o))
    rt.lib().rt_accum_opts_default(ctypes.byref(o))
    assert (o.samples, o.use_bvh, o.rebuild_bvh, o.textures, o.restart, o.host_outputs) == (1, 1, 1, 0, 0, 0)
    assert (o.rgba, o.radiance, o.hit_inst, o.hit_tri) == (None, None, None, None)
    rt.lib().rt_accum_opts_default(None)                           # a null pointer is ignored


def test_argument_checks_come_first(rt):
    """Null options, samples < 1, no output and the sample limit are reported with or without a
    device; RT_ERR_NODEV only after them.  Info and reset are host state."""
    L = rt.lib()
    s = rt.Scene.load_json(scene_path("world1"), 16, 12)
    n = ctypes.c_int(-7)
    buf = np.zeros((12, 16), np.uint32)

    def opts(**kw):
        o = rt.AccumOpts()
        L.rt_accum_opts_default(ctypes.byref(o))
        o.host_outputs, o.rgba = 1, buf.ctypes.data
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    assert L.rt_accumulate(s._h, None, ctypes.byref(n)) == rt.RT_ERR_ARG
    assert L.rt_accumulate(None, ctypes.byref(opts()), ctypes.byref(n)) == rt.RT_ERR_ARG
    for bad in (0, -1):
        assert L.rt_accumulate(s._h, ctypes.byref(opts(samples=bad)), ctypes.byref(n)) == rt.RT_ERR_ARG
    assert L.rt_accumulate(s._h, ctypes.byref(opts(rgba=None)), ctypes.byref(n)) == rt.RT_ERR_ARG
    assert b"no output" in L.rt_last_error()
    # the limit is on the count the call would reach: 65536 samples are admitted, one more is not
    assert L.rt_accumulate(s._h, ctypes.byref(opts(samples=65537)), ctypes.byref(n)) == rt.RT_ERR_LIMIT
    assert L.rt_accumulate(s._h, ctypes.byref(opts(samples=65537, restart=1)), ctypes.byref(n)) == rt.RT_ERR_LIMIT
    assert n.value == -7                                           # a failed call does not write the count
    assert s.accumulated == (0, 16, 12, 0)
    assert L.rt_accumulate_reset(s._h) == rt.RT_OK and L.rt_accumulate_reset(None) == rt.RT_ERR_ARG
    assert L.rt_accumulate_info(s._h, None) == rt.RT_ERR_ARG
    assert s.accumulated == (0, 16, 12, 0)                         # a reset of nothing is no restart
    if rt.device_count() == 0:                                     # (with a device: tests/test_gpu_accumulate.py)
        assert L.rt_accumulate(s._h, ctypes.byref(opts()), ctypes.byref(n)) == rt.RT_ERR_NODEV
        with pytest.raises(rt.RtError) as e:
            s.accumulate()
        assert e.value.code == rt.RT_ERR_NODEV
        assert s.accumulated == (0, 16, 12, 0)
