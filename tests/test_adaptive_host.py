"""Adaptive refinement on the host.

csrc/rt_adapt.h's tile mapping and edge predicate -- the definitions accum_edge_kernel compiles --
built for the host with the kernels' float rules (tests/adaptive_host.cpp) against the numpy
restatement (adaptive_cases.need_mask), byte for byte, on the oracle's 1-spp frames of the cases,
on a frame with a NaN and a -0 planted, and on canvases of 1 x 1, 7 x 9 and 8 x 8.  The recorded
needed-tile counts, and how far the oracle's nearest contrast lies from the 8/255 threshold (the
device test's mask equality then cannot sit on a tie).  And rt_accumulate_set_adaptive /
rt_accumulate_adaptive_info's argument checks, which need no device.  The GPU twin is
tests/test_gpu_adaptive.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import adaptive_cases as ac
from conftest import ROOT, scene_path
from twin import orc_render

SRC = os.path.join(ROOT, "tests", "adaptive_host.cpp")
INC = os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-I", INC]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("adaptive") / "adaptive_host")
    subprocess.run(["g++", "-O2", *FLAGS, SRC, "-o", path], check=True, capture_output=True, text=True)
    return path


@pytest.fixture(scope="module")
def frames(oracle):
    """case -> the oracle's 1-spp raw radiance (H, W, 4), rendered once and never written to."""
    out = {}
    for case in ac.CASES:
        _, o, bvh = ac.make(None, oracle, case)
        r = orc_render(oracle, o, spp=1, use_bvh=int(bvh), want=("radiance",))["radiance"]
        r.setflags(write=False)
        out[case] = r
    return out


def host_mask(exe, tmp_path, radiance, threshold, tile=ac.TILE):
    h, w = radiance.shape[:2]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(radiance, np.float32).tofile(fin)
    bits = int(np.float32(threshold).view(np.uint32))
    r = subprocess.run([exe, fin, fout, str(w), str(h), str(tile[0]), str(tile[1]), str(bits)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n_tx, n_ty, needed = (int(x) for x in r.stdout.split())
    m = np.fromfile(fout, np.uint8).reshape(n_ty, n_tx)
    assert int(m.sum()) == needed and set(np.unique(m)) <= {0, 1}
    return m.astype(bool)


@pytest.mark.parametrize("case", list(ac.CASES))
def test_predicate_matches_numpy_on_the_cases(exe, frames, tmp_path, case):
    r = frames[case]
    for thr in (ac.THRESHOLD, 0.0, 0.125):
        want = ac.need_mask(r, thr)
        got = host_mask(exe, tmp_path, r, thr)
        assert got.shape == want.shape and np.array_equal(got, want), (case, thr, int((got != want).sum()))
    n = int(ac.need_mask(r, ac.THRESHOLD).sum())
    assert n == ac.NEEDED[case], (case, n)
    total = ac.n_tiles(r.shape[1], r.shape[0])
    if case == "sky":
        assert n == 0 and not r.any()                              # the oracle's frame is all zeros
    else:
        assert 0 < n < total, (case, n, total)


def test_nan_and_negative_zero(exe, frames, tmp_path):
    """A NaN channel flags nothing by itself (its differences compare false) and a -0 is a 0."""
    base = np.zeros((24, 24, 4), np.float32)
    r = base.copy()
    r[12, 12, 1] = np.nan                                          # inside tile (1, 1), away from its borders
    r[3, 20] = -0.0
    assert not ac.need_mask(r, 0.0).any()
    assert not host_mask(exe, tmp_path, r, 0.0).any()
    r[12, 13, 2] = 0.5                                             # a real contrast beside the NaN: that tile alone
    want = ac.need_mask(r, ac.THRESHOLD)
    assert want.sum() == 1 and want[1, 1]
    assert np.array_equal(host_mask(exe, tmp_path, r, ac.THRESHOLD), want)
    # the same planted into a real frame
    s = frames["stress"].copy()
    s[10, 10, 0] = np.nan
    s[40, 40] = -0.0
    assert np.array_equal(host_mask(exe, tmp_path, s, ac.THRESHOLD), ac.need_mask(s, ac.THRESHOLD))


@pytest.mark.parametrize("size", [(1, 1), (7, 9), (8, 8), (9, 8), (17, 3)])
def test_small_canvases(exe, tmp_path, size):
    """Partial tiles, a single pixel (no neighbour: never an edge), contrasts across tile borders
    (both tiles flagged), diagonals included (the 8-neighbourhood)."""
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    for k in range(4):
        r = np.zeros((h, w, 4), np.float32)
        if k == 1:
            r[...] = rng.random((h, w, 4), np.float32) * np.float32(1.5)
        elif k >= 2:                                               # one bright pixel (values above 1 clamp to 1)
            r[rng.integers(0, h), rng.integers(0, w)] = (0.2, 3.0, 0.0, 1.0)
        for thr in (0.0, ac.THRESHOLD, 0.9):
            want = ac.need_mask(r, thr)
            assert np.array_equal(host_mask(exe, tmp_path, r, thr), want), (size, k, thr)
    if size == (1, 1):
        one = np.full((1, 1, 4), 0.7, np.float32)
        assert not host_mask(exe, tmp_path, one, 0.0).any()


def test_border_and_diagonal_contrasts(exe, tmp_path):
    """A bright pixel in a tile's corner flags the three tiles it touches as well: across an
    edge and across the corner (the diagonal neighbour)."""
    r = np.zeros((16, 16, 4), np.float32)
    r[7, 7] = 1.0                                                  # the last pixel of tile (0, 0)
    want = ac.need_mask(r, ac.THRESHOLD)
    assert want.all()                                              # (0, 0), (0, 1), (1, 0) and, diagonally, (1, 1)
    assert np.array_equal(host_mask(exe, tmp_path, r, ac.THRESHOLD), want)
    # two values above 1 are clamped to the same 1: no contrast, even at threshold 0
    r = np.full((8, 16, 4), 5.0, np.float32)
    r[:, 8:] = 2.0
    assert not host_mask(exe, tmp_path, r, 0.0).any() and not ac.need_mask(r, 0.0).any()


@pytest.mark.parametrize("case", ac.MARGIN_CASES)
def test_threshold_margin(frames, case):
    """At 8/255 the oracle's nearest neighbour contrast is at least 1e-3 relative away from the
    threshold (measured: 0.29, 0.35, 0.11), against the 1e-5 the product's radiance may differ by."""
    c = ac.neighbour_contrast(frames[case]).astype(np.float64)
    rel = np.abs(c - float(ac.THRESHOLD)) / float(ac.THRESHOLD)
    print("nearest contrast to the threshold, relative: %s %.4f" % (case, rel.min()))
    assert rel.min() >= 1e-3, (case, float(rel.min()))


def test_sanitized(tmp_path, frames):
    """The same program under AddressSanitizer and UBSan, stand-alone, on the odd-sized case."""
    exe = str(tmp_path / "adaptive_host_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                    "-fno-sanitize-recover=all", *FLAGS, SRC, "-o", exe], check=True, capture_output=True, text=True)
    r = frames["stress_odd"]
    assert np.array_equal(host_mask(exe, tmp_path, r, ac.THRESHOLD), ac.need_mask(r, ac.THRESHOLD))


def test_argument_checks_without_a_device(rt):
    L = rt.lib()
    s = rt.Scene.load_json(scene_path("world1"), 20, 12)
    assert rt.RT_ADAPTIVE_THRESHOLD_DEFAULT == 8.0 / 255.0
    t = s.accumulate_tiles()
    assert t == {"mode": 0, "threshold": pytest.approx(8.0 / 255.0), "tile": (8, 8), "need": None, "needed": -1, "traced": 0}
    for mode in (-1, 2, 7):
        assert L.rt_accumulate_set_adaptive(s._h, mode, 0.1) == rt.RT_ERR_ARG
    for thr in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert L.rt_accumulate_set_adaptive(s._h, 1, thr) == rt.RT_ERR_ARG
    assert L.rt_accumulate_set_adaptive(None, 1, 0.1) == rt.RT_ERR_ARG
    assert L.rt_accumulate_set_adaptive(s._h, 0, float("nan")) == rt.RT_OK     # ignored with mode 0
    assert s.accumulate_tiles()["mode"] == 0
    # changing the mode with nothing held counts no restart
    s.set_accumulate_adaptive(True, 0.25)
    t = s.accumulate_tiles()
    assert (t["mode"], t["threshold"], t["needed"], t["need"]) == (1, 0.25, -1, None)
    s.set_accumulate_adaptive(True, 0.0)
    s.set_accumulate_adaptive(False)
    s.set_accumulate_adaptive()
    assert s.accumulate_tiles()["threshold"] == pytest.approx(8.0 / 255.0)
    assert s.accumulated == (0, 20, 12, 0)
    # info: null output, the mask before it exists, a buffer too small
    o8 = np.zeros(8, np.int32)
    need = np.zeros(6, np.uint8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.rt_accumulate_adaptive_info(s._h, None, None, None, 0) == rt.RT_ERR_ARG
    assert L.rt_accumulate_adaptive_info(None, vp(o8), None, None, 0) == rt.RT_ERR_ARG
    assert L.rt_accumulate_adaptive_info(s._h, vp(o8), None, vp(need), 6) == rt.RT_ERR_STATE
    assert L.rt_accumulate_adaptive_info(s._h, vp(o8), None, vp(need), 5) == rt.RT_ERR_ARG
    assert L.rt_accumulate_adaptive_info(s._h, vp(o8), None, None, 0) == rt.RT_OK
    assert list(o8) == [1, 8, 8, 3, 2, -1, 0, 0]
    # the history hook is host state: no history before a frame
    assert L.rt_scene_history_info(s._h, None) == rt.RT_ERR_ARG and L.rt_scene_history_info(None, vp(o8)) == rt.RT_ERR_ARG
    h = s._history_info()
    assert len(h) == 12 and h[3] == 0
    if rt.device_count() == 0:
        assert h[:3] == (0, -1, 0) and h[4:] == (-1,) * 8
    # the pass buffer's hooks before the first rt_accumulate
    assert L.rt_accumulate_pass_fill(s._h, 1) == rt.RT_ERR_STATE
    buf = np.zeros(20 * 12 * 4, np.float32)
    assert L.rt_accumulate_pass_read(s._h, vp(buf), buf.size) == rt.RT_ERR_STATE
    assert L.rt_accumulate_pass_read(s._h, None, 0) == rt.RT_ERR_ARG
