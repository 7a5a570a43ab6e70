"""rt_occlusion's history across camera moves on the host.

- rt_occlusion_set_history / rt_occlusion_history_info / rt_occlusion_history_weights on a scene
  without a device: every RT_ERR_ARG case, the defaults read back, nothing dropped or counted while
  no samples are held, RT_ERR_STATE from the weights before an accumulation.
- The reprojection, the seed and the resolves with per-pixel totals that the kernels compile
  (csrc/rt_occl.h, through tests/occl_history_host.cpp with the kernels' float rules) against the
  numpy float32 restatement of tests/occl_history_lib.py, bit for bit, on synthetic records: the
  identity camera and a turned one on canvases of 1 x 1, 3 x 2 and 50 x 37 (every pixel maps onto
  itself), points behind the camera, off each canvas edge, cx + 0.5 at an integer and one float
  below and above it, NaN and infinite positions; T just below, at and above max_history, c = 0
  and c = T.
The GPU twin is tests/test_gpu_occlusion_history.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import occl_history_lib as hl
import occl_lib as ol
from conftest import ROOT, scene_path

F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    path = str(tmp_path_factory.mktemp("occl_history") / "occl_history_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math",
                    "-fno-slp-vectorize", "-I", os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "occl_history_host.cpp"), "-o", path],
                   check=True, capture_output=True, text=True)
    return path


# ---- the entries' argument checks and state --------------------------------------------------------------
def test_argument_checks_and_state(rt):
    L = rt.lib()
    s = rt.Scene.load_json(scene_path("world1"), 16, 12)
    defaults = {"on": False, "max_history": 32, "moves": 0, "cursor": 0, "n": 0, "weighted": False,
                "normal_min": float(F(0.9)), "plane_tol": float(F(1e-2))}
    assert s.occlusion_history == defaults
    assert rt.RT_AO_HISTORY_DEFAULT == hl.HISTORY_DEFAULT == 32
    for name in ("rt_occlusion_set_history", "rt_occlusion_history_info", "rt_occlusion_history_weights"):
        assert name in rt.SYMBOLS
    for on in (-1, 2):
        assert L.rt_occlusion_set_history(s._h, on, 32, 0.9, 1e-2) == rt.RT_ERR_ARG, on
    for on in (0, 1):                                              # everything is validated with on = 0 too
        for mh in (0, -1, 1025, 1 << 30):
            assert L.rt_occlusion_set_history(s._h, on, mh, 0.9, 1e-2) == rt.RT_ERR_ARG, (on, mh)
        for nm in (float("nan"), -1.0000001, 1.0000001, float("inf"), float("-inf")):
            assert L.rt_occlusion_set_history(s._h, on, 32, nm, 1e-2) == rt.RT_ERR_ARG, (on, nm)
        for pt in (-1e-9, float("nan"), float("inf"), float("-inf")):
            assert L.rt_occlusion_set_history(s._h, on, 32, 0.9, pt) == rt.RT_ERR_ARG, (on, pt)
    assert L.rt_occlusion_set_history(None, 1, 32, 0.9, 1e-2) == rt.RT_ERR_ARG
    assert s.occlusion_history == defaults                         # a refused call changes nothing
    s.set_occlusion_history(True, max_history=1, normal_min=-1.0, plane_tol=0.0)      # the ends of the ranges
    s.set_occlusion_history(True, max_history=1024, normal_min=1.0, plane_tol=1e30)
    h = s.occlusion_history
    assert h["on"] and h["max_history"] == 1024 and h["normal_min"] == 1.0 and h["plane_tol"] == float(F(1e30))
    s.set_occlusion_history(False, max_history=7, normal_min=0.5, plane_tol=0.25)
    h = s.occlusion_history
    assert not h["on"] and h["max_history"] == 7 and h["normal_min"] == 0.5 and h["plane_tol"] == 0.25
    s.set_occlusion_history()
    assert s.occlusion_history == dict(defaults, on=True)
    s.set_occlusion_history()                                      # nothing changes
    assert s.occlusion_info == (0, 16, 12, 0)                      # no samples were held: nothing dropped or counted
    # rt_occlusion_history_info: either destination may be null
    a, f = np.full(8, -9, np.int32), np.full(2, -9, np.float32)
    assert L.rt_occlusion_history_info(s._h, a.ctypes.data, None) == rt.RT_OK and tuple(a) == (1, 32, 0, 0, 0, 0, 0, 0)
    assert L.rt_occlusion_history_info(s._h, None, f.ctypes.data) == rt.RT_OK and (f[0], f[1]) == (F(0.9), F(1e-2))
    assert L.rt_occlusion_history_info(s._h, None, None) == rt.RT_OK
    assert L.rt_occlusion_history_info(None, a.ctypes.data, f.ctypes.data) == rt.RT_ERR_ARG
    # the weights: no accumulation yet; a destination that is too small
    w = np.zeros((12, 16), np.int32)
    assert L.rt_occlusion_history_weights(s._h, w.ctypes.data, w.size) == rt.RT_ERR_STATE
    assert L.rt_occlusion_history_weights(s._h, w.ctypes.data, w.size - 1) == rt.RT_ERR_ARG
    assert L.rt_occlusion_history_weights(s._h, None, w.size) == rt.RT_ERR_ARG
    assert L.rt_occlusion_history_weights(None, w.ctypes.data, w.size) == rt.RT_ERR_ARG
    with pytest.raises(rt.RtError) as e:
        s._occlusion_history_weights()
    assert e.value.code == rt.RT_ERR_STATE
    # the pattern's limit still comes with the arguments
    s.set_occlusion_pattern("interleaved")
    with pytest.raises(rt.RtError) as e:
        s.occlusion(samples=65)
    assert e.value.code == rt.RT_ERR_LIMIT
    assert s.occlusion_info == (0, 16, 12, 0) and s.occlusion_history["moves"] == 0


# ---- the reprojection -------------------------------------------------------------------------------------
def up(v):
    return np.nextafter(F(v), F(np.inf))


def down(v):
    return np.nextafter(F(v), F(-np.inf))


def make_camera(W, H, turned, near=1.0, unit=1.0):
    if turned:                                                     # an orthonormal frame, rounded to float32
        q = np.linalg.qr(np.array([[0.8, 0.1, -0.6], [0.2, 0.9, 0.3], [0.5, -0.4, 0.7]]))[0]
        r, u, f = q[:, 0], q[:, 1], np.cross(q[:, 0], q[:, 1])
        pos = (0.3, -1.2, 2.5)
    else:
        r, u, f, pos = (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)
    return {"pos": ol.f32(pos), "r": ol.f32(r), "u": ol.f32(u), "f": ol.f32(f), "near": F(near), "unit": F(unit),
            "W": F(W), "H": F(H)}


def pixel_points(cam, W, H, depth):
    """The point at `depth` along sample 0's ray of every pixel, in float64 then rounded once."""
    y, x = np.mgrid[0:H, 0:W]
    gx, gy = (x - 0.5 * W) / float(cam["unit"]), (0.5 * H - y) / float(cam["unit"])
    d = float(cam["near"]) * cam["f"].astype(np.float64) + gx[..., None] * cam["r"].astype(np.float64) + gy[..., None] * cam["u"].astype(np.float64)
    return (cam["pos"].astype(np.float64) + depth * d).astype(np.float32)


def run_reproject(exe, tmp_path, cam, pts):
    pts = ol.f32(pts).reshape(-1, 3)
    head = np.concatenate([cam["pos"], cam["r"], cam["u"], cam["f"], [cam["near"], cam["unit"], cam["W"], cam["H"]]]).astype(np.float32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([head, pts.ravel()]).astype(np.float32).tofile(fin)
    r = subprocess.run([exe, "reproject", fin, fout, str(len(pts))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.fromfile(fout, np.int32).reshape(-1, 3)
    return out[:, 0] != 0, out[:, 1], out[:, 2]


def both(exe, tmp_path, cam, pts):
    """The host program's verdicts, checked against the restatement's."""
    pts = ol.f32(pts).reshape(-1, 3)
    ok, qx, qy = run_reproject(exe, tmp_path, cam, pts)
    front, on, rx, ry, cx, cy = hl.reproject(pts, cam)
    assert np.array_equal(ok, on)
    assert np.array_equal(qx[ok], rx[on]) and np.array_equal(qy[ok], ry[on])
    assert (qx[~ok] == -1).all() and (qy[~ok] == -1).all()
    return ok, qx, qy, front, cx, cy


@pytest.mark.parametrize("turned", (False, True))
@pytest.mark.parametrize("size", [(1, 1), (3, 2), (50, 37)])
def test_every_pixel_maps_onto_itself(exe, tmp_path, size, turned):
    W, H = size
    cam = make_camera(W, H, turned, near=1.25, unit=20.0)
    y, x = np.mgrid[0:H, 0:W]
    for depth in (0.5, 3.0, 40.0):
        ok, qx, qy, front, cx, cy = both(exe, tmp_path, cam, pixel_points(cam, W, H, depth))
        assert ok.all() and np.array_equal(qx, x.ravel()) and np.array_equal(qy, y.ravel())
        assert np.abs(cx - x.ravel()).max() <= 1e-4 and np.abs(cy - y.ravel()).max() <= 1e-4
    # behind the camera (a < 0), and at the camera itself (a = 0)
    ok, _, _, front, _, _ = both(exe, tmp_path, cam, pixel_points(cam, W, H, -2.0))
    assert not ok.any() and not front.any()
    ok, _, _, front, _, _ = both(exe, tmp_path, cam, cam["pos"][None, :])
    assert not ok.any() and not front.any()


def test_canvas_edges_and_rounding(exe, tmp_path):
    """The identity camera with near = unit = 1 at depth a = 1: cx = sx + W / 2 and cy = H / 2 - sy."""
    W, H = 50, 37
    cam = make_camera(W, H, False)
    pts, want = [], []                                             # want: (axis, the pixels the point may fall on)
    for k in (0, 1, 17, 49, 50):                                   # cx + 0.5 = k exactly, one float below, one above
        sx = F(k - 0.5 - 0.5 * W)
        for v, q in ((sx, (k,)), (down(sx), (k - 1, k)), (up(sx), (k - 1, k))):
            pts.append((v, F(0), F(1)))
            want.append((0, q))
    for k in (0, 1, 20, 36, 37):                                   # the same for cy; cy falls as sy grows
        sy = F(0.5 * H - (k - 0.5))
        for v, q in ((sy, (k,)), (up(sy), (k - 1, k)), (down(sy), (k - 1, k))):
            pts.append((F(0), v, F(1)))
            want.append((1, q))
    ok, qx, qy, front, cx, cy = both(exe, tmp_path, cam, pts)
    assert front.all()
    for i, (axis, q) in enumerate(want):
        size, got, other = ((W, qx[i], qy[i]), (H, qy[i], qx[i]))[axis]
        if ok[i]:                                                  # the other coordinate is the canvas centre's: 25, 19
            assert got in q and 0 <= got < size and other == (19, 25)[axis], (i, axis, q, int(got))
        else:
            assert any(not 0 <= v < size for v in q), (i, axis, q)
        if len(q) == 1:                                            # the exact case is decided: floor(k) = k
            assert bool(ok[i]) == (0 <= q[0] < size), (i, axis, q)
    # off each edge by a pixel and by far; the corners just inside
    off = [(-26.0, 0, 1), (25.5, 0, 1), (0, 19.5, 1), (0, -19.0, 1), (-1e6, 0, 1), (1e6, 0, 1), (0, 1e30, 1), (0, -1e30, 1),
           (3e38, 3e38, 1e-30)]
    ok = both(exe, tmp_path, cam, off)[0]
    assert not ok.any()
    inside = [(-25.0, 18.5, 1), (24.0, 18.5, 1), (-25.0, -17.5, 1), (24.0, -17.5, 1)]
    ok, qx, qy = both(exe, tmp_path, cam, inside)[:3]
    assert ok.all() and list(zip(qx, qy)) == [(0, 0), (49, 0), (0, 36), (49, 36)]
    # NaN and infinite positions reject (the comparisons are in float, before any conversion)
    bad = [(np.nan, 0, 1), (0, np.nan, 1), (0, 0, np.nan), (np.inf, 0, 1), (-np.inf, 0, 1), (0, np.inf, 1), (0, 0, np.inf),
           (np.inf, np.inf, np.inf), (0, 0, -np.inf)]
    ok = both(exe, tmp_path, cam, bad)[0]
    assert not ok.any()


def test_random_points_agree(exe, tmp_path):
    rng = np.random.default_rng(5)
    for turned in (False, True):
        cam = make_camera(50, 37, turned, near=0.8, unit=30.0)
        pts = rng.normal(0, 3.0, (4000, 3)).astype(np.float32) + cam["pos"]
        ok, _, _, front, _, _ = both(exe, tmp_path, cam, pts)
        assert 0 < ok.sum() < len(pts) and 0 < front.sum() < len(pts)


# ---- the seed and the resolves ----------------------------------------------------------------------------
def run_pairs(exe, tmp_path, mode, pairs, dtype, extra=()):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(pairs, np.int32).tofile(fin)
    r = subprocess.run([exe, mode, fin, fout, str(len(pairs))] + [str(e) for e in extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.fromfile(fout, dtype).reshape(-1, 2)


@pytest.mark.parametrize("max_history", (1, 3, 32, 1024))
def test_seed_matches_numpy(exe, tmp_path, max_history):
    rng = np.random.default_rng(max_history)
    T = np.concatenate([np.arange(0, 2049), [max_history - 1, max_history, max_history + 1]]).clip(0, 2048)
    pairs = np.concatenate([np.stack([np.zeros_like(T), T], 1), np.stack([T, T], 1), np.stack([rng.integers(0, T + 1), T], 1),
                            np.stack([T // 2, T], 1)])
    got = run_pairs(exe, tmp_path, "seed", pairs, np.int32, (max_history,))
    c_h, n_h = hl.seed(pairs[:, 0], pairs[:, 1], max_history)
    assert np.array_equal(got[:, 0], c_h) and np.array_equal(got[:, 1], n_h)
    c, T = pairs[:, 0], pairs[:, 1]
    assert np.array_equal(n_h, np.minimum(T, max_history)) and (c_h <= n_h).all() and (c_h >= 0).all()
    assert np.array_equal(c_h[T <= max_history], c[T <= max_history])          # carried as they are, T = max_history included
    assert (c_h[c == 0] == 0).all() and np.array_equal(c_h[c == T], n_h[c == T])
    over = T > max_history                                                     # rounded to nearest: within half a sample
    assert (np.abs(c_h[over] * T[over].astype(np.int64) - c[over].astype(np.int64) * max_history) * 2 <= T[over]).all()


def test_seed_structured(exe, tmp_path):
    # max_history = 3 and 8 samples: c = 0 .. 8 -> (3 c + 4) / 8
    pairs = np.stack([np.arange(9), np.full(9, 8)], 1)
    got = run_pairs(exe, tmp_path, "seed", pairs, np.int32, (3,))
    assert list(got[:, 0]) == [0, 0, 1, 1, 2, 2, 2, 3, 3] and (got[:, 1] == 3).all()
    got = run_pairs(exe, tmp_path, "seed", [(2, 2), (2, 3), (2, 4)], np.int32, (3,))
    assert [tuple(g) for g in got] == [(2, 2), (2, 3), (2, 3)]     # just below, at, above: 2 of 4 -> (6 + 2) / 4 = 2 of 3


def test_resolves_match_numpy(exe, tmp_path):
    rng = np.random.default_rng(11)
    N = rng.integers(1, 16 * 2048 + 1, 5000)
    S = rng.integers(0, N + 1)
    pairs = np.concatenate([np.stack([S, N], 1), [(0, 1), (1, 1), (0, 7), (7, 7), (3, 7)]])
    got = run_pairs(exe, tmp_path, "resolve", pairs, np.float32)
    want = hl.resolve(pairs[:, 0], pairs[:, 1], 0)
    assert np.array_equal(got[:, 0].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, 1].view(np.uint32), want.view(np.uint32))
    # before any move every weight is 0: the totals are n and m n, the resolves history off computes
    assert np.array_equal(hl.resolve(S, np.zeros_like(S), 5).view(np.uint32), ol.visibility(S, 5).view(np.uint32))
