"""The interleaved direction pattern and the filtered resolve of rt_occlusion on the host.

- rt_occlusion_set_pattern / rt_occlusion_set_filter / rt_occlusion_config on a scene without a
  device: every RT_ERR_ARG case, the state read back, no restart from the filter, none counted from
  a pattern change while no samples are held, the interleaved pattern's limit of 64 checked with
  the arguments.
- The accept test and the resolve occl_filter_kernel compiles (csrc/rt_occl.h, through
  tests/occl_filter_host.cpp with the kernels' float rules) against the numpy float32 restatement
  of tests/occl_filter_lib.py, bit for bit, on synthetic records: coplanar pixels, planes stepped
  by just less than, exactly and just more than plane_tol, normals at, above and below normal_min,
  taps that are not live, NaN records, the canvas corners, canvases of 1 x 1, 3 x 2 and 5 x 5.
- occlusion_plan (csrc/rt_plan.h) for the class map: wave count and grid, and over all waves and
  lanes the restated pixel function hits every pixel exactly once with the right class.
- The window property: every 4 x 4 window position holds 16 distinct classes, so after n samples
  it has used entries 0 .. 16 n - 1 once each.
The GPU twin is tests/test_gpu_occlusion_filter.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import occl_filter_lib as fl
from conftest import ROOT, scene_path

F = np.float32
TOL = F(fl.PLANE_DEFAULT)
NMIN = F(fl.NORMAL_DEFAULT)


def f32_bits(v):
    return int(np.array([v], np.float32).view(np.uint32)[0])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    path = str(tmp_path_factory.mktemp("occl_filter") / "occl_filter_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math",
                    "-fno-slp-vectorize", "-I", os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "occl_filter_host.cpp"), "-o", path],
                   check=True, capture_output=True, text=True)
    return path


# ---- the entries' argument checks and state --------------------------------------------------------------
def test_argument_checks_and_state(rt):
    L = rt.lib()
    s = rt.Scene.load_json(scene_path("world1"), 16, 12)
    assert s.occlusion_config == {"pattern": "shared", "filter": False, "capacity": 1024, "map": None,
                                  "normal_min": float(NMIN), "plane_tol": float(TOL)}
    assert (rt.RT_AO_PATTERN_SHARED, rt.RT_AO_PATTERN_INTERLEAVED, rt.RT_AO_INTERLEAVED_MAX_SAMPLES) == (0, 1, 64)
    assert F(rt.RT_AO_FILTER_NORMAL_DEFAULT) == NMIN and F(rt.RT_AO_FILTER_PLANE_DEFAULT) == TOL
    # the pattern
    for bad in (-1, 2, 16):
        assert L.rt_occlusion_set_pattern(s._h, bad) == rt.RT_ERR_ARG, bad
    assert L.rt_occlusion_set_pattern(None, 0) == rt.RT_ERR_ARG
    assert s.occlusion_config["pattern"] == "shared"
    s.set_occlusion_pattern("interleaved")
    assert s.occlusion_config["pattern"] == "interleaved" and s.occlusion_config["capacity"] == 64
    s.set_occlusion_pattern("interleaved")                         # nothing changes
    s.set_occlusion_pattern(rt.RT_AO_PATTERN_SHARED)
    s.set_occlusion_pattern("interleaved")
    assert s.occlusion_info == (0, 16, 12, 0)                      # no samples were held: no restart is counted
    # the filter
    for on in (-1, 2):
        assert L.rt_occlusion_set_filter(s._h, on, 0.9, 1e-2) == rt.RT_ERR_ARG, on
    for on in (0, 1):                                              # the parameters are validated with on = 0 too
        for nm in (float("nan"), -1.0000001, 1.0000001, float("inf"), float("-inf")):
            assert L.rt_occlusion_set_filter(s._h, on, nm, 1e-2) == rt.RT_ERR_ARG, (on, nm)
        for pt in (-1e-9, float("nan"), float("inf"), float("-inf")):
            assert L.rt_occlusion_set_filter(s._h, on, 0.9, pt) == rt.RT_ERR_ARG, (on, pt)
    assert L.rt_occlusion_set_filter(None, 1, 0.9, 1e-2) == rt.RT_ERR_ARG
    assert not s.occlusion_config["filter"]
    s.set_occlusion_filter(True, normal_min=-1.0, plane_tol=0.0)   # the ends of both ranges
    s.set_occlusion_filter(True, normal_min=1.0, plane_tol=1e30)
    c = s.occlusion_config
    assert c["filter"] and c["normal_min"] == 1.0 and c["plane_tol"] == float(F(1e30))
    s.set_occlusion_filter(False, normal_min=0.5, plane_tol=0.25)  # off: the parameters are ignored
    c = s.occlusion_config
    assert not c["filter"] and c["normal_min"] == 1.0 and c["plane_tol"] == float(F(1e30))
    s.set_occlusion_filter()
    c = s.occlusion_config
    assert c["filter"] and c["normal_min"] == float(NMIN) and c["plane_tol"] == float(TOL)
    assert s.occlusion_info == (0, 16, 12, 0)                      # the filter restarts nothing
    # rt_occlusion_config: either destination may be null
    a, f = np.full(4, -9, np.int32), np.full(2, -9, np.float32)
    assert L.rt_occlusion_config(s._h, a.ctypes.data, None) == rt.RT_OK and tuple(a) == (1, 1, 64, -1)
    assert L.rt_occlusion_config(s._h, None, f.ctypes.data) == rt.RT_OK and (f[0], f[1]) == (NMIN, TOL)
    assert L.rt_occlusion_config(s._h, None, None) == rt.RT_OK
    assert L.rt_occlusion_config(None, a.ctypes.data, f.ctypes.data) == rt.RT_ERR_ARG
    # the interleaved pattern's limit comes with the arguments, before any device work
    buf = np.zeros((12, 16), np.float32)
    o = rt.OcclusionOpts()
    L.rt_occlusion_opts_default(ctypes.byref(o))
    o.host_outputs, o.visibility, o.samples = 1, buf.ctypes.data, 65
    n = ctypes.c_int(-7)
    assert L.rt_occlusion(s._h, ctypes.byref(o), ctypes.byref(n)) == rt.RT_ERR_LIMIT
    assert b"interleaved" in L.rt_last_error() and n.value == -7
    rays = np.zeros((12, 16, 6), np.float32)
    assert L.rt_occlusion_rays(s._h, 64, rays.ctypes.data, rays.size) == rt.RT_ERR_ARG
    assert L.rt_occlusion_rays(s._h, 63, rays.ctypes.data, rays.size) == rt.RT_ERR_STATE   # no accumulation yet
    s.set_occlusion_pattern("shared")
    assert L.rt_occlusion_rays(s._h, 64, rays.ctypes.data, rays.size) == rt.RT_ERR_STATE
    if rt.device_count() == 0:
        o.samples = 64
        s.set_occlusion_pattern("interleaved")
        assert L.rt_occlusion(s._h, ctypes.byref(o), ctypes.byref(n)) == rt.RT_ERR_NODEV   # 64 are admitted
    assert s.occlusion_info == (0, 16, 12, 0)


# ---- the accept test and the resolve ---------------------------------------------------------------------
def up(v):
    return np.nextafter(F(v), F(np.inf))


def down(v):
    return np.nextafter(F(v), F(-np.inf))


def synthetic(W, H, seed, n_samples):
    """Records on the plane z = 0 seen along -z, then per pixel at random: a step in z of just less
    than, exactly or just more than plane_tol (or far more); a normal whose dot with (0, 0, 1) is
    at, just above or just below normal_min, or that looks away; not live; NaN in p or n."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    steps = np.array([0, 0, 0, down(TOL), TOL, up(TOL), -TOL, -up(TOL), 0.5], np.float32)
    p = np.stack([F(0.125) * x, F(0.125) * y, steps[rng.integers(0, len(steps), (H, W))]], axis=-1).astype(np.float32)
    normals = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0.4, 0, NMIN], [0.4, 0, up(NMIN)], [0, 0.4, down(NMIN)],
                        [0, 0, -1], [1, 0, 0]], np.float32)
    n = normals[rng.integers(0, len(normals), (H, W))]
    live = rng.random((H, W)) < 0.85
    nan = rng.random((H, W)) < 0.04
    p[nan & (x % 2 == 0), 1] = np.nan
    n[nan & (x % 2 == 1), 2] = np.nan
    count = rng.integers(0, n_samples + 1, (H, W)).astype(np.int32)
    return p, n.astype(np.float32), live, count


def run_filter(exe, tmp_path, p, n, live, count, n_samples, normal_min, plane_tol):
    H, W = live.shape
    rec = np.zeros((H, W, 8), np.float32)
    rec[..., 0:3], rec[..., 3:6] = p, n
    rec.view(np.int32)[..., 6], rec.view(np.int32)[..., 7] = live.astype(np.int32), count
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rec.tofile(fin)
    r = subprocess.run([exe, "filter", fin, fout, str(W), str(H), str(n_samples), str(f32_bits(normal_min)), str(f32_bits(plane_tol))],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.fromfile(fout, np.uint32).reshape(H, W, 3)
    return out[..., 0], out[..., 1].astype(np.int32), out[..., 2].astype(np.int32)


@pytest.mark.parametrize("size", [(1, 1), (3, 2), (5, 5), (4, 4), (37, 21)])
@pytest.mark.parametrize("n_samples", [1, 4, 64])
def test_filter_matches_numpy(exe, tmp_path, size, n_samples):
    W, H = size
    total = {"not_live": 0, "normal": 0, "plane": 0, "clipped": 0}
    for seed in range(3):
        p, n, live, count = synthetic(W, H, 100 * seed + W, n_samples)
        if seed == 0:
            live[0, 0] = live[-1, -1] = live[0, -1] = live[-1, 0] = True     # the corners as centres
        for nm, pt in ((NMIN, TOL), (F(-1), F(1e30)), (F(1), F(0))):
            vis, census, S, m = fl.filtered(p, n, live, count, n_samples, nm, pt)
            gv, gS, gm = run_filter(exe, tmp_path, p, n, live, count, n_samples, nm, pt)
            assert np.array_equal(gv, vis.view(np.uint32)), (size, seed, float(nm))
            assert np.array_equal(gS[live], S[live]) and np.array_equal(gm[live], m[live])
            assert (gm[~live] == 0).all() and (gv[~live] == f32_bits(1.0)).all()
            assert (1 <= m[live]).all() and (m <= 16).all()
            if nm == NMIN:
                for k in total:
                    total[k] += census[k]
            if nm == F(-1):                                        # everything live and free of NaN is accepted
                clean = live & ~np.isnan(p).any(-1) & ~np.isnan(n).any(-1)
                if clean.all():
                    assert (m[live] == _window_sizes(W, H)[live]).all()
    if size == (37, 21):                                           # every reason occurs, and the canvas clips windows
        assert all(v > 0 for v in total.values()), total
    if W * H > 1:
        assert total["clipped"] > 0


def _window_sizes(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return (np.minimum(x, 2) + 1 + np.minimum(W - 1 - x, 1)) * (np.minimum(y, 2) + 1 + np.minimum(H - 1 - y, 1))


def test_filter_structured_cases(exe, tmp_path):
    """A 5 x 5 coplanar canvas, one feature at a time, read at the centre pixel (2, 2) whose window
    is x, y in [0, 3]: 16 taps."""
    W = H = 5
    y, x = np.mgrid[0:H, 0:W]

    def base():
        p = np.stack([F(0.125) * x, F(0.125) * y, np.zeros((H, W), np.float32)], axis=-1).astype(np.float32)
        n = np.zeros((H, W, 3), np.float32)
        n[..., 2] = 1
        return p, n, np.ones((H, W), bool), ((x + 2 * y) % 5).astype(np.int32)

    def both(p, n, live, count, n_samples=4):
        vis, _, S, m = fl.filtered(p, n, live, count, n_samples, NMIN, TOL)
        gv, gS, gm = run_filter(exe, tmp_path, p, n, live, count, n_samples, NMIN, TOL)
        assert np.array_equal(gv, vis.view(np.uint32)) and np.array_equal(gS, S) and np.array_equal(gm, m)
        return vis, S, m

    p, n, live, count = base()
    vis, S, m = both(p, n, live, count)
    assert m[2, 2] == 16 and S[2, 2] == count[0:4, 0:4].sum()
    assert m[0, 0] == 4 and m[4, 4] == 9 and m[0, 4] == 6 and m[4, 0] == 6      # the corners' clipped windows
    assert vis[2, 2] == F(1) - F(S[2, 2]) / F(16 * 4)
    for dz, accepted in ((down(TOL), True), (TOL, True), (up(TOL), False), (-TOL, True), (-up(TOL), False)):
        p, n, live, count = base()
        p[1, 1, 2] = dz
        _, S, m = both(p, n, live, count)
        assert m[2, 2] == (16 if accepted else 15), float(dz)
    for nz, accepted in ((NMIN, True), (up(NMIN), True), (down(NMIN), False), (F(-1), False)):
        p, n, live, count = base()
        n[1, 3] = (0.3, 0, nz)
        _, S, m = both(p, n, live, count)
        assert m[2, 2] == (16 if accepted else 15), float(nz)
    p, n, live, count = base()
    live[3, 0] = live[0, 3] = False
    _, S, m = both(p, n, live, count)
    assert m[2, 2] == 14 and S[2, 2] == count[0:4, 0:4].sum() - count[3, 0] - count[0, 3]
    p, n, live, count = base()                                     # a NaN tap accepts nothing; a NaN centre keeps itself only
    p[1, 2, 0] = np.nan
    n[2, 1, 1] = np.nan
    vis, S, m = both(p, n, live, count)
    assert m[2, 2] == 14 and m[1, 2] == 1 and m[2, 1] == 1
    assert vis[1, 2] == F(1) - F(count[1, 2]) / F(4)
    p, n, live, count = base()                                     # a centre that is not live: visibility 1
    live[2, 2] = False
    vis, S, m = both(p, n, live, count)
    assert vis[2, 2] == 1


# ---- the pattern and the class map -----------------------------------------------------------------------
def test_classes_and_the_window_property(exe, tmp_path):
    W, H = 50, 37
    for k in (0, 3, 63):
        out = str(tmp_path / "classes.bin")
        assert subprocess.run([exe, "classes", out, str(W), str(H), str(k)]).returncode == 0
        got = np.fromfile(out, np.int32).reshape(H, W, 2)
        assert np.array_equal(got[..., 0], fl.pixel_class(W, H)) and np.array_equal(got[..., 1], fl.entries(W, H, k))
        assert got[..., 1].min() == 16 * k and got[..., 1].max() == 16 * k + 15 < 1024
    cls = fl.pixel_class(W, H)
    for y0 in range(H - 3):
        for x0 in range(W - 3):
            assert len(np.unique(cls[y0:y0 + 4, x0:x0 + 4])) == 16, (x0, y0)
    # after n samples a window has used entries 0 .. 16 n - 1 once each
    n = 4
    used = np.stack([fl.entries(W, H, k) for k in range(n)])
    for (x0, y0) in ((0, 0), (1, 2), (46, 33), (7, 5)):
        assert sorted(used[:, y0:y0 + 4, x0:x0 + 4].ravel()) == list(range(16 * n))


def run_plan(exe, W, H, mapping, pattern):
    out = subprocess.run([exe, "plan", str(W), str(H), str(mapping), str(pattern)], check=True, capture_output=True, text=True).stdout.split()
    return dict(zip(("tree", "map", "n_waves", "block", "blocks", "pattern", "filter_bx", "filter_by", "default_il"), (int(v) for v in out)))


@pytest.mark.parametrize("size", [(1, 1), (33, 9), (50, 37), (1920, 1080)])
def test_class_map_plan_covers_the_frame(exe, size):
    W, H = size
    p = run_plan(exe, W, H, fl.CLASS, fl.INTERLEAVED)
    waves, blocks = fl.class_plan(W, H)
    assert (p["map"], p["pattern"], p["n_waves"], p["block"], p["blocks"]) == (fl.CLASS, fl.INTERLEAVED, waves, 256, blocks)
    assert waves == 16 * -(-W // 32) * -(-H // 32) and blocks * 4 >= waves
    assert (p["filter_bx"], p["filter_by"]) == (-(-W // 32), -(-H // 8))
    # every pixel exactly once, with its class, over all waves and lanes (vectorised restatement of class_pixel)
    g, lane = np.meshgrid(np.arange(waves), np.arange(64), indexing="ij")
    c, rg = g & 15, g >> 4
    n_rx = (W + 31) >> 5
    ry, rx = rg // n_rx, rg % n_rx
    x, y = 32 * rx + 4 * (lane & 7) + (c & 3), 32 * ry + 4 * (lane >> 3) + (c >> 2)
    ok = (x < W) & (y < H)
    idx = (y * W + x)[ok]
    assert idx.size == W * H and np.array_equal(np.sort(idx), np.arange(W * H))
    assert np.array_equal(fl.pixel_class(W, H).ravel()[idx], c[ok])
    for gg, ll in ((0, 0), (waves - 1, 63), (min(17, waves - 1), 9)):                  # the scalar form agrees
        i, cc = fl.class_pixel(W, H, gg, ll)
        assert cc == c[gg, ll] and i == (y[gg, ll] * W + x[gg, ll] if ok[gg, ll] else -1)


def test_plan_maps_per_pattern(exe):
    # the class map belongs to the interleaved pattern; the shared pattern's plan is what it was
    assert run_plan(exe, 96, 64, fl.CLASS, fl.SHARED)["map"] == fl.TILE
    assert run_plan(exe, 96, 64, -1, fl.SHARED)["map"] == fl.TILE
    for m in (fl.ROW, fl.TILE):
        a, b = run_plan(exe, 50, 37, m, fl.SHARED), run_plan(exe, 50, 37, m, fl.INTERLEAVED)
        assert a["map"] == b["map"] == m and a["n_waves"] == b["n_waves"] and a["blocks"] == b["blocks"]
    d = run_plan(exe, 96, 64, -1, fl.INTERLEAVED)
    assert d["map"] == d["default_il"] and d["default_il"] in (fl.TILE, fl.CLASS)
    assert run_plan(exe, 96, 64, 7, fl.INTERLEAVED)["map"] == d["default_il"]
