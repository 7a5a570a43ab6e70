"""The interleaved direction pattern and the filtered resolve of rt_occlusion on the GPU
(rt_occlusion_set_pattern / rt_occlusion_set_filter / rt_occlusion_config, Scene.set_occlusion_pattern /
set_occlusion_filter / occlusion_config, rtracer --occlusion N --interleave --filter).

The yardsticks are those of tests/test_gpu_occlusion.py: the rays of sample k are the numpy
restatement (tests/occl_lib.py) of the frame's pixel-mode query with table entry 16 k + c per
pixel, bit for bit; the counts are the sums of rt_query(any_hit, tmax = radius)'s flags on exactly
those rays, under both lane mappings (RT_OCCL_MAP = tile / class); the filtered outputs are the
restatement of tests/occl_filter_lib.py built from the call's own counts and the query's surface
records.  Cases and builders are test_gpu_occlusion.py's, plus world8_stress at 33 x 9 (two 32 x 32
regions, one clipped to a column) and 3 x 2 (smaller than a 4 x 4 block), and for the filter
rotated12 seen from the side (so that its defaults reject taps for each reason).  The references are
computed once per case and shared, never written to.  The host twin is
tests/test_occlusion_filter_host.py."""
import subprocess

import numpy as np
import pytest

import occl_filter_lib as fl
import occl_lib as ol
import query_cases as qc
import test_gpu_occlusion as base
from conftest import scene_path
from test_gpu_occlusion import CLI, INF, RADII, bits

pytestmark = pytest.mark.gpu
N = 4                                                              # samples of the count and filter checks
CASES = dict(base.CASES)
CASES["stress_33x9"] = ((33, 9), True, lambda rt, size, tmp: base._stress(rt, size))
CASES["stress_3x2"] = ((3, 2), True, lambda rt, size, tmp: base._stress(rt, size))
# rotated12 from the side, for the filter: from test_gpu_occlusion.py's camera no two neighbouring pixels
# lie on near-parallel faces of different cubes (no tap is rejected by the plane test); from here some do
SIDE_CAMERA = ((-4.5, 2.5, -3.0), (0.2, 0.35, 0.0, 0.915))
CASES["rotated12_side"] = ((64, 48), True, lambda rt, size, tmp: _rotated12_side(rt, size))
COUNT_CASES = ("stress_odd", "rotated12", "chain", "world1_brute", "stress_33x9", "stress_3x2")
FILTER_CASES = ("stress_odd", "rotated12_side")


def _rotated12_side(rt, size):
    s = base._rotated12(rt, size)
    s.set_camera(*SIDE_CAMERA)
    return s


def make(rt, name, tmp):
    size, bvh, build = CASES[name]
    return build(rt, size, tmp), bvh


@pytest.fixture(scope="module")
def table(gpu):
    t = np.stack([gpu.ao_direction(k) for k in range(ol.AO_MAX_SAMPLES)]).astype(np.float32)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def refs(gpu, table, tmp_path_factory):
    """Per case, once: the pixel-mode query's hit mask and surface records (p, faced n), the
    restated interleaved rays of samples 0 .. N - 1 at the default bias, and per radius the counts:
    the sum over k of rt_query(any_hit, tmax = radius)'s flag on sample k's rays, hit pixels only."""
    cache = {}

    def get(name):
        if name not in cache:
            s, bvh = make(gpu, name, tmp_path_factory.mktemp("occlf_" + name))
            (W, H) = CASES[name][0]
            q = s.query(pixels=qc.all_pixels(W, H), use_bvh=bvh, want=("t", "normal", "rays_out", "hit"))
            hit = q["hit"] != 0
            ro = q["rays_out"]
            t = np.where(hit, q["t"], np.float32(0)).astype(np.float32)
            p = ol.surface_point(ol.f32(ro[:, 0:3]), ol.f32(ro[:, 3:6]), t)
            n = ol.faced(ol.f32(q["normal"]), ol.f32(ro[:, 3:6]))
            rays = []
            for k in range(N):
                dk = table[fl.entries(W, H, k).ravel()]
                org, raw = ol.sample_rays(ro[:, 0:3], ro[:, 3:6], t, q["normal"], dk, gpu.RT_AO_BIAS_DEFAULT)
                r = np.concatenate([org, raw], axis=1).astype(np.float32)
                r[~hit] = 0
                rays.append(r)
            counts = {}
            for radius in RADII:
                c = np.zeros(W * H, np.int32)
                if hit.any():
                    for k in range(N):
                        f = s.query(origins=rays[k][hit, 0:3], dirs=rays[k][hit, 3:6], tmax=radius, any_hit=True, use_bvh=bvh,
                                    want=("hit",))["hit"]
                        c[hit] += (f != 0).astype(np.int32)
                counts[radius] = c
            ref = {"hit": hit, "p": p.reshape(H, W, 3), "n": n.reshape(H, W, 3), "rays": rays, "counts": counts}
            for v in [hit, ref["p"], ref["n"]] + rays + list(counts.values()):
                v.setflags(write=False)
            cache[name] = ref
        return cache[name]
    return get


def interleaved(rt, name, tmp):
    s, bvh = make(rt, name, tmp)
    s.set_occlusion_pattern("interleaved")
    return s, bvh


# ---- 1. rays ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("stress_odd", "rotated12"))
def test_interleaved_rays_are_the_restatement(gpu, refs, tmp_path, name):
    ref = refs(name)
    assert ref["hit"].any() and not ref["hit"].all()
    s, bvh = interleaved(gpu, name, tmp_path)
    (W, H) = CASES[name][0]
    assert s.occlusion(samples=1, use_bvh=bvh)["n"] == 1
    for k in (0, 1, 3):
        got = s._occlusion_rays(k).reshape(W * H, 6)
        ne = (bits(got) != bits(ref["rays"][k])).any(axis=1)
        assert not ne.any(), (name, k, int(ne.sum()))
    # the pixels of a block differ: the shared pattern's sample 0 is the normal everywhere, this one's only in class 0
    shared, _ = make(gpu, name, tmp_path)
    shared.occlusion(samples=1, use_bvh=bvh)
    same = (bits(shared._occlusion_rays(0).reshape(W * H, 6)) == bits(ref["rays"][0])).all(axis=1)
    cls0 = fl.pixel_class(W, H).ravel() == 0
    assert same[cls0 | ~ref["hit"]].all() and not same[~cls0 & ref["hit"]].any()
    with pytest.raises(gpu.RtError) as e:
        s._occlusion_rays(64)
    assert e.value.code == gpu.RT_ERR_ARG
    s._occlusion_rays(63)


# ---- 2. counts, under both lane mappings --------------------------------------------------------------
@pytest.mark.parametrize("mapping", ("tile", "class"))
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", COUNT_CASES)
def test_interleaved_counts_are_rt_query_on_the_same_rays(gpu, refs, tmp_path, monkeypatch, name, radius, mapping):
    ref = refs(name)
    monkeypatch.setenv("RT_OCCL_MAP", mapping)
    s, bvh = interleaved(gpu, name, tmp_path)
    (W, H) = CASES[name][0]
    assert s.occlusion_config["map"] is None
    fr = s.occlusion(samples=N, radius=radius, use_bvh=bvh, want=("visibility", "occluded", "rgba"))
    assert fr["n"] == N and s.occlusion_info == (N, W, H, 0)
    assert s.occlusion_config["map"] == mapping
    got, want = fr["occluded"].ravel(), ref["counts"][radius]
    assert np.array_equal(got, want), (name, radius, mapping, int((got != want).sum()))
    assert (got[~ref["hit"]] == 0).all()
    if name in ("stress_odd", "rotated12", "chain"):
        assert 0 < got.sum() < N * ref["hit"].sum(), "the case needs occluded and open samples"
    vis = ol.visibility(want, N)
    assert np.array_equal(bits(fr["visibility"].ravel()), bits(vis)), (name, radius)
    assert np.array_equal(fr["rgba"].ravel(), ol.grey(vis)), (name, radius)
    got_rays = s._occlusion_rays(N - 1).reshape(W * H, 6)
    assert np.array_equal(bits(got_rays), bits(ref["rays"][N - 1]))


def test_the_shared_pattern_has_no_class_map(gpu, tmp_path, monkeypatch):
    monkeypatch.setenv("RT_OCCL_MAP", "class")
    s, _ = make(gpu, "stress_odd", tmp_path)
    s.occlusion(samples=1)
    assert s.occlusion_config["map"] == "tile"


# ---- 3. splits and the limit --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("stress_odd", "rotated12"))
def test_splits_and_the_limit(gpu, refs, tmp_path, name):
    a, bvh = interleaved(gpu, name, tmp_path)
    b, _ = interleaved(gpu, name, tmp_path)
    want = ("occluded", "visibility")
    whole = a.occlusion(samples=4, radius=2.0, use_bvh=bvh, want=want)
    for n in (1, 2, 1):
        parts = b.occlusion(samples=n, radius=2.0, use_bvh=bvh, want=want)
    assert whole["n"] == parts["n"] == 4
    for k in want:
        assert np.array_equal(bits(whole[k]), bits(parts[k])), (name, k)
    assert np.array_equal(whole["occluded"].ravel(), refs(name)["counts"][2.0])
    with pytest.raises(gpu.RtError) as e:                              # 4 + 61 = 65
        a.occlusion(samples=61, radius=2.0, use_bvh=bvh, want=want)
    assert e.value.code == gpu.RT_ERR_LIMIT and a.occlusion_info[0] == 4 and a.occlusion_info[3] == 0
    with pytest.raises(gpu.RtError) as e:
        a.occlusion(samples=65, radius=2.0, restart=True, use_bvh=bvh, want=want)
    assert e.value.code == gpu.RT_ERR_LIMIT and a.occlusion_info[0] == 4
    full = a.occlusion(samples=60, radius=2.0, use_bvh=bvh, want=want)   # exactly 64
    once = b.occlusion(samples=64, radius=2.0, restart=True, use_bvh=bvh, want=want)
    assert full["n"] == once["n"] == 64 == a.occlusion_config["capacity"]
    for k in want:
        assert np.array_equal(bits(full[k]), bits(once[k])), (name, k)
    assert np.array_equal(bits(full["visibility"]), bits(ol.visibility(full["occluded"], 64)))


# ---- 4. the filtered outputs --------------------------------------------------------------------------
@pytest.mark.parametrize("params", ("defaults", "all"))
@pytest.mark.parametrize("pattern", ("shared", "interleaved"))
@pytest.mark.parametrize("name", FILTER_CASES)
def test_filtered_outputs_are_the_restatement(gpu, refs, tmp_path, name, pattern, params):
    ref = refs(name)
    (W, H) = CASES[name][0]
    live = ref["hit"].reshape(H, W)
    s, bvh = make(gpu, name, tmp_path)
    s.set_occlusion_pattern(pattern)
    want = ("visibility", "occluded", "rgba")
    plain = s.occlusion(samples=N, radius=2.0, use_bvh=bvh, want=want)
    nm, pt = (fl.NORMAL_DEFAULT, fl.PLANE_DEFAULT) if params == "defaults" else (-1.0, 1e30)
    s.set_occlusion_filter(True, normal_min=nm, plane_tol=pt)
    fr = s.occlusion(samples=N, radius=2.0, restart=True, use_bvh=bvh, want=want)
    assert fr["n"] == N
    assert np.array_equal(fr["occluded"], plain["occluded"])           # the counts are raw, filter on or off
    if pattern == "interleaved":
        assert np.array_equal(fr["occluded"].ravel(), ref["counts"][2.0])
    vis, census, S, m = fl.filtered(ref["p"], ref["n"], live, fr["occluded"], N, nm, pt)
    print(name, pattern, params, census, "mean |filtered - raw| %.4f" % float(np.abs(vis - plain["visibility"]).mean()))
    assert np.array_equal(bits(fr["visibility"]), bits(vis)), (name, pattern, params, int((bits(fr["visibility"]) != bits(vis)).sum()))
    assert np.array_equal(fr["rgba"], ol.grey(vis)), (name, pattern, params)
    assert (fr["visibility"][~live] == 1).all()
    if params == "defaults":                                           # the case exercises every reason to reject a tap
        assert census["not_live"] > 0 and census["normal"] > 0 and census["plane"] > 0 and census["clipped"] > 0, census
        assert not np.array_equal(bits(fr["visibility"]), bits(plain["visibility"]))
    else:                                                              # everything live is accepted
        assert census["normal"] == 0 and census["plane"] == 0 and census["not_live"] > 0
        cnt = np.where(live, 1, 0)
        assert np.array_equal(m, sum(fl._shift(cnt, dx, dy, 0) for dx, dy in fl.TAPS) * cnt)
    # one output alone, and more samples on top: the filter follows the samples held
    more = s.occlusion(samples=2, radius=2.0, use_bvh=bvh, want=("visibility", "occluded"))
    assert more["n"] == N + 2
    vis2 = fl.filtered(ref["p"], ref["n"], live, more["occluded"], N + 2, nm, pt)[0]
    assert np.array_equal(bits(more["visibility"]), bits(vis2))
    only = s.occlusion(samples=1, radius=2.0, use_bvh=bvh, want=("rgba",))
    raw = s.occlusion(samples=1, radius=2.0, use_bvh=bvh, want=("occluded",))
    assert raw["n"] == N + 4 and only["rgba"].shape == (H, W)


# ---- 5. closed forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ("shared", "interleaved"))
def test_closed_forms_with_the_filter(gpu, pattern):
    s = base._cubes(gpu, (32, 24), [((0.0, 0.0, 0.0), (0, 0, 0, 1))], scales=(1.0,), unit=24.0)
    s.set_occlusion_pattern(pattern)
    s.set_occlusion_filter(True)
    hit = s.query(pixels=qc.all_pixels(32, 24), want=("hit",))["hit"].reshape(24, 32) != 0
    assert 40 <= hit.sum() < 32 * 24
    fr = s.occlusion(samples=16, want=("visibility", "occluded"))
    assert (fr["occluded"] == 0).all() and (fr["visibility"] == 1).all()
    edge = 20.0
    s = base._cubes(gpu, (32, 24), [((0.0, 0.0, 0.0), (0, 0, 0, 1))], scales=(edge,), cam=((1.0, 2.0, -3.0), base.DOWN45), unit=24.0)
    s.set_occlusion_pattern(pattern)
    s.set_occlusion_filter(True)
    fr = s.occlusion(samples=16, want=("visibility", "occluded", "rgba"))
    assert (fr["occluded"] == 16).all() and (fr["visibility"] == 0).all() and (fr["rgba"] == 0x000000FF).all()


# ---- 6. state -----------------------------------------------------------------------------------------
def test_state(gpu, refs, tmp_path):
    ref = refs("stress_odd")
    (W, H) = CASES["stress_odd"][0]
    live = ref["hit"].reshape(H, W)
    s, _ = make(gpu, "stress_odd", tmp_path)
    want = ("visibility", "occluded")
    s.set_occlusion_pattern("interleaved")
    s.set_occlusion_pattern("interleaved")
    assert s.occlusion_info == (0, W, H, 0)                            # nothing held: nothing counted
    a = s.occlusion(samples=2, radius=2.0, want=want)
    assert np.array_equal(bits(a["visibility"]), bits(ol.visibility(a["occluded"], 2)))
    # the filter toggles between calls: n and the restart counter stay, the outputs follow
    s.set_occlusion_filter(True)
    assert s.occlusion_info == (2, W, H, 0)
    b = s.occlusion(samples=2, radius=2.0, want=want)
    assert b["n"] == 4 and s.occlusion_info[3] == 0
    assert np.array_equal(b["occluded"].ravel(), ref["counts"][2.0])
    assert np.array_equal(bits(b["visibility"]), bits(fl.filtered(ref["p"], ref["n"], live, b["occluded"], 4)[0]))
    s.set_occlusion_filter(False)
    c = s.occlusion(samples=1, radius=2.0, want=want)
    assert c["n"] == 5 and s.occlusion_info[3] == 0
    assert np.array_equal(bits(c["visibility"]), bits(ol.visibility(c["occluded"], 5)))
    # the same pattern again: nothing; another: the samples are dropped, one restart
    s.set_occlusion_pattern("interleaved")
    assert s.occlusion_info == (5, W, H, 0)
    s.set_occlusion_pattern("shared")
    assert s.occlusion_info == (0, W, H, 1)
    s.set_occlusion_pattern("shared")
    assert s.occlusion_info == (0, W, H, 1)
    d = s.occlusion(samples=2, radius=2.0, want=want)
    fresh, _ = make(gpu, "stress_odd", tmp_path)
    e = fresh.occlusion(samples=2, radius=2.0, want=want)
    assert d["n"] == 2 and all(np.array_equal(bits(d[k]), bits(e[k])) for k in want)
    s.set_occlusion_pattern("interleaved")                             # held: counted once
    assert s.occlusion_info == (0, W, H, 2) and s.occlusion_config["pattern"] == "interleaved"


def test_render_in_between_and_the_frame_state(gpu, tmp_path):
    a, _ = make(gpu, "stress", tmp_path)
    b, _ = make(gpu, "stress", tmp_path)
    for s in (a, b):
        s.set_occlusion_pattern("interleaved")
        s.set_occlusion_filter(True)
    want = ("rgba", "radiance", "hit_inst", "hit_tri")
    r4 = b.render(spp=4, want=want, stats=False)
    k4 = b.last_trace()
    for n in (1, 2):
        ra = a.render(spp=4, want=want, stats=False)
        assert all(np.array_equal(bits(ra[k]), bits(r4[k])) for k in want) and a.last_trace() == k4
        trace, hist = a.last_trace(), a._history_info()
        fa = a.occlusion(radius=2.0, rebuild_bvh=(n != 2), want=("occluded", "visibility"))
        now = a._history_info()
        assert a.last_trace() == trace
        assert now[:1] + now[2:] == hist[:1] + hist[2:], (n, hist, now)
        if n == 2:
            assert now == hist, (hist, now)
        fb = b.occlusion(radius=2.0, want=("occluded", "visibility"))
        assert fa["n"] == fb["n"] == n
        for k in ("occluded", "visibility"):
            assert np.array_equal(bits(fa[k]), bits(fb[k])), (n, k)
    ra = a.render(spp=4, want=want, stats=False)
    assert all(np.array_equal(bits(ra[k]), bits(r4[k])) for k in want)


# ---- 7. the defaults are the scene that never touched the new entries ---------------------------------
@pytest.mark.parametrize("name", ("stress_odd", "rotated12"))
def test_defaults_are_untouched(gpu, tmp_path, name):
    plain, bvh = make(gpu, name, tmp_path)
    s, _ = make(gpu, name, tmp_path)
    s.set_occlusion_pattern("interleaved")
    s.set_occlusion_filter(True, normal_min=0.5, plane_tol=0.1)
    s.occlusion(samples=3, radius=2.0, use_bvh=bvh)
    s.set_occlusion_pattern("shared")
    s.set_occlusion_filter(False)
    want = ("visibility", "occluded", "rgba")
    for n in (3, 2):
        x = s.occlusion(samples=n, radius=2.0, use_bvh=bvh, want=want)
        y = plain.occlusion(samples=n, radius=2.0, use_bvh=bvh, want=want)
        assert x["n"] == y["n"]
        for k in want:
            assert x[k].tobytes() == y[k].tobytes(), (name, n, k)
    assert s._occlusion_rays(4).tobytes() == plain._occlusion_rays(4).tobytes()


# ---- 8. host and device pointers ----------------------------------------------------------------------
def test_host_and_device_pointers_agree_with_the_filter(gpu, tmp_path):
    import torch
    a, _ = interleaved(gpu, "stress_odd", tmp_path)
    b, _ = interleaved(gpu, "stress_odd", tmp_path)
    for s in (a, b):
        s.set_occlusion_filter(True)
    (W, H) = CASES["stress_odd"][0]
    vis = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    occ = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    rgba = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    for n in (1, 2, 3):
        host = a.occlusion(radius=2.0, want=("visibility", "occluded", "rgba"))
        got = b.occlusion_device(radius=2.0, visibility_ptr=vis.data_ptr(), occluded_ptr=occ.data_ptr(), rgba_ptr=rgba.data_ptr())
        assert got == host["n"] == n
        assert np.array_equal(bits(vis.cpu().numpy()), bits(host["visibility"]))
        assert np.array_equal(occ.cpu().numpy(), host["occluded"])
        assert np.array_equal(rgba.cpu().numpy().view(np.uint32), host["rgba"])
    vis.fill_(-5.0)
    assert b.occlusion_device(radius=2.0, rgba_ptr=rgba.data_ptr()) == 4      # one filtered output alone
    assert (vis == -5.0).all()
    assert np.array_equal(rgba.cpu().numpy().view(np.uint32), a.occlusion(radius=2.0, want=("rgba",))["rgba"])


# ---- 9. CLI -------------------------------------------------------------------------------------------
def test_cli_interleave_and_filter(gpu, tmp_path):
    W, H = 96, 64
    cli = [CLI, "-c", scene_path("world8_stress"), "--width", str(W), "--height", str(H)]
    for flags in (["--interleave", "--filter"], ["--interleave"], ["--filter", "--radius", "2"]):
        s = gpu.Scene.load_json(scene_path("world8_stress"), W, H)
        if "--interleave" in flags:
            s.set_occlusion_pattern("interleaved")
        if "--filter" in flags:
            s.set_occlusion_filter(True)
        out = str(tmp_path / "ao.ppm")
        r = subprocess.run(cli + ["--occlusion", "4", "--out", out] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "Occlusion: 4 samples" in r.stdout
        rgba = s.occlusion(samples=4, radius=2.0 if "--radius" in flags else INF, want=("rgba",))["rgba"]
        want = np.stack([(rgba >> 24) & 255, (rgba >> 16) & 255, (rgba >> 8) & 255], axis=-1).astype(np.uint8)
        assert np.array_equal(base._ppm_rgb(out, W, H), want), flags
        if flags == ["--interleave", "--filter"]:
            assert len(np.unique(want)) > 5                            # more grey levels than 4 shared samples have
    for lone in (["--interleave"], ["--filter"], ["--interleave", "--filter"]):
        assert subprocess.run(cli + lone, capture_output=True, text=True, timeout=120).returncode == 2
    assert subprocess.run(cli + ["--occlusion", "65", "--interleave"], capture_output=True, text=True, timeout=120).returncode == 1
