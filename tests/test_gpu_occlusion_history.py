"""rt_occlusion's history across camera moves on the GPU (rt_occlusion_set_history /
rt_occlusion_history_info / rt_occlusion_history_weights, Scene.set_occlusion_history /
occlusion_history, rtracer --occlusion N --history).

The yardstick is never the new kernels: the surface records at every pose are the numpy
restatement of the frame's pixel-mode query (tests/occl_lib.py), the occluded samples are the sums
of rt_query(any_hit, tmax = radius)'s flags on the restated rays of the sample indices the cursor
names, and the seed, the weights and both resolves are the restatement of
tests/occl_history_lib.py -- all compared bit for bit.  Cases and builders are
tests/test_gpu_occlusion.py's and test_gpu_occlusion_filter.py's; the poses B were chosen so that
one move rejects pixels for every reason (the restatement's census is asserted).  The references
are computed once per (case, pose, pattern, radius, sample) and shared, never written to.  The
host twin is tests/test_occlusion_history_host.py."""
import subprocess

import numpy as np
import pytest

import occl_filter_lib as fl
import occl_history_lib as hl
import occl_lib as ol
import query_cases as qc
import test_gpu_occlusion as base
import test_gpu_occlusion_filter as flt
from conftest import scene_path
from test_gpu_occlusion import CLI, RADII, bits

pytestmark = pytest.mark.gpu
CASES = flt.CASES
WANT = ("visibility", "occluded", "rgba")
# pose A is the case's own camera; B turns and shifts it (every reason to reject a source occurs);
# C is a further small shift of B
POSES = {
    "stress_odd": (qc.VALUES_CAMERA, ((-1.06, 7.85, -6.72), (0.3664, -0.02495, 0.01293, 0.93003)),
                   ((-0.81, 7.85, -7.22), (0.3664, -0.02495, 0.01293, 0.93003))),
    "rotated12_side": (flt.SIDE_CAMERA, ((-4.23, 2.88, -2.42), (0.20047, 0.38832, 0.02568, 0.89909)),
                       ((-3.98, 2.88, -2.92), (0.20047, 0.38832, 0.02568, 0.89909))),
    "stress_3x2": (qc.VALUES_CAMERA,),
    "rotated12": (((0.1, 4.5, -4.2), base.DOWN45), ((0.35, 4.5, -4.7), base.DOWN45), ((0.6, 4.5, -5.2), base.DOWN45)),
}


def make(rt, name, tmp, pose=0, pattern="shared", history=True, **kw):
    s, bvh = flt.make(rt, name, tmp)
    if pose:
        s.set_camera(*POSES[name][pose])
    s.set_occlusion_pattern(pattern)
    if history:
        s.set_occlusion_history(True, **kw)
    return s, bvh


@pytest.fixture(scope="module")
def table(gpu):
    t = np.stack([gpu.ao_direction(k) for k in range(ol.AO_MAX_SAMPLES)]).astype(np.float32)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def frames(gpu, table, tmp_path_factory):
    """get(name, pose) -> the frame at that pose from parent code and numpy alone: "live", "p", "n"
    (the query's surface record), "cam" (DCamera's fields) and count(pattern, radius, ks): the
    occluded samples among the pattern's sample indices ks, (H, W) int32."""
    cache = {}

    def get(name, pose):
        if (name, pose) in cache:
            return cache[(name, pose)]
        s, bvh = flt.make(gpu, name, tmp_path_factory.mktemp("occlh_%s_%d" % (name, pose)))
        s.set_camera(*POSES[name][pose])
        (W, H) = CASES[name][0]
        q = s.query(pixels=qc.all_pixels(W, H), use_bvh=bvh, want=("t", "normal", "rays_out", "hit"))
        hit = q["hit"] != 0
        ro = q["rays_out"]
        t = np.where(hit, q["t"], np.float32(0)).astype(np.float32)
        p = ol.surface_point(ol.f32(ro[:, 0:3]), ol.f32(ro[:, 3:6]), t).reshape(H, W, 3)
        n = ol.faced(ol.f32(q["normal"]), ol.f32(ro[:, 3:6])).reshape(H, W, 3)
        flags = {}

        def flag(pattern, radius, k):
            if (pattern, radius, k) not in flags:
                dk = table[fl.entries(W, H, k).ravel()] if pattern == "interleaved" else table[k]
                org, raw = ol.sample_rays(ro[:, 0:3], ro[:, 3:6], t, q["normal"], dk, gpu.RT_AO_BIAS_DEFAULT)
                c = np.zeros(W * H, np.int32)
                if hit.any():
                    f = s.query(origins=ol.f32(org[hit]), dirs=ol.f32(raw[hit]), tmax=radius, any_hit=True, use_bvh=bvh, want=("hit",))["hit"]
                    c[hit] = (f != 0).astype(np.int32)
                c = c.reshape(H, W)
                c.setflags(write=False)
                flags[(pattern, radius, k)] = c
            return flags[(pattern, radius, k)]

        def count(pattern, radius, ks):
            return sum((flag(pattern, radius, k) for k in ks), np.zeros((H, W), np.int32))

        ref = {"live": hit.reshape(H, W), "p": p, "n": n, "cam": hl.camera(s.export("camera")), "count": count}
        for v in (ref["live"], p, n):
            v.setflags(write=False)
        cache[(name, pose)] = ref
        return ref
    return get


def prev_of(frame, count, weight=None):
    return {"p": frame["p"], "n": frame["n"], "live": frame["live"], "count": count,
            "weight": np.zeros_like(count) if weight is None else weight}


def check_outputs(fr, occluded, weight, n, tag):
    vis = hl.resolve(occluded, weight, n)
    assert np.array_equal(fr["occluded"], occluded), (tag, int((fr["occluded"] != occluded).sum()))
    assert np.array_equal(bits(fr["visibility"]), bits(vis)), (tag, int((bits(fr["visibility"]) != bits(vis)).sum()))
    assert np.array_equal(fr["rgba"], ol.grey(vis)), tag


# ---- 1. no move: history on is history off ------------------------------------------------------------
@pytest.mark.parametrize("filt", (False, True))
@pytest.mark.parametrize("pattern", ("shared", "interleaved"))
def test_no_move_is_history_off(gpu, tmp_path, pattern, filt):
    for name in ("stress_odd", "rotated12"):
        off, bvh = make(gpu, name, tmp_path, pattern=pattern, history=False)
        on, _ = make(gpu, name, tmp_path, pattern=pattern)
        for s in (off, on):
            s.set_occlusion_filter(filt)
        for n in (3, 2):
            a = off.occlusion(samples=n, radius=2.0, use_bvh=bvh, want=WANT)
            b = on.occlusion(samples=n, radius=2.0, use_bvh=bvh, want=WANT)
            assert a["n"] == b["n"]
            for k in WANT:
                assert a[k].tobytes() == b[k].tobytes(), (name, pattern, filt, n, k)
        h = on.occlusion_history
        assert (h["moves"], h["cursor"], h["n"], h["weighted"]) == (0, 5, 5, False) and on.occlusion_info[3] == 0
        assert (on._occlusion_history_weights() == 0).all()
        assert off.occlusion_history["cursor"] == 0 and not off.occlusion_history["on"]


# ---- 2. a move to the same pose ------------------------------------------------------------------------
@pytest.mark.parametrize("name,pattern", (("stress_odd", "shared"), ("rotated12", "interleaved"), ("stress_3x2", "shared")))
def test_zero_move(gpu, frames, tmp_path, name, pattern):
    ref = frames(name, 0)
    s, bvh = make(gpu, name, tmp_path, pattern=pattern)
    static, _ = make(gpu, name, tmp_path, pattern=pattern, history=False)
    (W, H) = CASES[name][0]
    s.occlusion(samples=4, radius=2.0, use_bvh=bvh, want=WANT)
    s.set_camera(*s.camera())                                          # the same pose: still a move
    fr = s.occlusion(samples=3, radius=2.0, use_bvh=bvh, want=WANT)
    whole = static.occlusion(samples=7, radius=2.0, use_bvh=bvh, want=WANT)
    assert np.array_equal(fr["occluded"], whole["occluded"])
    assert np.array_equal(fr["occluded"], ref["count"](pattern, 2.0, range(7)))
    w = s._occlusion_history_weights()
    assert np.array_equal(w, np.where(ref["live"], 4, 0)), int((w != np.where(ref["live"], 4, 0)).sum())
    h = s.occlusion_history
    assert (h["moves"], h["cursor"], h["n"], h["weighted"]) == (1, 7, 3, True)
    assert fr["n"] == 3 and s.occlusion_info == (3, W, H, 0)
    check_outputs(fr, whole["occluded"], w, 3, name)
    assert np.array_equal(bits(fr["visibility"]), bits(whole["visibility"]))       # 1 - c / (4 + 3) = 1 - c / 7


# ---- 3. one real move, and 6. the filter after it ------------------------------------------------------
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name,pattern", (("stress_odd", "shared"), ("rotated12_side", "interleaved"),
                                          ("stress_odd", "interleaved"), ("rotated12_side", "shared")))
def test_one_real_move(gpu, frames, tmp_path, name, pattern, radius):
    A, B = frames(name, 0), frames(name, 1)
    count_a = A["count"](pattern, radius, range(4))
    c_h, n_h, census = hl.move(B, prev_of(A, count_a), A["cam"], 4, 32)
    print(name, pattern, radius, census)
    # the pose exercises every verdict of the reprojection
    assert 4 * census["accepted"] >= census["live"] > 0, census
    assert census["off_canvas"] > 0 and census["not_live"] > 0 and census["normal"] > 0 and census["plane"] > 0, census
    assert (n_h[n_h != 0] == 4).all() and 0 < c_h.sum()
    occluded = c_h + B["count"](pattern, radius, (4, 5))
    s, bvh = make(gpu, name, tmp_path, pattern=pattern)
    (W, H) = CASES[name][0]
    fa = s.occlusion(samples=4, radius=radius, use_bvh=bvh, want=WANT)
    assert np.array_equal(fa["occluded"], count_a)
    s.set_camera(*POSES[name][1])
    fr = s.occlusion(samples=2, radius=radius, use_bvh=bvh, want=WANT)
    assert fr["n"] == 2 and s.occlusion_info == (2, W, H, 0)
    h = s.occlusion_history
    assert (h["moves"], h["cursor"], h["n"], h["weighted"]) == (1, 6, 2, True)
    w = s._occlusion_history_weights()
    assert np.array_equal(w, n_h), (name, int((w != n_h).sum()))
    check_outputs(fr, occluded, n_h, 2, (name, pattern, radius))
    assert (fr["visibility"][~B["live"]] == 1).all() and (w[~B["live"]] == 0).all()
    # one output alone, and the next call adds to the moved accumulation
    more = s.occlusion(samples=1, radius=radius, use_bvh=bvh, want=("visibility",))
    assert more["n"] == 3 and s.occlusion_history["cursor"] == 7
    occ3 = occluded + B["count"](pattern, radius, (6,))
    assert np.array_equal(bits(more["visibility"]), bits(hl.resolve(occ3, n_h, 3)))
    # the filtered resolve with per-tap denominators, on the same accumulation
    s.set_occlusion_filter(True)
    ff = s.occlusion(samples=1, radius=radius, use_bvh=bvh, want=WANT)
    occ4 = occ3 + B["count"](pattern, radius, (7,))
    vis, S, N = hl.filtered(B["p"], B["n"], B["live"], occ4, n_h, 4)
    assert ff["n"] == 4 and np.array_equal(ff["occluded"], occ4)
    assert np.array_equal(bits(ff["visibility"]), bits(vis)), int((bits(ff["visibility"]) != bits(vis)).sum())
    assert np.array_equal(ff["rgba"], ol.grey(vis))
    assert not np.array_equal(bits(vis), bits(hl.resolve(occ4, n_h, 4)))            # the filter changes the frame
    assert not np.array_equal(bits(vis), bits(fl.filtered(B["p"], B["n"], B["live"], occ4, 4)[0]))   # and so do the weights


# ---- 4. a chain of moves with a small cap --------------------------------------------------------------
@pytest.mark.parametrize("name,pattern", (("stress_odd", "interleaved"), ("rotated12_side", "shared")))
def test_chain_with_a_cap(gpu, frames, tmp_path, name, pattern):
    A, B, C = (frames(name, k) for k in range(3))
    s, bvh = make(gpu, name, tmp_path, pattern=pattern, max_history=3)
    s.occlusion(samples=8, radius=2.0, use_bvh=bvh, want=WANT)
    count_a = A["count"](pattern, 2.0, range(8))
    cb, wb, _ = hl.move(B, prev_of(A, count_a), A["cam"], 8, 3)
    assert set(np.unique(wb)) == {0, 3} and (cb <= wb).all()          # 8 > 3: scaled, (3 c + 4) / 8
    s.set_camera(*POSES[name][1])
    fb = s.occlusion(samples=2, radius=2.0, use_bvh=bvh, want=WANT)
    occ_b = cb + B["count"](pattern, 2.0, (8, 9))
    check_outputs(fb, occ_b, wb, 2, (name, "B"))
    assert np.array_equal(s._occlusion_history_weights(), wb)
    cc, wc, _ = hl.move(C, prev_of(B, occ_b, wb), B["cam"], 2, 3)     # T = 3 + 2 > 3 where B had history, T = 2 elsewhere
    assert set(np.unique(wc)) == {0, 2, 3}
    s.set_camera(*POSES[name][2])
    fc = s.occlusion(samples=2, radius=2.0, use_bvh=bvh, want=WANT)
    occ_c = cc + C["count"](pattern, 2.0, (10, 11))
    check_outputs(fc, occ_c, wc, 2, (name, "C"))
    assert np.array_equal(s._occlusion_history_weights(), wc)
    h = s.occlusion_history
    assert (h["moves"], h["cursor"], h["n"], h["max_history"]) == (2, 12, 2, 3) and s.occlusion_info[3] == 0


# ---- 5. the table's wrap -------------------------------------------------------------------------------
def test_wrap(gpu, frames, tmp_path):
    name, pattern = "stress_odd", "interleaved"
    A, B = frames(name, 0), frames(name, 1)
    s, bvh = make(gpu, name, tmp_path, pattern=pattern)
    fa = s.occlusion(samples=62, radius=2.0, use_bvh=bvh, want=WANT)
    count_a = A["count"](pattern, 2.0, range(62))
    assert np.array_equal(fa["occluded"], count_a)
    s.set_camera(*POSES[name][1])
    with pytest.raises(gpu.RtError) as e:                              # the samples since the move count, not the cursor
        s.occlusion(samples=65, radius=2.0, use_bvh=bvh, want=WANT)
    assert e.value.code == gpu.RT_ERR_LIMIT and s.occlusion_history["cursor"] == 62
    fr = s.occlusion(samples=5, radius=2.0, use_bvh=bvh, want=WANT)    # sample indices 62, 63, 0, 1, 2
    c_h, n_h, _ = hl.move(B, prev_of(A, count_a), A["cam"], 62, 32)
    assert set(np.unique(n_h)) == {0, 32}
    occluded = c_h + B["count"](pattern, 2.0, (62, 63, 0, 1, 2))
    check_outputs(fr, occluded, n_h, 5, "wrap")
    h = s.occlusion_history
    assert (h["moves"], h["cursor"], h["n"]) == (1, 67, 5)
    with pytest.raises(gpu.RtError) as e:                              # 5 + 60 > 64
        s.occlusion(samples=60, radius=2.0, use_bvh=bvh, want=WANT)
    assert e.value.code == gpu.RT_ERR_LIMIT and s.occlusion_history["cursor"] == 67
    more = s.occlusion(samples=59, radius=2.0, use_bvh=bvh, want=WANT)  # indices 3 .. 61: the pattern is full again
    assert more["n"] == 64 and s.occlusion_history["cursor"] == 126
    check_outputs(more, occluded + B["count"](pattern, 2.0, range(3, 62)), n_h, 64, "wrap, full")


# ---- 7. what drops the history -------------------------------------------------------------------------
def _moved(gpu, tmp_path, name="stress_odd", **kw):
    s, bvh = make(gpu, name, tmp_path, **kw)
    s.occlusion(samples=2, radius=2.0)
    s.set_camera(*POSES[name][1])
    s.occlusion(samples=1, radius=2.0)
    h = s.occlusion_history
    assert (h["moves"], h["cursor"], h["n"], h["weighted"]) == (1, 3, 1, True) and s.occlusion_info[3] == 0
    assert (s._occlusion_history_weights() == 2).any()
    return s


@pytest.mark.parametrize("what", ("instance", "radius", "bias", "restart", "pattern", "max_history", "reset"))
def test_drops(gpu, tmp_path, what):
    s = _moved(gpu, tmp_path)
    fresh, _ = make(gpu, "stress_odd", tmp_path, pose=1, history=False)
    kw = {"samples": 2, "radius": 2.0, "want": WANT}
    if what == "instance":
        inst = s.export("instances")
        for x in (s, fresh):
            x.set_trans(0, pos=inst[0, 4:7] + np.array([0, 3.0, 0], np.float32))
    elif what == "radius":
        kw["radius"] = 1.0
    elif what == "bias":
        kw["bias"] = 0.05
    elif what == "pattern":
        for x in (s, fresh):
            x.set_occlusion_pattern("interleaved")
        assert s.occlusion_history["cursor"] == 0 and s.occlusion_info[3] == 1
    elif what == "max_history":
        s.set_occlusion_history(True, max_history=16)
        assert s.occlusion_history["cursor"] == 0 and s.occlusion_info[3] == 1
    elif what == "reset":
        s.occlusion_reset()
        assert s.occlusion_history["cursor"] == 0 and not s.occlusion_history["weighted"]
    fr = s.occlusion(restart=(what == "restart"), **kw)
    want = fresh.occlusion(**kw)
    h = s.occlusion_history
    assert (h["moves"], h["cursor"], h["n"], h["weighted"]) == (1, 2, 2, False), (what, h)
    assert s.occlusion_info[3] == 1 and fr["n"] == 2
    assert (s._occlusion_history_weights() == 0).all()
    for k in WANT:                                                     # a restart: the scene that starts at this pose
        assert fr[k].tobytes() == want[k].tobytes(), (what, k)


def test_thresholds_alone_drop_nothing(gpu, frames, tmp_path):
    name = "stress_odd"
    s = _moved(gpu, tmp_path)
    before = s._occlusion_history_weights()
    s.set_occlusion_history(True, normal_min=-1.0, plane_tol=1e30)    # applies at the next move
    h = s.occlusion_history
    assert (h["moves"], h["cursor"], h["n"], h["weighted"]) == (1, 3, 1, True) and s.occlusion_info[3] == 0
    assert s.occlusion(samples=1, radius=2.0)["n"] == 2
    assert np.array_equal(s._occlusion_history_weights(), before)
    s.set_camera(*POSES[name][2])
    assert s.occlusion(samples=1, radius=2.0)["n"] == 1
    B, C = frames(name, 1), frames(name, 2)
    # with everything accepted a pixel has history exactly when its source is on the canvas and live
    _, on, qx, qy, _, _ = hl.reproject(C["p"], B["cam"])
    w = s._occlusion_history_weights()
    assert np.array_equal(w != 0, C["live"] & on & B["live"][qy, qx])
    assert s.occlusion_history["moves"] == 2 and s.occlusion_info[3] == 0


# ---- 8. the frame state, host and device pointers ------------------------------------------------------
def test_render_in_between_and_the_frame_state(gpu, tmp_path):
    a, _ = make(gpu, "stress_odd", tmp_path)
    b, _ = make(gpu, "stress_odd", tmp_path)
    plain, _ = make(gpu, "stress_odd", tmp_path, history=False)
    want = ("rgba", "radiance", "hit_inst", "hit_tri")
    for pose in (0, 1, 2):
        for s in (a, b, plain):
            s.set_camera(*POSES["stress_odd"][pose])
        ra = a.render(spp=4, want=want, stats=False)
        rp = plain.render(spp=4, want=want, stats=False)
        assert all(np.array_equal(bits(ra[k]), bits(rp[k])) for k in want) and a.last_trace() == plain.last_trace()
        trace, hist = a.last_trace(), a._history_info()
        fa = a.occlusion(samples=2, radius=2.0, rebuild_bvh=False, want=WANT)    # a moving call for pose > 0
        assert a._history_info() == hist and a.last_trace() == trace
        fb = b.occlusion(samples=2, radius=2.0, want=WANT)
        assert fa["n"] == fb["n"] == 2 and a.occlusion_history["moves"] == pose
        for k in WANT:
            assert fa[k].tobytes() == fb[k].tobytes(), (pose, k)
    ra = a.render(spp=4, want=want, stats=False)
    assert all(np.array_equal(bits(ra[k]), bits(rp[k])) for k in want)


@pytest.mark.parametrize("filt", (False, True))
def test_host_and_device_pointers_agree(gpu, tmp_path, filt):
    import torch
    a, _ = make(gpu, "stress_odd", tmp_path, pattern="interleaved")
    b, _ = make(gpu, "stress_odd", tmp_path, pattern="interleaved")
    (W, H) = CASES["stress_odd"][0]
    vis = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    occ = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    rgba = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    for pose in (0, 1, 2):
        for s in (a, b):
            s.set_occlusion_filter(filt)
            s.set_camera(*POSES["stress_odd"][pose])
        host = a.occlusion(samples=2, radius=2.0, want=WANT)
        got = b.occlusion_device(samples=2, radius=2.0, visibility_ptr=vis.data_ptr(), occluded_ptr=occ.data_ptr(), rgba_ptr=rgba.data_ptr())
        assert got == host["n"] == 2 and b.occlusion_history["moves"] == pose
        assert np.array_equal(bits(vis.cpu().numpy()), bits(host["visibility"]))
        assert np.array_equal(occ.cpu().numpy(), host["occluded"])
        assert np.array_equal(rgba.cpu().numpy().view(np.uint32), host["rgba"])
    vis.fill_(-5.0)
    assert b.occlusion_device(radius=2.0, rgba_ptr=rgba.data_ptr()) == 3          # one output alone
    assert (vis == -5.0).all()
    assert np.array_equal(rgba.cpu().numpy().view(np.uint32), a.occlusion(radius=2.0, want=("rgba",))["rgba"])


# ---- 9. a split scene ----------------------------------------------------------------------------------
def test_split_scene_is_refused(gpu):
    s = gpu.Scene.load_json(scene_path("world8"), 64, 48)
    s.set_occlusion_history(True)
    assert s.occlusion()["n"] == 1
    s.set_devices([0], 2)
    s.set_occlusion_history(True, max_history=8)                       # the setting is host state
    with pytest.raises(gpu.RtError) as e:
        s.occlusion()
    assert e.value.code == gpu.RT_ERR_STATE
    s.set_devices([0], 1)
    assert s.occlusion()["n"] == 1 and s.occlusion_history["max_history"] == 8


# ---- 10. CLI -------------------------------------------------------------------------------------------
def test_cli_history(gpu, tmp_path):
    W, H = 96, 64
    cli = [CLI, "-c", scene_path("world8_stress"), "--width", str(W), "--height", str(H)]
    out = str(tmp_path / "f.ppm")
    r = subprocess.run(cli + ["--occlusion", "2", "--history", "--frames", "3", "--pan", "0.1", "--out", out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("Occlusion: 2 samples") == 3
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("History:")] == \
        ["History: moves 0 cursor 2", "History: moves 1 cursor 4", "History: moves 2 cursor 6"]
    s = gpu.Scene.load_json(scene_path("world8_stress"), W, H)
    s.set_occlusion_history(True)
    for call in range(3):
        if call:
            s.translate_camera((0.1, 0.0, 0.0))
        rgba = s.occlusion(samples=2, want=("rgba",))["rgba"]
    assert s.occlusion_history["moves"] == 2
    want = np.stack([(rgba >> 24) & 255, (rgba >> 16) & 255, (rgba >> 8) & 255], axis=-1).astype(np.uint8)
    assert np.array_equal(base._ppm_rgb(out, W, H), want)
    plain = gpu.Scene.load_json(scene_path("world8_stress"), W, H)
    for call in range(3):
        if call:
            plain.translate_camera((0.1, 0.0, 0.0))
        off = plain.occlusion(samples=2, want=("rgba",))["rgba"]
    assert not np.array_equal(off, rgba) and len(np.unique(rgba)) > len(np.unique(off))   # more grey levels than 2 samples have
    # --history 8: the cap; --history or --pan without what they belong to: usage errors
    r = subprocess.run(cli + ["--occlusion", "2", "--history", "8", "--frames", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "History: moves 1 cursor 4" in r.stdout
    assert subprocess.run(cli + ["--history"], capture_output=True, text=True, timeout=120).returncode == 2
    assert subprocess.run(cli + ["--occlusion", "2", "--pan", "0.1"], capture_output=True, text=True, timeout=120).returncode == 2
    assert subprocess.run(cli + ["--occlusion", "2", "--history", "0"], capture_output=True, text=True, timeout=120).returncode == 1
