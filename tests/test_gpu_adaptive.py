"""Adaptive refinement on the GPU (rt_accumulate_set_adaptive): after sample 0 only the tiles
with an edge take further samples.  The device's mask against the numpy restatement of the
criterion (adaptive_cases.need_mask) and the oracle's; after n samples the needed tiles' pixels are
render(spp = n)'s and the others render(spp = 1)'s, RGBA8 bytes and radiance bits, and the composed
frame is the oracle's; a refinement pass writes no pixel of an unneeded tile into the pass buffer
(it traces the needed tiles only); an all-sky frame launches nothing; batching, restarts, renders
in between, the launch record and the CLI.  Cases: tests/adaptive_cases.py.  The oracle's frames
are rendered once per (case, n) and shared, never written to.  The host twin is
tests/test_adaptive_host.py."""
import os
import subprocess

import numpy as np
import pytest

import adaptive_cases as ac
from conftest import ROOT, scene_path
from twin import assert_frames_equal, mirror_camera, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
CLI = os.path.join(ROOT, "gpu-ray-tracer_amd", "rtracer")
N_PREFIX = 5
PATTERN = 0x7fc00123                                               # a NaN no kernel writes


@pytest.fixture(scope="module")
def frames(gpu, oracle):
    """The oracle's frame of `case` in its initial state at spp = n."""
    cache, scenes = {}, {}

    def get(case, n):
        if (case, n) not in cache:
            if case not in scenes:
                scenes[case] = ac.make(None, oracle, case)[1]
            fr = orc_render(oracle, scenes[case], spp=n, use_bvh=int(ac.CASES[case][3]))
            for v in fr.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            cache[case, n] = fr
        return cache[case, n]
    return get


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, keys=WANT):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def adaptive(gpu, case, threshold=ac.THRESHOLD):
    s, _, bvh = ac.make(gpu, None, case)
    s.set_accumulate_adaptive(True, float(threshold))
    return s, bvh


def check_frame(s, fr, need, case, n, bvh, frames, ctx):
    """fr, the adaptive frame of n samples: the needed tiles' pixels are render(spp=n)'s, the
    others render(spp=1)'s, bit for bit; composed the same way, the oracle's frames; sample 0's hit ids."""
    w, h = ac.CASES[case][1:3]
    own_n = s.render(spp=n, use_bvh=bvh, want=WANT, stats=False)
    own_1 = s.render(spp=1, use_bvh=bvh, want=WANT, stats=False)
    m = ac.pixel_mask(need, w, h)
    for k in ("rgba", "radiance"):
        g, a, b = bits(fr[k]), bits(own_n[k]), bits(own_1[k])
        assert np.array_equal(g[m], a[m]), (ctx, case, n, k, "needed tiles", int((g[m] != a[m]).sum()))
        assert np.array_equal(g[~m], b[~m]), (ctx, case, n, k, "other tiles", int((g[~m] != b[~m]).sum()))
    for k in ("hit_inst", "hit_tri"):
        assert np.array_equal(fr[k], own_1[k]), (ctx, case, n, k)
    want = ac.compose(need, frames(case, n), frames(case, 1))
    assert_frames_equal(fr, want, ctx=(ctx, case, n), max_pm1=0)


@pytest.mark.parametrize("case,threshold", [(c, ac.THRESHOLD) for c in ac.CASES] + [("stress_odd", 0.0), ("stress_odd", 0.125)])
def test_mask(gpu, frames, case, threshold):
    s, bvh = adaptive(gpu, case, threshold)
    w, h = ac.CASES[case][1:3]
    assert s.accumulate_tiles()["need"] is None
    fr = s.accumulate(use_bvh=bvh, want=WANT)
    assert fr["n"] == 1
    t = s.accumulate_tiles()
    want = ac.need_mask(fr["radiance"], threshold)
    assert t["mode"] == 1 and t["tile"] == ac.TILE and t["need"].shape == want.shape
    assert np.array_equal(t["need"], want), (case, int((t["need"] != want).sum()))
    assert t["needed"] == int(want.sum()) and t["traced"] == ac.n_tiles(w, h)
    assert_frames_equal(fr, frames(case, 1), ctx=("adaptive n=1", case), max_pm1=0)
    if threshold == ac.THRESHOLD and case in ac.MARGIN_CASES:
        assert np.array_equal(t["need"], ac.need_mask(frames(case, 1)["radiance"], threshold)), case
        assert t["needed"] == ac.NEEDED[case]
    print("needed tiles: %s thr %.4f: %d of %d" % (case, threshold, t["needed"], want.size))


def test_threshold_reaches_the_kernel(gpu, frames):
    """`stress` at 0.9 against 8/255: another mask (14 tiles against 22 on the oracle's frame, whose
    nearest contrast lies 0.11 relative from 0.9 and 0.29 from 8/255), each the restatement's."""
    masks = {}
    for thr in (ac.THRESHOLD, 0.9):
        s, bvh = adaptive(gpu, "stress", thr)
        fr = s.accumulate(use_bvh=bvh, want=WANT)
        t = s.accumulate_tiles()
        assert t["threshold"] == float(np.float32(thr))
        assert np.array_equal(t["need"], ac.need_mask(fr["radiance"], thr)), thr
        assert np.array_equal(t["need"], ac.need_mask(frames("stress", 1)["radiance"], thr)), thr
        masks[float(thr)] = t["need"]
    lo, hi = masks[float(ac.THRESHOLD)], masks[0.9]
    assert lo.sum() == ac.NEEDED["stress"] and hi.sum() == 14
    assert not np.array_equal(lo, hi) and not (hi & ~lo).any()     # a higher threshold flags a subset


@pytest.mark.parametrize("case", list(ac.CASES))
def test_prefix_parity_adaptive(gpu, frames, case):
    s, bvh = adaptive(gpu, case)
    for n in range(1, N_PREFIX + 1):
        fr = s.accumulate(use_bvh=bvh, want=WANT)
        assert fr["n"] == n and s.accumulated[0] == n
        need = s.accumulate_tiles()["need"]
        check_frame(s, fr, need, case, n, bvh, frames, "prefix")
    assert s.accumulated == (N_PREFIX, ac.CASES[case][1], ac.CASES[case][2], 0)


@pytest.mark.parametrize("case", ("stress", "world1_brute", "media", "one_leaf"))
def test_only_needed_tiles_are_traced(gpu, frames, case):
    s, bvh = adaptive(gpu, case)
    w, h = ac.CASES[case][1:3]
    s.accumulate(use_bvh=bvh)
    need = s.accumulate_tiles()["need"]
    assert 0 < need.sum() < need.size
    s._accumulate_pass_fill(PATTERN)
    assert (bits(s._accumulate_pass_read()) == PATTERN).all()
    fr = s.accumulate(use_bvh=bvh, want=WANT)
    assert fr["n"] == 2
    t = s.accumulate_tiles()
    p = bits(s._accumulate_pass_read())
    m = ac.pixel_mask(need, w, h)
    assert np.isfinite(p.view(np.float32)[m]).all()                # the needed tiles' canvas pixels were traced
    if case == "one_leaf":                                         # the fallback: every tile traced, the fold masked
        assert t["traced"] == need.size
        assert np.isfinite(p.view(np.float32)).all()
    else:
        assert t["traced"] == t["needed"] == int(need.sum())
        assert (p[~m] == PATTERN).all(), (case, int((p[~m] != PATTERN).sum()))
    check_frame(s, fr, need, case, 2, bvh, frames, "after pass_fill")   # the fold read nothing it should not


def test_sky(gpu, frames):
    s, bvh = adaptive(gpu, "sky")
    one = s.accumulate(want=WANT)
    t = s.accumulate_tiles()
    assert t["needed"] == 0 and not t["need"].any()
    s._accumulate_pass_fill(PATTERN)
    fr = s.accumulate(samples=4, want=WANT)
    assert fr["n"] == 5 and s.accumulated[0] == 5
    assert same_bits(fr, one)
    assert_frames_equal(fr, frames("sky", 1), ctx="sky", max_pm1=0)
    assert (bits(s._accumulate_pass_read()) == PATTERN).all()      # nothing was launched
    assert s.accumulate_tiles()["traced"] == 0


def test_batching(gpu, frames):
    """samples = 5 fresh is five calls of one, bit for bit."""
    a, bvh = adaptive(gpu, "stress_odd")
    b, _ = adaptive(gpu, "stress_odd")
    one = a.accumulate(samples=5, want=WANT)
    for _ in range(5):
        five = b.accumulate(want=WANT)
    assert one["n"] == five["n"] == 5
    assert same_bits(one, five)
    ta, tb = a.accumulate_tiles(), b.accumulate_tiles()
    assert np.array_equal(ta["need"], tb["need"]) and ta["needed"] == tb["needed"] == ta["traced"] == tb["traced"]
    check_frame(a, one, ta["need"], "stress_odd", 5, bvh, frames, "batch of 5")
    # and a batch on top: 5 + 3
    eight = a.accumulate(samples=3, want=WANT)
    check_frame(a, eight, ta["need"], "stress_odd", 8, bvh, frames, "5 + 3")


def test_restarts(gpu, oracle, frames):
    s, o, bvh = ac.make(gpu, oracle, "stress_odd")
    s.set_accumulate_adaptive(True)
    assert s.accumulate(samples=3)["n"] == 3
    need0 = s.accumulate_tiles()["need"]
    # a camera move recomputes the mask
    s.translate_camera([1.5, 0.5, 0.0])                            # (far enough to move an edge into another tile)
    mirror_camera(s, o)
    fr = s.accumulate(want=WANT)
    assert fr["n"] == 1 and s.accumulated[3] == 1
    assert_frames_equal(fr, orc_render(oracle, o, spp=1), ctx="camera", max_pm1=0)
    need1 = s.accumulate_tiles()["need"]
    assert not np.array_equal(need1, need0)
    assert np.array_equal(need1, ac.need_mask(fr["radiance"], ac.THRESHOLD))
    fr = s.accumulate(samples=2, want=WANT)
    o1, o3 = orc_render(oracle, o, spp=1), orc_render(oracle, o, spp=3)
    assert_frames_equal(fr, ac.compose(need1, o3, o1), ctx="camera, 3 samples", max_pm1=0)
    # the same values: nothing happens; another threshold, another mode: a restart each
    s.set_accumulate_adaptive(True)
    assert s.accumulated[0] == 3 and s.accumulated[3] == 1
    s.set_accumulate_adaptive(True, 0.25)
    assert s.accumulated[0] == 0 and s.accumulated[3] == 2 and s.accumulate_tiles()["need"] is None
    fr = s.accumulate(want=WANT)
    t = s.accumulate_tiles()
    assert fr["n"] == 1 and np.array_equal(t["need"], ac.need_mask(fr["radiance"], 0.25)) and t["needed"] <= need1.sum()
    assert s.accumulate()["n"] == 2
    s.set_accumulate_adaptive(False)
    assert s.accumulated[0] == 0 and s.accumulated[3] == 3
    s.set_accumulate_adaptive(False, 0.5)                          # mode 0 ignores the threshold
    assert s.accumulated[3] == 3
    # mode off afterwards: the uniform frame
    fr = s.accumulate(samples=4, want=WANT)
    assert fr["n"] == 4 and s.accumulate_tiles()["need"] is None
    assert_frames_equal(fr, orc_render(oracle, o, spp=4), ctx="mode off", max_pm1=0)
    own = s.render(spp=4, want=WANT, stats=False)
    assert same_bits(fr, own)


def test_render_in_between(gpu, frames):
    """rt_render(spp = 4) and rt_update_scene between refinement calls change neither the lists nor
    the frames; render's own frames and launch record are what they are without the accumulation."""
    a, bvh = adaptive(gpu, "stress")
    b, _ = adaptive(gpu, "stress")
    plain, _, _ = ac.make(gpu, None, "stress")
    r4 = plain.render(spp=4, want=WANT, stats=False)
    k4 = plain.last_trace()
    plain.update_scene()
    canvas = plain.canvas().copy()
    for n in range(1, 5):
        hist = a._history_info()
        fa = a.accumulate(want=WANT)
        now = a._history_info()
        # a refinement pass leaves the slot's scheduling history alone: parity, capacity, slot and key
        # (not [1]: the call's BVH build re-arms the zeroing of the buffer the next frame records into);
        # sample 0 is an ordinary launch and records history
        if n > 1:
            assert now[:1] + now[2:] == hist[:1] + hist[2:], (n, hist, now)
        else:
            assert now[0] != hist[0] or now[4:] != hist[4:], (hist, now)
        ra = a.render(spp=4, want=WANT, stats=False)
        assert same_bits(ra, r4) and a.last_trace() == k4, n
        a.update_scene()
        assert np.array_equal(a.canvas(), canvas), n
        fb = b.accumulate(want=WANT)
        assert fa["n"] == fb["n"] == n
        assert same_bits(fa, fb), n
        ta, tb = a.accumulate_tiles(), b.accumulate_tiles()
        assert np.array_equal(ta["need"], tb["need"]) and ta["traced"] == tb["traced"]
    # two more renders are the undisturbed scene's
    for _ in range(2):
        assert same_bits(a.render(spp=4, want=WANT, stats=False), plain.render(spp=4, want=WANT, stats=False))
    check_frame(a, fa, ta["need"], "stress", 4, bvh, frames, "renders in between")


@pytest.mark.parametrize("case", ("stress", "world1_brute", "media", "one_leaf"))
def test_launch_record(gpu, case):
    """The refinement passes' launches are the spp = 1 kernel render(spp=1) uses on that scene."""
    s, bvh = adaptive(gpu, case)
    s.render(spp=1, use_bvh=bvh, stats=False)
    ref = s.last_trace()
    s.render(spp=16, use_bvh=bvh, stats=True)
    assert s.last_trace() != ref
    s.accumulate(samples=3, use_bvh=bvh)
    assert s.last_trace() == ref, (case, s.last_trace(), ref)


def _ppm(path):
    raw = open(path, "rb").read()
    head = b"P6\n96 64\n255\n"
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], np.uint8).reshape(64, 96, 3)


def test_cli_adaptive(tmp_path, frames):
    a, b, c = (str(tmp_path / n) for n in ("a.ppm", "b.ppm", "c.ppm"))
    base = [CLI, "-c", scene_path("world8_stress"), "--width", "96", "--height", "64"]
    ra = subprocess.run(base + ["--accumulate", "4", "--adaptive", "--out", a], capture_output=True, text=True, timeout=120)
    assert ra.returncode == 0, ra.stderr
    assert "Accumulated 4 samples" in ra.stdout
    assert "Adaptive: %d of 96 tiles refined" % ac.NEEDED["stress"] in ra.stdout, ra.stdout
    for spp, path in ((4, b), (1, c)):
        r = subprocess.run(base + ["--spp", str(spp), "-b", "--out", path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    need = ac.need_mask(frames("stress", 1)["radiance"], ac.THRESHOLD)
    m = ac.pixel_mask(need, 96, 64)
    want = np.where(m[..., None], _ppm(b), _ppm(c))
    assert np.array_equal(_ppm(a), want)
    assert not np.array_equal(_ppm(b), _ppm(c))
    # --adaptive alone is a usage error; an explicit threshold is taken
    assert subprocess.run(base + ["--adaptive"], capture_output=True, text=True, timeout=120).returncode == 2
    rz = subprocess.run(base + ["--accumulate", "2", "--adaptive", "0.9"], capture_output=True, text=True, timeout=120)
    assert rz.returncode == 0 and "Adaptive: " in rz.stdout and "Adaptive: 22 of" not in rz.stdout, rz.stdout
