"""trace_sample's integrator against the oracle where its rules can be told apart: the scenes of
tests/integrator_cases.py (several overlapping refractive media of different eta and Kt, eta below
and equal to 1, a Kt channel of 0, of 1 and above 1, total internal reflection, a point light
inside the field), at every depth rt_env_set admits -- 0 and 1 in the NS 2 bucket, 5 to 9 with
the NS 9 kernels' SavedFrame stack full.  tests/test_integrator_host.py proves on the oracle alone
(the census) that these frames are decided by: the Isect shared by a sample, eta from the
frame's last_mat and time^Kt from the material hit on the way out where the two differ, hit point
and normal of a frame resumed from the stack, in_obj inherited by reflection children, TIR on
entering and on leaving, shadow segments continued through transmissive hits with max_t reduced.

Every frame is 48 x 32 and held to the project bar (twin.assert_frames_equal: hit ids equal,
radiance within 1e-5 relative, RGBA8 bytes equal, max_pm1 = 0), and every launch's kernel is
asserted through Scene.last_trace()."""
import numpy as np
import pytest

import integrator_cases as ic
import kernel_recipes as kr
from test_integrator_host import VARIANTS, variant_key
from twin import Twin, assert_frames_equal, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
STAT_KEYS = ("rays", "nodes", "leaves", "tri_tests")
W, H = ic.SIZE


@pytest.fixture(scope="module")
def twins(gpu, oracle):
    """(product scene, oracle scene) per scene name, built once by the same builder calls."""
    cache = {}

    def get(name):
        if name not in cache:
            t = Twin(gpu, oracle)
            ic.build(t, name)
            cache[name] = (t.gpu, t.orc)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def at(twins, oracle):
    """Both scenes of `name` at a pose and depth, and the oracle's frame there (rendered once per
    (scene, pose, depth, spp, use_bvh), shared, never written to)."""
    cache = {}

    def get(name, pose, depth, spp=1, use_bvh=True):
        s, o = twins(name)
        p, q = ic.poses(name)[pose]
        for scene in (s, o):
            scene.set_camera(p, q)
            scene.set_env(depth=depth)
        k = (name, pose, depth, spp, bool(use_bvh))
        if k not in cache:
            cache[k] = orc_render(oracle, o, spp=spp, use_bvh=int(use_bvh))
        return s, o, cache[k]
    return get


def _launched(s, label, depth, ctx):
    lt = s.last_trace()
    assert (lt["ns_bucket"], lt["lds"], lt["mode"]) == variant_key(label, depth), (ctx, label, lt)
    assert lt["ftree"] == 1, (ctx, lt)
    return lt


def _bits_equal(a, b, ctx):
    for k in WANT:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (ctx, k)


def _stats(fr):
    return tuple(fr["stats"][k] for k in STAT_KEYS)


@pytest.mark.parametrize("pose", list(ic.MEDIA_POSES))
@pytest.mark.parametrize("depth", range(10))
def test_depth_sweep(at, monkeypatch, depth, pose):
    """media, every depth and pose, the fast frame: NS 2 up to depth 2, NS 9 from depth 3."""
    monkeypatch.delenv("RT_NO_PART", raising=False)
    s, _, of = at("media", pose, depth)
    ctx = ("media", pose, depth)
    fast = s.render(spp=1, want=WANT, stats=False)
    lt = _launched(s, "fast", depth, ctx)
    assert lt["ns_bucket"] == (2 if depth <= 2 else 9), (ctx, lt)
    assert_frames_equal(fast, of, ctx=ctx, max_pm1=0)


@pytest.mark.parametrize("pose", list(ic.MEDIA_POSES))
@pytest.mark.parametrize("depth", (0, 1, 5, 9))
def test_other_kernels_of_the_scene(at, monkeypatch, depth, pose):
    """The counted frame (the oracle's four work counters; the fast frame's bits), brute force fast and
    counted, 4 spp, and RT_NO_PART: each launch on the kernel tests/test_integrator_host.py derives for it --
    four different kernels; 4 spp and RT_NO_PART stay on the fast frame's (a scene this small parks whole)."""
    monkeypatch.delenv("RT_NO_PART", raising=False)
    s, _, of = at("media", pose, depth)
    ctx = ("media", pose, depth)
    fast = s.render(spp=1, want=WANT, stats=False)
    seen = {"fast": _launched(s, "fast", depth, ctx)}
    counted = s.render(spp=1, want=WANT, stats=True)
    seen["counted"] = _launched(s, "counted", depth, ctx)
    assert_frames_equal(counted, of, ctx=ctx + ("counted",), max_pm1=0)
    assert _stats(counted) == tuple(int(x) for x in of["stats"]), ctx
    _bits_equal(fast, counted, ctx)

    _, _, ob = at("media", pose, depth, use_bvh=False)
    brute = s.render(spp=1, want=WANT, stats=False, use_bvh=False)
    seen["brute"] = _launched(s, "brute", depth, ctx)
    assert_frames_equal(brute, ob, ctx=ctx + ("brute",), max_pm1=0)
    brute_counted = s.render(spp=1, want=WANT, stats=True, use_bvh=False)
    _launched(s, "brute counted", depth, ctx)
    assert_frames_equal(brute_counted, ob, ctx=ctx + ("brute counted",), max_pm1=0)
    assert _stats(brute_counted) == tuple(int(x) for x in ob["stats"]), ctx
    _bits_equal(brute, brute_counted, ctx)

    _, _, o4 = at("media", pose, depth, spp=4)
    f4 = s.render(spp=4, want=WANT, stats=False)
    _launched(s, "spp4", depth, ctx)
    assert_frames_equal(f4, o4, ctx=ctx + ("spp4",), max_pm1=0)

    monkeypatch.setenv("RT_NO_PART", "1")                      # choose_trace_variant reads it at every launch
    fn = s.render(spp=1, want=WANT, stats=False)
    _launched(s, "no_part", depth, ctx)
    _bits_equal(fn, fast, ctx + ("no_part",))
    assert_frames_equal(fn, of, ctx=ctx + ("no_part",), max_pm1=0)

    keys = {k: (v["ns_bucket"], v["lds"], v["mode"]) for k, v in seen.items()}
    assert len(set(keys.values())) == 3, keys                  # fast, counted and brute force: three kernels
    assert VARIANTS["spp4"][1] == VARIANTS["no_part"][1] == VARIANTS["fast"][1]


@pytest.mark.parametrize("name", ("media_kt_gt1", "two_slabs"))
@pytest.mark.parametrize("depth", (1, 4, 9))
def test_other_scenes(at, monkeypatch, name, depth):
    """A Kt channel above 1 (no unlit skip on a refractive scene) and the two-slab control, every pose:
    fast and counted."""
    monkeypatch.delenv("RT_NO_PART", raising=False)
    for pose in ic.poses(name):
        s, _, of = at(name, pose, depth)
        ctx = (name, pose, depth)
        fast = s.render(spp=1, want=WANT, stats=False)
        _launched(s, "fast", depth, ctx)
        assert_frames_equal(fast, of, ctx=ctx, max_pm1=0)
        counted = s.render(spp=1, want=WANT, stats=True)
        _launched(s, "counted", depth, ctx)
        assert_frames_equal(counted, of, ctx=ctx + ("counted",), max_pm1=0)
        assert _stats(counted) == tuple(int(x) for x in of["stats"]), ctx
        _bits_equal(fast, counted, ctx)


def _tir_pop(log):
    """A refraction event that no ray follows for that frame: the next event is not "shooting a ray"
    (the refracted ray's NORMAL step) -- total internal reflection popped the frame (scene.cu:149-184)."""
    return any(e == "preparing to shoot a refraction ray" and (i + 1 == len(log) or log[i + 1] != "shooting a ray")
               for i, e in enumerate(log))


def test_event_logs(at):
    """rt_debug_cast's event log, line for line, for pixels picked on the oracle alone at depth 9: the three
    longest logs of the frame and three whose log has a total internal reflection."""
    s, o, _ = at("media", "above", 9)
    logs = {(x, y): o.debug_cast(x, y) for y in range(H) for x in range(W)}
    longest = sorted(logs, key=lambda p: (-len(logs[p]), p))[:3]
    tir = [p for p in sorted(logs, key=lambda p: (p[1], p[0])) if _tir_pop(logs[p]) and p not in longest][:3]
    assert len(tir) == 3 and len(logs[longest[2]]) >= 100, (tir, [len(logs[p]) for p in longest])
    for x, y in longest + tir:
        g = s.debug_cast(x, y)
        assert g == logs[x, y], ((x, y), len(g), len(logs[x, y]),
                                 next((i for i, (a, b) in enumerate(zip(g, logs[x, y])) if a != b), None))


@pytest.mark.parametrize("pose", list(ic.MEDIA_POSES))
def test_frame_work_at_depth_9(gpu, at, monkeypatch, pose):
    """rt_frame_work takes the scene at depth 9 (the parked axis kernel's profiling variant, NS 9): its frame
    is the fast frame's and the oracle's, its counters keep test_gpu_frame_work.py's identities."""
    monkeypatch.delenv("RT_NO_PART", raising=False)
    s, _, of = at("media", pose, 9)
    ctx = ("media", pose, 9, "frame_work")
    w, rgba = s.frame_work(spp=1, want_rgba=True)
    lt = _launched(s, "prof", 9, ctx)
    assert not lt["sky"], lt
    fast = s.render(spp=1, want=WANT, stats=False)
    _launched(s, "fast", 9, ctx)
    assert np.array_equal(rgba, fast["rgba"]), ctx
    assert_frames_equal({"rgba": rgba}, of, keys=("rgba",), ctx=ctx, max_pm1=0)
    assert w["lanes_primary"] == W * H, (ctx, w)
    assert w["queries"] == w["lanes_primary"] + w["lanes_secondary"] + w["lanes_shadow"], (ctx, w)
    assert w["lanes_shadow"] > 0 and w["lanes_secondary"] > 0, (ctx, w)
    assert sum(w["hist_wave_queries"]) == w["live_wave_queries"], (ctx, w)
    assert 0 < w["live_wave_queries"] <= w["wave_queries"], (ctx, w)
    assert w["live_wave_queries"] <= w["live_lanes"] <= 64 * w["live_wave_queries"], (ctx, w)
    assert w["lanes_secondary"] + w["lanes_shadow"] <= w["live_lanes"] <= w["queries"], (ctx, w)
    assert w["queries"] - w["live_lanes"] <= w["lanes_primary"], (ctx, w)
    assert sum(w["hist_leaf_visits"]) == w["leaf_visits"], (ctx, w)
    assert sum(w["hist_pair_steps"]) <= w["pair_steps"], (ctx, w)
    assert w["leaf_visits"] <= w["leaf_lanes"] <= 64 * w["leaf_visits"], (ctx, w)
    assert w["wave_queries"] <= w["queries"] + w["lanes_unlit"], (ctx, w)
    # the fast kernel only skips (the unlit skip): the oracle's rays are the reference's cast_ray calls
    assert w["queries"] <= int(of["stats"][0]), (ctx, w)
