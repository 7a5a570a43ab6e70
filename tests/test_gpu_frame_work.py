"""rt_frame_work's counters (rt_amd.h: rt_work), which feed the roofline figures of README / DESIGN.

The profiling variant of the fast kernel (M_PROF) counts in trace_sample (rt_kernels.hip), once per
wave query, after closest_hit: the lanes that issued the query by integrator phase (primary,
secondary, shadow), the shadow steps the unlit skip answered without one, and -- over live groups
only (some primary enters the tree's root) and queries with at least one lane -- the query, its
lanes and its child-pair steps and leaf visits by occupancy bucket.  closest_hit itself counts every
query lane (rt_work.queries) and every wave query.  The identities that code implies are asserted
here, on the two-cube scene, the all-opaque cube field world8_stress and the refractive two-cube
scene of tests/kernel_recipes.py, whole frames and a row slice; the frame the profiling run renders
is held to the oracle's."""
import ctypes

import numpy as np
import pytest

import kernel_recipes as kr
from conftest import scene_path
from test_plan_host import fields, plan  # noqa: F401  (the plan_host fixture)
from twin import assert_frames_equal, mirror_camera, orc_render

W, H = 64, 48


@pytest.fixture(scope="module")
def work_scenes(gpu, oracle, tmp_path_factory):
    tmp, cache = tmp_path_factory.mktemp("work"), {}

    def get(name):
        if name not in cache:
            if name == "world8_stress":
                cache[name] = (gpu.Scene.load_json(scene_path(name), W, H), oracle.load(scene_path(name), W, H))
            else:
                cache[name] = kr.build_scene(name, (W, H), gpu, oracle, tmp)
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("spp,row0,row_step", [(1, 0, 1), (8, 0, 1), (3, 0, 1), (8, 1, 3)])
@pytest.mark.parametrize("name,depth", [("two", 3), ("world8_stress", 2), ("two_r", 4)])
def test_frame_work_identities(gpu, oracle, plan, work_scenes, name, depth, spp, row0, row_step):  # noqa: F811
    s, o = work_scenes(name)
    s.set_env(depth=depth)
    o.set_env(depth=depth)
    o.set_textures(False)
    if name != "world8_stress":
        s.set_camera(*kr.second_camera(name, s))
    mirror_camera(s, o)
    rows = len(range(row0, H, row_step))
    w, rgba = s.frame_work(spp=spp, row0=row0, row_step=row_step, compact=True, want_rgba=True)
    lt = s.last_trace()
    assert lt["mode"] == kr.M_PARK | kr.M_FT | kr.M_AXIS | kr.M_PROF and not lt["sky"], lt
    of = orc_render(oracle, o, spp=spp, row0=row0, row_step=row_step)
    orc_rays = int(of["stats"][0])
    opaque = kr.scene_ns(s, depth) == 0
    ctx = (name, spp, row0, row_step, w)

    # the profiling frame is the frame (compact: slice row j is frame row row0 + j row_step)
    assert rgba.shape == (rows, W)
    assert_frames_equal({"rgba": rgba}, {"rgba": of["rgba"][row0::row_step]}, keys=("rgba",), ctx=ctx, max_pm1=0)

    # one primary query per sample: the profiling variant runs without the sky pre-pass
    assert w["lanes_primary"] == rows * W * spp, ctx
    # closest_hit counts the lanes the occupancy code classifies
    assert w["queries"] == w["lanes_primary"] + w["lanes_secondary"] + w["lanes_shadow"], ctx
    assert w["lanes_shadow"] > 0 and w["lanes_secondary"] > 0, ctx   # (every scene here has a reflective cube in view)
    # live groups only
    assert sum(w["hist_wave_queries"]) == w["live_wave_queries"], ctx
    assert 0 < w["live_wave_queries"] <= w["wave_queries"], ctx
    assert w["live_wave_queries"] <= w["live_lanes"] <= 64 * w["live_wave_queries"], ctx
    for b, n in enumerate(w["hist_wave_queries"]):            # bucket b: 8 b + 1 to 8 b + 8 lanes
        assert n == 0 or w["hist_pair_steps"][b] >= n, (ctx, b)      # every query tests the root's pair
    # a group none of whose primaries enters the root issues primaries only, and they visit no leaf
    assert w["lanes_secondary"] + w["lanes_shadow"] <= w["live_lanes"] <= w["queries"], ctx
    assert w["queries"] - w["live_lanes"] <= w["lanes_primary"], ctx
    assert sum(w["hist_leaf_visits"]) == w["leaf_visits"], ctx
    assert sum(w["hist_pair_steps"]) <= w["pair_steps"], ctx
    assert w["leaf_visits"] <= w["leaf_lanes"] <= 64 * w["leaf_visits"], ctx
    assert w["wave_queries"] <= w["queries"] + w["lanes_unlit"], ctx          # no wave query without a lane's step
    # the fast kernel only skips: the oracle's rays are the reference's cast_ray calls
    assert w["queries"] <= orc_rays, ctx
    if opaque:     # all-opaque: one shadow ray per light and hit, traced or answered by the unlit skip
        assert w["queries"] + w["lanes_unlit"] == orc_rays, ctx
    # the scene image of a fast kernel's block
    i = s.info()
    n = i["n_instances"]
    want = fields(plan("scene_bytes", n, n, i["n_tris"], i["n_mats"], i["n_lights"], i["n_meshes"]))["scene_bytes"]
    assert w["scene_bytes"] == want, ctx


def _work_call(rt, s, **kw):
    o = rt.RenderOpts()
    rt.lib().rt_render_opts_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return rt.lib().rt_frame_work(s._h, ctypes.byref(o), ctypes.byref(rt.Work()))


def test_frame_work_arguments(rt):
    """Checked before anything touches a device: BVH frames, 1 <= spp <= 64, untextured."""
    s = rt.Scene.load_json(scene_path("world1"), 16, 16)
    for bad in (dict(spp=0), dict(spp=65), dict(use_bvh=0), dict(textures=1), dict(row_step=0), dict(row0=-1)):
        assert _work_call(rt, s, **bad) == rt.RT_ERR_ARG, bad
    assert rt.lib().rt_frame_work(s._h, None, ctypes.byref(rt.Work())) == rt.RT_ERR_ARG


def test_last_trace_before_a_launch(rt):
    """rt_scene_last_trace is host state: RT_ERR_STATE until a trace kernel was launched (a machine with a
    device warms a finished scene with one rt_update_scene frame, which counts)."""
    out = (ctypes.c_int32 * 8)()
    b = rt.Scene.create()
    assert rt.lib().rt_scene_last_trace(b._h, out) == rt.RT_ERR_STATE      # still building
    s = rt.Scene.load_json(scene_path("world1"), 16, 16)
    assert rt.lib().rt_scene_last_trace(s._h, None) == rt.RT_ERR_ARG
    if rt.device_count() == 0:
        with pytest.raises(rt.RtError) as e:
            s.last_trace()
        assert e.value.code == rt.RT_ERR_STATE
    else:
        assert s.last_trace()["ns_bucket"] in (0, 2, 9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "mid"])
def test_frame_work_without_a_profiling_variant(gpu, work_scenes, name):
    """The profiling variant is the parked axis kernel's: a single cube has no ordered tree, and the
    876-cube field's tree leaves no room for the parking area (80 n - 64 + 102400 + 4096 > 161792 B)."""
    s, _ = work_scenes(name)
    s.set_env(depth=3)
    with pytest.raises(gpu.RtError) as e:
        s.frame_work(spp=2)
    assert e.value.code == gpu.RT_ERR_STATE
    assert not s.last_trace()["mode"] & kr.M_PROF


@pytest.mark.gpu
def test_last_trace_follows_every_entry(gpu, work_scenes):
    """rt_scene_last_trace is the launch's own record: it changes with the entry that launched last."""
    s, _ = work_scenes("two")
    s.set_env(depth=3)
    s.render(spp=2, stats=False)
    assert s.last_trace()["mode"] == kr.M_PARK | kr.M_FT | kr.M_AXIS | kr.M_SHADE
    s.render(spp=2, stats=True)
    assert (s.last_trace()["ns_bucket"], s.last_trace()["mode"]) == (9, kr.M_STATS)
    s.update_scene(16, False)
    assert s.last_trace()["mode"] == kr.M_BRUTE | kr.M_PARK | kr.M_SHADE | kr.M_AXIS
    s.debug_cast(3, 5)
    assert s.last_trace()["mode"] == kr.M_STATS
    s.frame_work(spp=2)
    assert s.last_trace()["mode"] & kr.M_PROF
