"""The integrator scenes of tests/integrator_cases.py on the oracle alone: before a frame of them is
compared on a device (tests/test_gpu_integrator.py), the oracle's census proves that the frame
is decided by the rules a single refractive material cannot tell apart.  The floors below are
conditions on the scenes (a pose or a lattice that misses one is changed, not the floor); the measured
counts are in profiles/integrator/census.txt.  Also here: the census entry renders what orc_render
renders and counts the same with any thread count, the depth limits of both libraries, the launch
plan's shortcuts and kernels for these scenes, and the committed depth-9 frame."""
import os

import numpy as np
import pytest

import integrator_cases as ic
import kernel_recipes as kr
from conftest import GOLDEN
from oracle_lib import CENSUS
from test_plan_host import plan  # noqa: F401  (the plan_host fixture)

DEPTHS = tuple(range(10))
OUT = ("rgba", "radiance", "hit_inst", "hit_tri")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def frames(oracle):
    """The oracle's frame and census of (scene, pose, depth) at 1 spp: rendered once, shared, never written to."""
    scenes, cache = {}, {}

    def get(name, pose, depth):
        if name not in scenes:
            scenes[name] = oracle.create()
            ic.build(scenes[name], name)
        if (name, pose, depth) not in cache:
            o = scenes[name]
            o.set_camera(*ic.poses(name)[pose])
            o.set_env(depth=depth)
            cache[name, pose, depth] = oracle.render(o, nthreads=4, census=True)
        return cache[name, pose, depth]
    return get


def test_no_two_cubes_share_a_face_plane():
    """Coincident faces tie on the hit time; the winner is then the traversal's visiting order."""
    for axis, planes in enumerate(ic.face_planes(ic.media_cubes())):
        assert len(np.unique(planes)) == planes.size == 64, axis
    mats = [m for m, _ in ic.media_cubes()]
    assert sorted(set(mats)) == [0, 1, 2, 3, 4] and mats[ic.INSIDE_CUBE] == 0
    c = np.array(ic.media_cubes()[ic.INSIDE_CUBE][1])
    assert (np.abs(np.array(ic.MEDIA_POSES["inside"][0]) - c) < 0.3).all()     # within the cube, clear of its neighbours


def test_media_reaches_every_rule(frames):
    c = frames("media", "above", 9)["census"]
    print(ic.census_row(c))
    assert c["max_top"] == 9
    for k in ("inobj_other_mat", "refract_eta_differs", "refract_resumed", "tir_entering", "shadow_continued",
              "shadow_back_face"):
        assert c[k] >= 50, (k, c)
    assert c["tir"] - c["tir_entering"] >= 50, c
    assert c["shadow_past_light"] >= 1, c
    # the counts nest as their definitions do
    assert c["inobj_hits"] >= c["inobj_other_mat"]
    assert c["refract_mat_differs"] >= c["refract_mat_differs_refractive"] >= c["refract_eta_differs"]
    assert c["shadow_continued"] >= c["shadow_back_face"]
    c0 = frames("media", "above", 0)["census"]
    assert c0["depth0_hits"] >= 1000, c0
    assert c0["max_top"] == c0["inobj_hits"] == c0["refract_mat_differs"] == c0["tir"] == 0, c0


def test_kt_above_one_leaves_the_paths_alone(frames):
    """media_kt_gt1 differs from media in one Kt channel: the same events, another frame."""
    a, b = frames("media", "above", 9), frames("media_kt_gt1", "above", 9)
    assert a["census"] == b["census"]
    assert np.array_equal(a["hit_inst"], b["hit_inst"]) and not np.array_equal(a["rgba"], b["rgba"])


def test_two_slabs_is_the_control(frames):
    c = frames("two_slabs", "own", 9)["census"]
    print(ic.census_row(c))
    assert c["inobj_other_mat"] == 0 and c["refract_eta_differs"] == 0 and c["refract_mat_differs"] == 0
    assert c["max_top"] == 0 and c["refract_resumed"] == 0             # no reflective material: no suspended frame
    # ... and still a refraction scene: both slabs entered and left, light through them
    assert c["inobj_hits"] >= 50 and c["tir_entering"] >= 1 and c["tir"] > c["tir_entering"] and c["shadow_back_face"] >= 50, c
    assert not np.array_equal(frames("two_slabs", "own", 4)["rgba"], frames("two_slabs", "own", 1)["rgba"])


def test_sky_pose_sees_sky(frames):
    miss = float((frames("media", "sky", 9)["hit_inst"] < 0).mean())
    assert 0.05 <= miss <= 0.95, miss


@pytest.mark.parametrize("pose", sorted(ic.MEDIA_POSES))
def test_every_depth_shows_and_fills_its_stack(frames, pose):
    for d in DEPTHS:
        fr = frames("media", pose, d)
        assert fr["census"]["max_top"] == d, (pose, d, fr["census"])
        if d:
            assert not np.array_equal(fr["rgba"], frames("media", pose, d - 1)["rgba"]), (pose, d)


@pytest.mark.parametrize("name,pose,depth,spp,use_bvh", [("media", "above", 9, 1, 1), ("media", "sky", 5, 4, 1),
                                                         ("media", "inside", 2, 1, 0), ("two_slabs", "own", 9, 1, 1)])
def test_census_renders_what_orc_render_renders(oracle, name, pose, depth, spp, use_bvh):
    o = oracle.create()
    ic.build(o, name, depth=depth)
    o.set_camera(*ic.poses(name)[pose])
    plain = oracle.render(o, spp=spp, use_bvh=use_bvh, nthreads=2)
    counted = oracle.render(o, spp=spp, use_bvh=use_bvh, nthreads=2, census=True)
    assert "census" not in plain and tuple(counted["census"]) == CENSUS
    for k in OUT + ("stats",):
        assert np.array_equal(_bits(plain[k]), _bits(counted[k])), k


def test_census_is_the_same_with_any_thread_count(oracle, frames):
    o = oracle.create()
    ic.build(o, "media")
    one = oracle.render(o, nthreads=1, census=True)
    eight = oracle.render(o, nthreads=8, census=True)
    assert one["census"] == eight["census"] == frames("media", "above", 9)["census"]
    assert np.array_equal(one["rgba"], eight["rgba"])
    rows = oracle.render(o, nthreads=3, row0=1, row_step=2, census=True)["census"]       # a row slice counts its rows only
    assert 0 < rows["inobj_hits"] < one["census"]["inobj_hits"]


def test_depth_limits(rt, oracle):
    """The frame stack holds MAX_DEPTH = 10 frames (scene.cu:25): depth 9 is the deepest either library takes."""
    s, o = rt.Scene.create(), oracle.create()
    for b in (s, o):
        ic.build(b, "two_slabs", depth=9)
    assert s.info()["depth"] == o.depth == 9
    for bad in (10, -1):
        assert rt.lib().rt_env_set(s._h, None, None, bad) == rt.RT_ERR_ARG
        assert oracle.L.orc_set_env(o.h, None, None, bad) == -1
        assert s.info()["depth"] == 9
        o._counts()
        assert o.depth == 9
    for d in (0, 9):
        s.set_env(depth=d)
        o.set_env(depth=d)
        assert s.info()["depth"] == o.depth == d
    for bad in (10, -1):                                                     # and at finish
        assert oracle.L.orc_builder_finish(oracle.create().h, 8, 8, ic.FOV, ic.UNIT, None, None, None, None, bad) == -1


def _host_scene(rt, name):
    s = rt.Scene.create()
    ic.build(s, name)
    return s


def shortcuts(plan, s, depth, want_stats=0):  # noqa: F811  (the fixture's runner, passed in)
    m, lights, env = s.export("materials"), s.export("lights"), s.export("env")
    args = ["shortcuts", want_stats, 0, depth] + [repr(float(v)) for v in env[3:7]] + [len(m), len(lights)]
    for row in m:
        args += [repr(float(v)) for v in list(row[0:8]) + list(row[16:20])]          # Ke, Ka, Kt
    for row in lights:
        args += [repr(float(v)) for v in row[4:8]]
    t = plan(*args).split()
    return {k: int(v) for k, v in zip(t[::2], t[1::2])}


def test_shortcuts_of_the_scenes(rt, plan):  # noqa: F811
    """shade_shortcuts (rt_plan.h) on the scenes' own materials and lights: the unlit skip is on for media and
    two_slabs (every Kt in [0, 1]) and off with one Kt channel at 1.25; ns = max(depth, 1); never the
    occlusion exit (a refractive material)."""
    for name, skip in (("media", 2), ("media_kt_gt1", 0), ("two_slabs", 2)):
        s = _host_scene(rt, name)
        assert float(s.export("materials")[:, 16:20].max()) == (1.25 if name == "media_kt_gt1" else 1.0)
        for d in (0, 1, 9):
            assert shortcuts(plan, s, d) == dict(unlit_skip=skip, occl_exit=0, ns=max(d, 1)), (name, d)
            assert kr.scene_ns(s, d) == max(d, 1)
        assert shortcuts(plan, s, 9, want_stats=1)["unlit_skip"] == 0, name      # counted frames trace every shadow ray


# what each launch of test_gpu_integrator.py must run: (label, launch options) -> MODE; the bucket is 2 up to depth 2
VARIANTS = {
    "fast": (dict(), kr.M_FT | kr.M_PARK | kr.M_AXIS | kr.M_SHADE),
    "counted": (dict(stats=True), kr.M_STATS),
    "brute": (dict(use_bvh=False), kr.M_BRUTE | kr.M_PARK | kr.M_SHADE | kr.M_AXIS),
    "brute counted": (dict(use_bvh=False, stats=True), kr.M_STATS),
    "spp4": (dict(spp=4), kr.M_FT | kr.M_PARK | kr.M_AXIS | kr.M_SHADE),
    "no_part": (dict(no_part=True), kr.M_FT | kr.M_PARK | kr.M_AXIS | kr.M_SHADE),
    "prof": (dict(prof=True), kr.M_FT | kr.M_PARK | kr.M_AXIS | kr.M_PROF),
}


def variant_key(label, depth):
    """(ns_bucket, lds, mode): counted frames run the generic kernels (NS 9) at any depth."""
    mode = VARIANTS[label][1]
    return (9 if depth >= 3 or mode == kr.M_STATS else 2, 1, mode)


@pytest.mark.parametrize("name", ic.SCENES)
def test_plan_of_the_variants(rt, plan, name):  # noqa: F811
    s = _host_scene(rt, name)
    assert kr.scene_ftree(s) == 1
    for d in DEPTHS:
        for label, (opts, _) in VARIANTS.items():
            got = kr.plan_key(plan, s, kr._r(name, d, **dict(dict(spp=1), **opts)))
            assert (got["ns_bucket"], got["lds"], got["mode"]) == variant_key(label, d), (name, d, label, got)
    # the fast, counted, brute-force and profiling frames are four kernels; 4 spp and RT_NO_PART stay on the fast one
    assert len({variant_key(k, 9) for k in VARIANTS}) == 4 and len({variant_key(k, 1) for k in VARIANTS}) == 4


def test_golden_media_frame_reproduces(frames):
    """tests/golden/frame_media_48x32_d9.npz (make_golden.py): media, first pose, depth 9, 1 spp."""
    g = np.load(os.path.join(GOLDEN, "frame_media_48x32_d9.npz"))
    fr = frames("media", "above", 9)
    for k in OUT + ("stats",):
        assert np.array_equal(_bits(fr[k]), _bits(g[k])), k
    assert [int(v) for v in g["census"]] == [fr["census"][k] for k in CENSUS]
