"""Every trace kernel of the build, by name, against the oracle.

choose_trace_variant's table (rt_kernels.hip) holds 47 trace_kernel<NS, LDS, MODE> instantiations;
tests/kernel_recipes.py has one scene + launch options per kernel (proved on the host by
tests/test_kernel_recipes.py).  Each case here renders its recipe at 64 x 48 (32 x 24 at 65 spp)
from two cameras, asserts through Scene.last_trace() that the launch used exactly that kernel
(a frame that ran some other kernel fails here), and holds the frame to the parity bar: hit
ids equal, radiance within 1e-5 relative, RGBA8 bytes equal to the oracle's.  Counted kernels
also match the oracle's work counters; uncounted ones also equal the counted frame bit for bit;
the M_PROF kernels' frames come from rt_frame_work and equal the fast frame's.  NS 2 / NS 9
recipes must exercise their frame stack: the oracle's frame changes with the depth."""
import numpy as np
import pytest

import kernel_recipes as kr
from test_plan_host import plan  # noqa: F401  (the plan_host fixture)
from twin import Twin, assert_frames_equal, mirror_camera, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
STAT_KEYS = ("rays", "nodes", "leaves", "tri_tests")


@pytest.fixture(scope="module")
def scenes(gpu, oracle, tmp_path_factory):
    """(product scene, oracle scene, the scene's own camera pose), built once per scene and frame size."""
    tmp, cache = tmp_path_factory.mktemp("recipes"), {}

    def get(name, size):
        if (name, size) not in cache:
            s, o = kr.build_scene(name, size, gpu, oracle, tmp)
            p, q = s.camera()
            cache[name, size] = (s, o, (tuple(float(x) for x in p), tuple(float(x) for x in q)))
        return cache[name, size]
    return get


@pytest.fixture(scope="module")
def oracle_frames(oracle):
    """The oracle's frame of a scene, pose, depth and options: rendered once, shared, never written to."""
    cache = {}

    def get(o, ident, depth, tex, spp, use_bvh):
        k = ident + (depth, bool(tex), spp, bool(use_bvh))
        if k not in cache:
            o.set_env(depth=depth)
            o.set_textures(bool(tex))
            cache[k] = orc_render(oracle, o, spp=spp, use_bvh=int(use_bvh))
        return cache[k]
    return get


def _bits_equal(a, b, keys, ctx):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (ctx, k)


@pytest.mark.parametrize("key", sorted(kr.RECIPES), ids=kr.kernel_id)
def test_kernel_against_oracle(gpu, plan, scenes, oracle_frames, monkeypatch, key):  # noqa: F811
    r = kr.RECIPES[key]
    size = kr.frame_size(r)
    s, o, own = scenes(r.scene, size)
    family = kr.parse(r.scene)[0]
    if r.no_part:
        monkeypatch.setenv("RT_NO_PART", "1")                 # choose_trace_variant reads it at every launch
    else:
        monkeypatch.delenv("RT_NO_PART", raising=False)
    s.set_env(depth=r.depth)
    want = kr.plan_key(plan, s, r)
    assert (want["ns_bucket"], want["lds"], want["mode"]) == key
    kw = dict(spp=r.spp, use_bvh=r.use_bvh, textures=r.tex, want=WANT)

    def check_launch(ctx):
        lt = s.last_trace()
        assert (lt["ns_bucket"], lt["lds"], lt["mode"]) == key, (ctx, lt)
        for f in ("mode", "shm", "part_k", "sky", "sky_brute"):
            assert lt[f] == want[f], (ctx, f, lt, want)
        assert lt["ftree"] == (0 if family in ("one", "chain") else 1), (ctx, lt)   # one leaf; a tree deeper than 31

    for cam, pose in enumerate((own, kr.second_camera(r.scene, s))):
        ctx = (kr.kernel_id(key), r.scene, "cam%d" % cam)
        s.set_camera(*pose)
        mirror_camera(s, o)
        of = oracle_frames(o, (r.scene, size, cam), r.depth, r.tex, r.spp, r.use_bvh)
        if cam == 1:                                          # part of the frame hits, part misses
            hit = float((of["hit_inst"] >= 0).mean())
            assert hit >= 0.05 and 1.0 - hit >= 0.05, (ctx, hit)
        if r.prof:
            # the profiling variant's frame: the fast frame's bytes, and the oracle's
            _, rgba = s.frame_work(spp=r.spp, want_rgba=True)
            check_launch(ctx)
            fast = s.render(stats=False, **kw)
            assert s.last_trace()["mode"] == key[2] & ~kr.M_PROF | kr.M_SHADE, ctx
            assert np.array_equal(rgba, fast["rgba"]), ctx
            assert_frames_equal({"rgba": rgba}, of, keys=("rgba",), ctx=ctx, max_pm1=0)
            assert_frames_equal(fast, of, ctx=ctx, max_pm1=0)
            continue
        fr = s.render(stats=r.stats, **kw)
        check_launch(ctx)
        assert_frames_equal(fr, of, ctx=ctx, max_pm1=0)
        if r.stats:
            assert tuple(fr["stats"][k] for k in STAT_KEYS) == tuple(int(x) for x in of["stats"]), ctx
        else:                                                 # the counted frame of the same scene and pose
            full = s.render(stats=True, **kw)
            assert s.last_trace()["mode"] & kr.M_STATS, ctx
            _bits_equal(fr, full, WANT, ctx)

    # the recipe exercises its frame stack (on the oracle alone; the second camera's frame)
    if key[0] != 0:
        ident = (r.scene, size, 1)
        of = oracle_frames(o, ident, r.depth, r.tex, r.spp, r.use_bvh)
        for shallower in ((0,) if key[0] == 2 else (0, 2)):
            of_s = oracle_frames(o, ident, shallower, r.tex, r.spp, r.use_bvh)
            assert not np.array_equal(of["rgba"], of_s["rgba"]), (kr.kernel_id(key), "refraction never shows", shallower)


def test_deep_ordered_tree_falls_back_to_the_heap(gpu, oracle):
    """ftree = 0 by shape with more than one instance: ordered_tree_shape turns the fast tree off
    above depth 31 (the fast traversal's stack).  37 cubes whose centres' Morton keys form a chain
    (kernel_recipes.chain_positions) give depth 36; the frame then runs a heap kernel and must equal the oracle's."""
    pos = kr.chain_positions()
    keys = sorted(int(k) for k in oracle.kat("zorder", -pos))  # gen_morton's key of a box: z_order(-centre)
    assert keys == kr.morton_keys(pos)                         # (z_order.cu:5-36 interleaves the bits of -v)
    assert len(set(keys)) == len(pos) >= 34 and kr.radix_tree_depth(keys) > kr.FT_MAX_DEPTH
    m = gpu.material
    t = Twin(gpu, oracle)
    meshes = [t.build_cube(0.25, mt) for mt in (m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.6, 0.3, 0.1, 1)),
                                                m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.2, 0.5, 0.2, 1), Ks=(0.8, 0.8, 0.8, 1), alpha=6.0))]
    for k, p in enumerate(pos):
        t.set_trans(t.add_trans(meshes[k % 2]), pos=[float(x) for x in p])
    t.add_point_light((100.0, 140.0, 60.0), (1.0, 1.0, 1.0, 1.0))
    t.add_directional_light((0.3, -1.0, 0.8), (0.9, 0.8, 0.7, 1.0))
    c = pos[-1]
    t.finish(64, 48, 60.0, 100.0, cam_pos=(float(c[0]) - 0.5, float(c[1]) - 0.5, float(c[2]) - 4.0),
             dist_atten=(0.1, 0.0, 0.0), ambience=(0.3, 0.3, 0.3, 1.0), depth=2)
    s, o = t.gpu, t.orc
    of = orc_render(oracle, o, spp=4)
    hit = float((of["hit_inst"] >= 0).mean())
    assert hit >= 0.05 and 1.0 - hit >= 0.05, hit
    fast = s.render(spp=4, want=WANT, stats=False)
    lt = s.last_trace()
    assert lt["ftree"] == 0 and not lt["mode"] & (kr.M_FT | kr.M_AXIS), lt
    assert_frames_equal(fast, of, ctx="deep tree, fast", max_pm1=0)
    full = s.render(spp=4, want=WANT, stats=True)
    assert_frames_equal(full, of, ctx="deep tree, counted", max_pm1=0)
    assert tuple(full["stats"][k] for k in STAT_KEYS) == tuple(int(x) for x in of["stats"])
    _bits_equal(fast, full, WANT, "deep tree")
