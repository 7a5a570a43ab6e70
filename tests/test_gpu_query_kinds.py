"""One walk per query kind: a wave query of the hinted kernels takes the shadow
walk (hints, occlusion exit) or the normal walk (nearer child first), chosen once at the query site.
A frame cannot catch a wrong choice -- a shadow lane sent down the normal walk still returns the right
bit, only without the exit -- so every case asserts counters as well as frames.

Each scene is rendered with hints and near-first on (twice: a cold and a warm hint table), with both
switches off, from the counted kernel and from the oracle: the same bits.  The near-first counters
(queries, swaps, reruns) and the hint counters' query count do not depend on the table's races; they
equal the values recorded from the library before the walks were separated
(tests/golden/query_kinds_counters.json: the sums over a case's views, two frames each).  The seeded
and ended-by-seed counts depend on timing: only 0 <= ended <= seeded <= queries.  Frames are 64 x 48
unless a case says otherwise."""
import json
import os

import numpy as np
import pytest

import integrator_cases as ic
import kernel_recipes as kr
from twin import Twin, assert_frames_equal, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
FWD, BACK = (0.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 0.0)        # looking along +z, along -z
KA = (0.1, 0.1, 0.1, 1)
GREY = ic.material(Ka=KA, Kd=(0.6, 0.5, 0.3, 1), Ks=(0.2, 0.2, 0.2, 1), alpha=8.0)
RED = ic.material(Ka=KA, Kd=(0.6, 0.2, 0.2, 1), Ks=(0.3, 0.3, 0.3, 1), alpha=4.0)
MATT = ic.material(Ka=KA, Kd=(0.6, 0.5, 0.3, 1), alpha=1.0)   # no specular lobe: unlit where the light is behind
MIRROR = ic.material(Ka=(0.05, 0.05, 0.05, 1), Kd=(0.3, 0.3, 0.3, 1), Kr=(0.7, 0.7, 0.7, 1))
POINT = (-1.5, 6.0, -2.0)

# two cubes in line: in one of the two views the tree's first child is the far cube
INLINE = [(1.0, RED, (0.0, 0.0, 3.0)), (1.0, GREY, (0.1, 0.05, 5.0))]
INLINE_VIEWS = (((0.2, 0.3, 0.0), FWD), ((0.2, 0.3, 8.0), BACK))
YARD = [(12.0, GREY, (0.0, -6.0, 5.0)), (1.0, RED, (0.0, 0.5, 4.0)), (2.0, GREY, (-1.6, 1.0, 5.0)), (1.0, MIRROR, (1.7, 0.5, 4.9)),
        (1.0, RED, (2.2, 0.5, 2.8)), (1.0, RED, (0.3, 0.5, 6.1)), (1.0, GREY, (-0.9, 0.5, 2.9))]
YARD_VIEWS = (((0.2, 4.0, -0.5), ic.DOWN45),)
# a low cube whose top face the tall cube beside it half shadows (the light over the tall cube's edge)
HALF = [(8.0, GREY, (0.0, -4.0, 0.0)), (1.0, RED, (0.0, 0.5, 0.0)), (2.0, GREY, (-1.5, 1.0, 0.0))]
HALF_VIEWS = (((0.2, 5.0, -5.0), ic.DOWN45),)
COINCIDENT = [(1.0, RED, (0.0, 0.0, 3.0)), (1.0, GREY, (0.0, 0.0, 3.0)), (1.0, GREY, (2.0, 0.0, 4.0))]
COINCIDENT_VIEWS = (((0.3, 0.4, 0.0), FWD), ((0.3, 0.4, 7.0), BACK))

# name: cubes, views, lights, point light's position, depth, width, spp, (row0, row_step), and what must hold:
# near-first queries / swaps / reruns / hint queries each "+" (> 0), "0" (== 0) or "" (only the recorded value)
CASES = {
    "inline_point": (INLINE, INLINE_VIEWS, "point", POINT, 0, 64, 1, (0, 1), "++ +"),
    "inline_both_1spp": (INLINE, INLINE_VIEWS, "both", POINT, 0, 64, 1, (0, 1), "++ +"),
    "inline_both_8spp": (INLINE, INLINE_VIEWS, "both", POINT, 0, 64, 8, (0, 1), "++ +"),
    "mirror_depth2": (YARD, YARD_VIEWS, "point", POINT, 2, 64, 1, (0, 1), "++ +"),
    "half_shadow": (HALF, HALF_VIEWS, "point", (-1.5, 4.0, 0.3), 0, 64, 1, (0, 1), "+  +"),
    # the one face in view looks at the camera, the light is beyond the cubes (the second one is hidden behind
    # the first: two leaves, so the tree is the ordered one): every lane is unlit-skipped
    "facing_away": ([(1.0, MATT, (0.0, 0.0, 3.0)), (1.0, MATT, (0.0, 0.0, 5.0))], (((0.0, 0.0, 0.0), FWD),), "point", (0.0, 0.0, 9.0), 0, 64, 1, (0, 1), "+  0"),
    "width_62": (INLINE, INLINE_VIEWS, "both", POINT, 0, 62, 1, (0, 1), "++ +"),
    "row_slice": (YARD, YARD_VIEWS, "both", POINT, 2, 64, 1, (1, 4), "+  +"),
    "coincident": (COINCIDENT, COINCIDENT_VIEWS, "point", POINT, 0, 64, 1, (0, 1), "+ ++"),
    "refractive": ("two_slabs", (None,), None, None, 2, 48, 1, (0, 1), "0000"),
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_kinds_counters.json")
H = 48


def _scene(gpu, oracle, cubes, lights, point, depth, width):
    t = Twin(gpu, oracle)
    if isinstance(cubes, str):
        ic.build(t, cubes, depth=depth)
        return t.gpu, t.orc
    meshes = {}
    for c in cubes:
        key = (c[0], id(c[1]))
        if key not in meshes:
            meshes[key] = t.build_cube(c[0], c[1])
        t.set_trans(t.add_trans(meshes[key]), pos=c[2])
    if lights in ("point", "both"):
        t.add_point_light(point, (1.0, 1.0, 1.0, 1.0))
    if lights in ("dir", "both"):
        t.add_directional_light((0.5, -1.0, 0.1), (0.9, 0.8, 0.7, 1.0))
    t.finish(width, H, ic.FOV, ic.UNIT, cam_pos=(0.0, 0.0, 0.0), cam_quat=FWD, dist_atten=ic.DIST_ATTEN,
             ambience=ic.AMBIENCE, depth=depth)
    return t.gpu, t.orc


def _bits_equal(a, b, ctx):
    for k in WANT:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (ctx, k)


def run_case(gpu, oracle, name):
    """Renders the case every way, asserts the frames equal, and returns the counters of the frames
    rendered with both switches on, summed over the case's views."""
    cubes, views, lights, point, depth, width, spp, (row0, row_step), _ = CASES[name]
    s, o = _scene(gpu, oracle, cubes, lights, point, depth, width)
    kw = dict(spp=spp, want=WANT, row0=row0, row_step=row_step, compact=row_step > 1)
    tot = dict(nf_queries=0, nf_swaps=0, nf_reruns=0, hint_queries=0)
    for vi, cam in enumerate(views):
        ctx = (name, vi)
        if cam is not None:
            s.set_camera(*cam)
            o.set_camera(*cam)
        s.set_near_first(1)
        s.set_shadow_hints(True)
        s.shadow_hints_fill(0)
        on = [s.render(stats=False, **kw) for _ in range(2)]   # a cold table, then a warm one
        lt = s.last_trace()
        in_class = lt["ns_bucket"] == 0 and lt["mode"] & kr.M_FT and not lt["mode"] & (kr.M_PART | kr.M_STATS | kr.M_PROF) and \
            lt["ftree"] == 1
        assert bool(in_class) == (name != "refractive"), (ctx, lt)
        c, h = s.near_first_counters(), s.shadow_hint_counters()
        print(ctx, "near-first", c, "hints", h)
        assert 0 <= h["ended"] <= h["seeded"] <= h["queries"], (ctx, h)
        assert c["reruns"] <= c["queries"], (ctx, c)
        s.set_near_first(0)
        s.set_shadow_hints(False)
        s.shadow_hints_fill(0)
        off = s.render(stats=False, **kw)
        c0, h0 = s.near_first_counters(), s.shadow_hint_counters()
        assert (c0["queries"], c0["reruns"], c0["swaps"], h0["queries"], h0["seeded"], h0["ended"]) == (0,) * 6, (ctx, c0, h0)
        s.set_near_first(1)
        s.set_shadow_hints(True)
        counted = s.render(stats=True, **kw)
        for i, f in enumerate(on):
            _bits_equal(f, off, ctx + ("on/off", i))
        _bits_equal(on[0], counted, ctx + ("on/counted",))
        of = orc_render(oracle, o, spp=spp, row0=row0, row_step=row_step)
        if row_step > 1:
            n = on[0]["rgba"].shape[0]
            of = {k: np.ascontiguousarray(v[row0::row_step][:n]) for k, v in of.items() if k in WANT}
        assert_frames_equal(on[0], of, ctx=ctx, max_pm1=0)
        tot["nf_queries"] += c["queries"]; tot["nf_swaps"] += c["swaps"]; tot["nf_reruns"] += c["reruns"]
        tot["hint_queries"] += h["queries"]
    return tot


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(CASES))
def test_query_kinds(gpu, oracle, golden, name):
    tot = run_case(gpu, oracle, name)
    want = CASES[name][8]
    for k, w in zip(("nf_queries", "nf_swaps", "nf_reruns", "hint_queries"), want):
        if w == "+":
            assert tot[k] > 0, (name, k, tot)
        if w == "0":
            assert tot[k] == 0, (name, k, tot)
    assert tot == golden[name], (name, tot, golden[name])
