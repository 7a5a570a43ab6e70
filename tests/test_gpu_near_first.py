"""Nearer child first in closest-hit queries: a frame is the same bits with
the switch on, with it off, from the counted kernel (the reference's walk) and from the oracle, on
scenes built to make the visiting order matter -- a far cube that the tree lists first, exact ties
between leaves (coincident cubes, coplanar overlapping faces), neighbours 0.001 apart seen at grazing
angles and from their face planes and edges, lanes of a wave that disagree on the nearer child,
reflection queries -- and the counters say that the order was in fact changed (swaps) and that the
ties were in fact caught (reruns).  Frames are 64 x 48."""
import numpy as np
import pytest

import integrator_cases as ic
import kernel_recipes as kr
from twin import Twin, assert_frames_equal, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
W, H = 64, 48
FWD, BACK = (0.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 0.0)      # looking along +z, along -z (half a turn about y)
LEFT, RIGHT = (0.0, -0.7071068, 0.0, 0.7071068), (0.0, 0.7071068, 0.0, 0.7071068)   # along -x, along +x
KA = (0.1, 0.1, 0.1, 1)
GREY = ic.material(Ka=KA, Kd=(0.6, 0.5, 0.3, 1), Ks=(0.2, 0.2, 0.2, 1), alpha=8.0)
RED = ic.material(Ka=KA, Kd=(0.6, 0.2, 0.2, 1), Ks=(0.3, 0.3, 0.3, 1), alpha=4.0)
MIRROR = ic.material(Ka=(0.05, 0.05, 0.05, 1), Kd=(0.3, 0.3, 0.3, 1), Kr=(0.7, 0.7, 0.7, 1))


def _scene(gpu, oracle, cubes, lights="point", depth=0, cam=((0.0, 0.0, 0.0), FWD)):
    """cubes: (size, material, position[, quaternion]) each; returns (product scene, oracle scene)."""
    t = Twin(gpu, oracle)
    meshes = {}
    for c in cubes:
        key = (c[0], id(c[1]))
        if key not in meshes:
            meshes[key] = t.build_cube(c[0], c[1])
        i = t.add_trans(meshes[key])
        t.set_trans(i, pos=c[2], quat=c[3] if len(c) > 3 else None)
    if lights in ("point", "both"):
        t.add_point_light((-1.5, 6.0, -2.0), (1.0, 1.0, 1.0, 1.0))
    if lights in ("dir", "both"):
        t.add_directional_light((0.5, -1.0, 0.1), (0.9, 0.8, 0.7, 1.0))
    t.finish(W, H, ic.FOV, ic.UNIT, cam_pos=cam[0], cam_quat=cam[1], dist_atten=ic.DIST_ATTEN, ambience=ic.AMBIENCE,
             depth=depth)
    return t.gpu, t.orc


def _bits_equal(a, b, ctx):
    for k in WANT:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (ctx, k)


def _four_ways(s, o, oracle, ctx, cam=None, spp=1, row0=0, row_step=1, in_class=True):
    """The frame with the switch on, off, from the counted kernel and from the oracle: all equal.
    Returns the counters of the frame rendered with the switch on."""
    if cam is not None:
        s.set_camera(*cam)
        o.set_camera(*cam)
    kw = dict(spp=spp, want=WANT, row0=row0, row_step=row_step, compact=row_step > 1)
    s.set_near_first(1)
    s.shadow_hints_fill(0)
    on = s.render(stats=False, **kw)
    lt = s.last_trace()
    c = s.near_first_counters()
    hinted = lt["ns_bucket"] == 0 and lt["mode"] & kr.M_FT and not lt["mode"] & (kr.M_PART | kr.M_STATS | kr.M_PROF) and \
        lt["ftree"] == 1
    assert bool(hinted) == in_class, (ctx, lt)
    s.set_near_first(0)
    s.shadow_hints_fill(0)
    off = s.render(stats=False, **kw)
    c_off = s.near_first_counters()
    s.set_near_first(1)
    assert (c_off["queries"], c_off["reruns"], c_off["swaps"]) == (0, 0, 0), (ctx, c_off)
    counted = s.render(stats=True, **kw)
    _bits_equal(on, off, ctx + ("on/off",))
    _bits_equal(on, counted, ctx + ("on/counted",))
    of = orc_render(oracle, o, spp=spp, row0=row0, row_step=row_step)
    if row_step > 1:
        n = on["rgba"].shape[0]
        of = {k: np.ascontiguousarray(v[row0::row_step][:n]) for k, v in of.items() if k in WANT}
    assert_frames_equal(on, of, ctx=ctx, max_pm1=0)
    assert c["reruns"] <= c["queries"], (ctx, c)
    return c


def test_far_cube_first_in_the_tree(gpu, oracle):
    """Two cubes one behind the other, from both sides: in one view the tree's first child is the far cube."""
    s, o = _scene(gpu, oracle, [(1.0, RED, (0.0, 0.0, 3.0)), (1.0, GREY, (0.1, 0.05, 5.0))])
    cs = [_four_ways(s, o, oracle, ("behind", i), cam=cam) for i, cam in
          enumerate((((0.2, 0.3, 0.0), FWD), ((0.2, 0.3, 8.0), BACK)))]
    assert all(c["queries"] > 0 and c["reruns"] == 0 for c in cs), cs
    assert sum(c["swaps"] for c in cs) > 0 and min(c["swaps"] for c in cs) == 0, cs


def test_coincident_cubes(gpu, oracle):
    """Two cubes in the same place: every hit on them is an exact tie between two leaves.  The frames are
    compared first (in _four_ways), the rerun counter after."""
    s, o = _scene(gpu, oracle, [(1.0, RED, (0.0, 0.0, 3.0)), (1.0, GREY, (0.0, 0.0, 3.0)), (1.0, GREY, (2.0, 0.0, 4.0))])
    cs = [_four_ways(s, o, oracle, ("coincident", i), cam=cam) for i, cam in
          enumerate((((0.3, 0.4, 0.0), FWD), ((0.3, 0.4, 7.0), BACK)))]
    assert all(c["reruns"] > 0 for c in cs), cs


def test_coplanar_overlapping_faces(gpu, oracle):
    """Cubes whose front faces share the plane z = 2.5 and overlap on screen: ties between leaves where they do."""
    s, o = _scene(gpu, oracle, [(1.0, RED, (0.0, 0.0, 3.0)), (1.0, GREY, (0.5, 0.25, 3.0)), (2.0, GREY, (-0.5, 0.0, 3.5)),
                                (1.0, RED, (0.0, 0.0, 6.0))])
    # (the first view looks straight at the shared plane; the others see it from the side and from behind)
    cs = [_four_ways(s, o, oracle, ("coplanar", i), cam=cam) for i, cam in
          enumerate((((0.2, 0.1, 0.0), FWD), ((1.5, 0.6, 0.5), FWD), ((0.2, 0.1, 9.0), BACK)))]
    assert cs[0]["reruns"] > 0, cs


ROW = [(1.0, (RED, GREY)[k & 1], (1.001 * k, 0.0, 4.0)) for k in range(7)]


@pytest.fixture(scope="module")
def row(gpu, oracle):
    return _scene(gpu, oracle, ROW + [(12.0, GREY, (3.0, -6.5, 4.0))])


@pytest.mark.parametrize("cam", [
    ((-3.0, 0.2, 3.4), RIGHT), ((9.0, 0.2, 4.3), LEFT),             # grazing, along the row from either end
    ((-2.0, 0.5, 3.5), RIGHT), ((8.5, 0.5, 3.5), LEFT),             # the eye on the plane of the faces z = 3.5, and y = 0.5
    ((0.5, 0.5, 0.0), FWD), ((1.5005, 0.3, 0.0), FWD),              # on a face plane x = 0.5; in a gap between neighbours
    ((3.5025, 0.5, 3.5), FWD), ((3.0, 2.0, 1.0), ic.DOWN45),        # on an edge; from above
], ids=lambda c: "%g_%g_%g" % c[0])
def test_adjacent_cubes(row, oracle, cam):
    s, o = row
    c = _four_ways(s, o, oracle, ("row",) + cam[0], cam=cam)
    assert c["queries"] > 0, c


def test_lanes_disagree_on_the_nearer_child(gpu, oracle):
    """A 3 x 3 field of cubes and a camera on its middle plane, looking along it and across it."""
    cubes = [(1.0, (RED, GREY)[(i + j) & 1], (1.5 * i, 0.0, 5.0 + 1.5 * j)) for i in (-1, 0, 1) for j in (0, 1, 2)]
    s, o = _scene(gpu, oracle, cubes + [(12.0, GREY, (0.0, -6.5, 6.0))], lights="both")
    swaps = 0
    for i, cam in enumerate((((0.0, 0.2, 0.0), FWD), ((0.0, 0.3, 12.0), BACK), ((-6.0, 0.2, 6.5), RIGHT),
                             ((0.75, 3.0, 1.0), ic.DOWN45))):
        c = _four_ways(s, o, oracle, ("field", i), cam=cam)
        swaps += c["swaps"]
    assert swaps > 0


YARD = [(12.0, GREY, (0.0, -6.0, 5.0)), (1.0, RED, (0.0, 0.5, 4.0)), (2.0, GREY, (-1.6, 1.0, 5.0)), (1.0, MIRROR, (1.7, 0.5, 4.9)),
        (1.0, RED, (2.2, 0.5, 2.8)), (1.0, RED, (0.3, 0.5, 6.1)), (1.0, GREY, (-0.9, 0.5, 2.9))]
YARD_CAM = ((0.2, 4.0, -0.5), ic.DOWN45)


@pytest.fixture(scope="module")
def yards(gpu, oracle):
    cache = {}

    def get(lights):
        if lights not in cache:
            cache[lights] = _scene(gpu, oracle, YARD, lights=lights, depth=2, cam=YARD_CAM)
        return cache[lights]
    return get


def test_mirror_at_depth_two(yards, oracle):
    s, o = yards("point")
    c = _four_ways(s, o, oracle, ("mirror",))
    of = orc_render(oracle, o)
    assert (of["hit_inst"] == 3).sum() > 20 and s.info()["depth"] == 2
    assert c["queries"] > 0 and c["swaps"] > 0, c


@pytest.mark.parametrize("row0,row_step", [(0, 1), (1, 2)], ids=("whole", "slice"))
@pytest.mark.parametrize("spp", (1, 8))
@pytest.mark.parametrize("lights", ("point", "dir", "both"))
def test_lights_samples_slices(yards, oracle, lights, spp, row0, row_step):
    s, o = yards(lights)
    c = _four_ways(s, o, oracle, ("yard", lights, spp, row0, row_step), spp=spp, row0=row0, row_step=row_step)
    assert c["queries"] > 0, c


def test_outside_the_class(gpu, oracle):
    """A rotated instance (no pruning claim) and a refractive scene (NS > 0): the walk is today's, the counters stay 0."""
    q = (0.0, 0.1305262, 0.0, 0.9914449)                       # 15 degrees about y
    s, o = _scene(gpu, oracle, [(1.0, RED, (0.0, 0.0, 3.0)), (1.0, GREY, (0.1, 0.05, 5.0), q), (1.0, GREY, (1.2, 0.0, 4.0))])
    # (the kernel is one that takes hints -- ordered tree, NS = 0 -- and the host clears the mode for the scene)
    for i, cam in enumerate((((0.2, 0.3, 0.0), FWD), ((0.2, 0.3, 8.0), BACK))):
        c = _four_ways(s, o, oracle, ("rotated", i), cam=cam, in_class=True)
        assert (c["queries"], c["reruns"], c["swaps"]) == (0, 0, 0), c
    t = Twin(gpu, oracle)
    ic.build(t, "two_slabs", depth=2)
    c = _four_ways(t.gpu, t.orc, oracle, ("two_slabs",), in_class=False)
    assert (c["queries"], c["reruns"], c["swaps"]) == (0, 0, 0), c
