"""Shadow-query occluder hints: the frame is the same bytes whatever the hint
table holds -- empty, warm, poisoned with every code of the tree and with values that name nothing,
stale after an occluder moved -- and with the switch off, and it is the oracle's frame.

The scene: a floor, a low cube, a cube twice as tall beside it whose shadow (point light and
directional light alike) covers half of the low cube's top face, a mirror cube (depth 2), two more
cubes for a deeper tree, and a cube past the point light on the line from the low cube's top face
through the light (its hits lie beyond max_t: it occludes nothing).  Frames are 64 x 48."""
import numpy as np
import pytest

import integrator_cases as ic
import kernel_recipes as kr
from twin import Twin, assert_frames_equal, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
W, H = 64, 48
LIGHT, LIGHT_WIDE = (-1.5, 4.0, 0.3), (-3.0, 4.0, 0.3)
FLOOR, LOW, TALL, MIRROR, BEHIND = 0, 1, 2, 3, 6
TALL_POS, TALL_AWAY = (-1.5, 1.0, 0.0), (-1.5, 1.0, 9.0)
CAMERA = ((0.2, 5.0, -5.0), ic.DOWN45)


def build(b, lights, depth=2):
    ka = (0.1, 0.1, 0.1, 1)
    grey = ic.material(Ka=ka, Kd=(0.6, 0.5, 0.3, 1), Ks=(0.2, 0.2, 0.2, 1), alpha=8.0)
    red = ic.material(Ka=ka, Kd=(0.6, 0.2, 0.2, 1), Ks=(0.3, 0.3, 0.3, 1), alpha=4.0)
    mirror = ic.material(Ka=(0.05, 0.05, 0.05, 1), Kd=(0.3, 0.3, 0.3, 1), Kr=(0.7, 0.7, 0.7, 1))
    unit, tall, floor, mir = b.build_cube(1.0, red), b.build_cube(2.0, grey), b.build_cube(8.0, grey), b.build_cube(1.0, mirror)
    # the light over the tall cube's edge x = -0.5: its top edge (y = 2) shadows the low cube's top (y = 1) up to x = 0
    behind = tuple(float(np.float32(l + 0.5 * (l - p))) for l, p in zip(LIGHT, (0.25, 1.0, 0.0)))
    for mesh, pos in ((floor, (0.0, -4.0, 0.0)), (unit, (0.0, 0.5, 0.0)), (tall, TALL_POS), (mir, (1.7, 0.5, 0.9)),
                      (unit, (2.2, 0.5, -1.2)), (unit, (0.3, 0.5, 2.1)), (unit, behind)):
        b.set_trans(b.add_trans(mesh), pos=pos)
    if lights in ("point", "both"):
        b.add_point_light(LIGHT, (1.0, 1.0, 1.0, 1.0))
    if lights == "wide":                                       # further out: the whole top face of the low cube in shadow
        b.add_point_light(LIGHT_WIDE, (1.0, 1.0, 1.0, 1.0))
    if lights in ("dir", "both"):
        b.add_directional_light((0.5, -1.0, 0.1), (0.9, 0.8, 0.7, 1.0))
    b.finish(W, H, ic.FOV, ic.UNIT, cam_pos=CAMERA[0], cam_quat=CAMERA[1], dist_atten=ic.DIST_ATTEN,
             ambience=ic.AMBIENCE, depth=depth)


@pytest.fixture(scope="module")
def twins(gpu, oracle):
    cache = {}

    def get(lights):
        if lights not in cache:
            t = Twin(gpu, oracle)
            build(t, lights)
            cache[lights] = (t.gpu, t.orc)
        return cache[lights]
    return get


@pytest.fixture(scope="module")
def ref(twins, oracle):
    """The oracle's frame of a scene at the tall cube's home position (rendered once per case, shared)."""
    cache = {}

    def get(lights, spp=1, row0=0, row_step=1):
        k = (lights, spp, row0, row_step)
        if k not in cache:
            cache[k] = orc_render(oracle, twins(lights)[1], spp=spp, row0=row0, row_step=row_step)
        return cache[k]
    return get


def _bits_equal(a, b, ctx):
    for k in WANT:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (ctx, k)


def _hinted(s, ctx):
    """The launch ran a kernel that takes hints: ordered tree, NS = 0, wholly parked or unparked."""
    lt = s.last_trace()
    assert lt["ns_bucket"] == 0 and lt["mode"] & kr.M_FT and not lt["mode"] & (kr.M_PART | kr.M_STATS | kr.M_PROF) and \
        lt["ftree"] == 1, (ctx, lt)


def _frame(s, spp=1, row0=0, row_step=1):
    return s.render(spp=spp, want=WANT, stats=False, row0=row0, row_step=row_step, compact=row_step > 1)


def _rows(fr, of, row0, row_step):
    """The oracle's rows of a compact slice (the oracle renders the slice in place in a whole frame)."""
    if row_step == 1:
        return of
    n = fr["rgba"].shape[0]
    return {k: np.ascontiguousarray(v[row0::row_step][:n]) for k, v in of.items() if k in WANT}


CASES = [("point", 1, 0, 1), ("dir", 1, 0, 1), ("both", 1, 0, 1), ("both", 8, 0, 1), ("point", 8, 0, 1), ("both", 1, 1, 2)]


@pytest.mark.parametrize("lights,spp,row0,row_step", CASES)
def test_cold_warm_off(twins, ref, lights, spp, row0, row_step):
    s, _ = twins(lights)
    ctx = (lights, spp, row0, row_step)
    s.set_shadow_hints(True)
    s.shadow_hints_fill(0)
    on = [_frame(s, spp, row0, row_step) for _ in range(3)]
    _hinted(s, ctx)
    c = s.shadow_hint_counters()
    assert c["entries"] == 7 * 64 and c["queries"] > 0 and c["seeded"] > 0 and c["ended"] > 0, (ctx, c)
    assert c["ended"] <= c["seeded"] <= c["queries"], (ctx, c)
    s.set_shadow_hints(False)
    s.shadow_hints_fill(0)
    off = _frame(s, spp, row0, row_step)
    _hinted(s, ctx)
    c = s.shadow_hint_counters()
    assert (c["queries"], c["seeded"], c["ended"]) == (0, 0, 0), (ctx, c)
    s.set_shadow_hints(True)
    for i, f in enumerate(on):
        _bits_equal(f, off, ctx + (i,))
    assert_frames_equal(off, _rows(off, ref(lights, spp, row0, row_step), row0, row_step), ctx=ctx, max_pm1=0)


def test_mirror_pixels_shade_and_shadow(twins, ref):
    """The scene does what the cases need: the mirror cube is seen, the low cube's top face is part lit and
    part shadowed (the oracle's radiance differs along it), at depth 2."""
    s, o = twins("point")
    of = ref("point")
    assert (of["hit_inst"] == MIRROR).sum() > 20 and s.info()["depth"] == 2
    top = (of["hit_inst"] == LOW)
    lum = of["radiance"][..., :3].sum(-1)[top]
    assert top.sum() > 40 and lum.max() > 2.0 * lum.min() > 0.0, (int(top.sum()), float(lum.min()), float(lum.max()))


@pytest.mark.parametrize("lights", ("point", "both"))
def test_poisoned_table(twins, ref, lights):
    """Every entry set to one value: the code of each instance's leaf (the shaded cubes themselves and the
    cube behind the light among them), every other code of the tree, and values that name no record."""
    s, _ = twins(lights)
    s.set_shadow_hints(True)
    base = _frame(s)
    assert_frames_equal(base, ref(lights), ctx=lights, max_pm1=0)
    codes = {k: s.shadow_hint_code(k) for k in range(7)}
    n_real = s.export("bvh_info")["n_real"]
    assert n_real == 7 and sorted(codes.values()) == sorted(set(codes.values())) and min(codes.values()) >= 1, codes
    assert max(codes.values()) <= 2 * (n_real - 1), codes
    fills = [codes[k] for k in (LOW, TALL, FLOOR, MIRROR, BEHIND, 4, 5)]
    fills += [c for c in range(1, 2 * (n_real - 1) + 1) if c not in codes.values()]      # sides that are internal nodes
    fills += [2 * (n_real - 1) + 1, 7 + 7, -1, -2**31, 0x7fffffff, 0x7ffffffe]
    for v in fills:
        s.shadow_hints_fill(v)
        f = _frame(s)
        _bits_equal(f, base, (lights, v))
        c = s.shadow_hint_counters()
        assert c["queries"] > 0 and (c["seeded"] > 0 or not 1 <= v <= 2 * (n_real - 1)), (v, c)
    s.shadow_hints_fill(0)


def test_occluder_beyond_the_point_light(twins, ref):
    """The cube past the light is hit by every shadow ray from the lit half of the low cube's top face, beyond
    max_t: seeded with it, those queries are not ended by the seed and the face stays lit, as in the oracle."""
    s, _ = twins("point")
    s.set_shadow_hints(True)
    _frame(s)
    s.shadow_hints_fill(s.shadow_hint_code(BEHIND))
    f = _frame(s)
    c = s.shadow_hint_counters()
    assert c["seeded"] > 0 and c["ended"] < c["seeded"], c      # (the walk replaces the wasted seeds as the frame goes)
    assert_frames_equal(f, ref("point"), ctx="behind", max_pm1=0)
    s.shadow_hints_fill(0)


def test_moving_occluder(twins, oracle):
    """Warm table (the low cube's whole top face in the tall cube's shadow: every writer of its entries names
    the tall cube's leaf), then the tall cube leaves: the frame is the oracle's at once, and after the
    following frame no entry of the low cube names the tall cube's leaf (nothing shadows it any more)."""
    s, o = twins("wide")
    s.set_shadow_hints(True)
    s.shadow_hints_fill(0)
    try:
        for _ in range(2):
            _frame(s)
        tall = s.shadow_hint_code(TALL)
        assert (s.shadow_hints()[LOW] == tall).any(), (tall, s.shadow_hints()[LOW])
        for sc in (s, o):
            sc.set_trans(TALL, pos=TALL_AWAY)
        of = orc_render(oracle, o)
        a = _frame(s)
        b = _frame(s)
        assert_frames_equal(a, of, ctx="moved", max_pm1=0)
        _bits_equal(b, a, "moved, second frame")
        # cleared, or replaced by what the walk found for another lane of a wave keyed by the low cube (a lane
        # on the floor in another cube's shadow): zero or the leaf of an instance that is not the tall cube
        others = {0} | {s.shadow_hint_code(k) for k in range(7) if k != TALL}
        left = set(int(v) for v in s.shadow_hints()[LOW].ravel())
        assert left <= others and s.shadow_hint_code(TALL) not in left, (left, others)
    finally:
        for sc in (s, o):
            sc.set_trans(TALL, pos=TALL_POS)
        s.shadow_hints_fill(0)


def test_refractive_scene_takes_no_hints(gpu, oracle):
    """NS > 0 (a refractive material: no occlusion early exit): no query is counted or seeded, whatever the table holds."""
    t = Twin(gpu, oracle)
    ic.build(t, "two_slabs", depth=2)
    s, o = t.gpu, t.orc
    of = orc_render(oracle, o)
    base = s.render(spp=1, want=WANT, stats=False)
    assert s.last_trace()["ns_bucket"] > 0
    for v in (0, 1, 2, 3, 4, -1):
        s.shadow_hints_fill(v)
        f = s.render(spp=1, want=WANT, stats=False)
        _bits_equal(f, base, v)
        c = s.shadow_hint_counters()
        assert (c["queries"], c["seeded"], c["ended"]) == (0, 0, 0), (v, c)
    assert_frames_equal(base, of, ctx="two_slabs", max_pm1=0)


def test_teeth_warm_half_shadow(twins):
    """On the warm static scene the seed ends whole wave queries; with the switch off nothing is seeded."""
    s, _ = twins("point")
    s.set_shadow_hints(True)
    s.shadow_hints_fill(0)
    _frame(s, spp=8)
    cold = s.shadow_hint_counters()
    _frame(s, spp=8)
    warm = s.shadow_hint_counters()
    ended_warm = warm["ended"] - cold["ended"]
    assert ended_warm > 0 and ended_warm >= cold["ended"], (cold, warm)
    s.set_shadow_hints(False)
    s.shadow_hints_fill(0)
    _frame(s, spp=8)
    c = s.shadow_hint_counters()
    assert (c["queries"], c["seeded"], c["ended"]) == (0, 0, 0), c
    s.set_shadow_hints(True)
