"""The per-frame BVH build on the device against the oracle, node for node.

Scene.export("bvh_*") (RT_EXPORT_BVH_*, a read-back of the built tree) returns the three arrays
every frame and ray query starts from: the heap's child-pair boxes, the leaf -> instance map and
the ordered radix tree of the fast kernels.  bvh_cases.Expected computes all three from the
oracle's BVH alone.  The matrix (bvh_cases.CASES) sits on both sides of every switch of the build
-- LDS bitonic / chunked rank sort / shuffle bitonic / tree in HBM / grid-wide with hipCUB's
sort -- with tied Morton keys (lattice, one_point), rotated boxes (scattered) and degenerate real
instances (an empty mesh: n_real < n_inst), none of which the scene files have.
tests/test_bvh_host.py checks on the CPU that each case has the ties and counts it is run for.

Heap boxes, leaf map and the ordered tree's references must be equal bit for bit; the ordered
tree's boxes as float values (the device groups a range's min / max differently from numpy, which
can only change the sign of a zero)."""
import numpy as np
import pytest

import bvh_cases as bc
import query_cases as qc
from twin import Twin, assert_frames_equal, mirror_instances, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")


@pytest.mark.parametrize("case", bc.CASES, ids=bc.case_id)
def test_built_tree_equals_the_oracles(gpu, oracle, case):
    n_inst, placement, rule = case
    tw = Twin(gpu, oracle)
    bc.build(tw, n_inst, placement, rule)
    exp = bc.Expected(oracle, tw.orc)
    tw.gpu.render(spp=1, stats=False)                            # one 8 x 8 frame builds the tree
    info = bc.check_export(tw.gpu, exp, ctx=bc.case_id(case))
    assert info["slot"] == 0
    # a short buffer is an argument error, as for the other exports
    buf = np.zeros(8, np.int32)
    export = gpu.lib().rt_scene_export
    assert export(tw.gpu._h, gpu.BVH_EXPORTS["bvh_info"], buf.ctypes.data, 31) == gpu.RT_ERR_ARG
    assert export(tw.gpu._h, gpu.BVH_EXPORTS["bvh_pairs"], buf.ctypes.data, 48 * exp.n_leaf - 1) == gpu.RT_ERR_ARG
    assert export(tw.gpu._h, gpu.BVH_EXPORTS["bvh_leaf_inst"], buf.ctypes.data, 4 * exp.n_leaf - 1) == gpu.RT_ERR_ARG
    if exp.n_real >= 2:
        assert export(tw.gpu._h, gpu.BVH_EXPORTS["bvh_fnode"], buf.ctypes.data, 64 * (exp.n_real - 1) - 1) == gpu.RT_ERR_ARG
    # the counted frame after the read-back is the frame before it (the hook changes nothing)
    if n_inst <= 70:
        a = tw.gpu.render(spp=1, want=WANT, stats=True)
        tw.gpu.export("bvh_fnode")
        b = tw.gpu.render(spp=1, want=WANT, stats=True)
        for k in WANT:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        assert {k: a["stats"][k] for k in ("rays", "nodes", "leaves", "tri_tests")} == \
               {k: b["stats"][k] for k in ("rays", "nodes", "leaves", "tri_tests")}


@pytest.mark.parametrize("n_inst", bc.MOVING)
def test_moving_instances_with_frames_in_flight(gpu, oracle, n_inst):
    """Three frame slots; before each of four frames a tenth of the instances move onto other
    instances' centres.  After each frame the slot that built holds the oracle's tree for those
    poses: per-slot trees and sort scratch, and the regenerated n_real / fdepth."""
    tw = Twin(gpu, oracle)
    L = bc.build(tw, n_inst)
    tw.gpu.set_frame_slots(3)
    slots = []
    for frame in range(4):
        bc.move_tenth(tw.gpu, L, frame)
        mirror_instances(tw.gpu, tw.orc)
        tw.gpu.render(spp=1, stats=False)
        info = bc.check_export(tw.gpu, bc.Expected(oracle, tw.orc), ctx="frame %d" % frame)
        slots.append(info["slot"])
    assert len(set(slots[:3])) == 3 and slots[3] == slots[0], slots


@pytest.fixture(scope="module", params=bc.RAY_SCENES)
def ray_scene(request, gpu, oracle):
    """(twin, oracle frame, oracle frame with use_bvh = 0 at 70 instances): computed once."""
    tw = Twin(gpu, oracle)
    L = bc.build(tw, request.param, width=96, height=64, lit=True)
    of = orc_render(oracle, tw.orc, spp=1)
    brute = orc_render(oracle, tw.orc, spp=1, use_bvh=0) if request.param == 70 else None
    return tw, L, of, brute


def test_frames_over_tied_leaves(gpu, oracle, ray_scene):
    """Counted and fast frames of the lattice scenes (stacked and duplicated cubes, a point light,
    reflective materials at depth 2): which of two coincident instances wins a hit at equal t is
    decided by the order in which the leaves are met."""
    tw, L, of, brute = ray_scene
    share, hit = bc.coincident_hit_share(L, of["hit_inst"])
    assert hit >= 0.2 and share >= 0.05, (hit, share)
    full = tw.gpu.render(spp=1, want=WANT, stats=True)
    assert_frames_equal(full, of, ctx="counted")
    st = full["stats"]
    assert (st["rays"], st["nodes"], st["leaves"], st["tri_tests"]) == tuple(int(x) for x in of["stats"])
    fast = tw.gpu.render(spp=1, want=WANT, stats=False)
    assert tw.gpu.last_trace()["ftree"] == 1                     # the ordered tree was walked
    assert_frames_equal(fast, of, ctx="fast")
    if brute is not None:
        for stats in (True, False):
            fr = tw.gpu.render(spp=1, use_bvh=False, want=WANT, stats=stats)
            assert_frames_equal(fr, brute, ctx="use_bvh=0, stats=%s" % stats)
            if stats:
                st = fr["stats"]
                assert (st["rays"], st["nodes"], st["leaves"], st["tri_tests"]) == tuple(int(x) for x in brute["stats"])
    tw.gpu.render(spp=1, stats=False)
    bc.check_export(tw.gpu, bc.Expected(oracle, tw.orc), ctx="ray scene")     # and the tree these frames walked


def test_queries_over_tied_leaves(gpu, oracle, ray_scene):
    tw, L, of, _ = ray_scene
    pix = qc.all_pixels(96, 64)
    inst, tri = of["hit_inst"].ravel(), of["hit_tri"].ravel()
    for kw in ({}, {"reorder": True}, {"stats": True}):
        q = tw.gpu.query(pixels=pix, want=("inst", "tri"), **kw)
        assert np.array_equal(q["inst"], inst), (kw, int((q["inst"] != inst).sum()))
        assert np.array_equal(q["tri"], tri), (kw, int((q["tri"] != tri).sum()))
