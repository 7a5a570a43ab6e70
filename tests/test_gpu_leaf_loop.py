"""The leaf visit's triangle loops (rt_kernels.hip cast_local): the axis-plane loop of the fast
kernels -- one structured body per triangle, the twin skip as a scalar step at the latch, the plane
time and in-plane reject specialised per axis (rt_math.h axis_plane_pass / axis_inplane_reject),
general triangles through the same inside test -- and the filtered loop of the other kernels.
The tests that run, their order and their arithmetic are the reference's: every frame of the fast
kernel equals the counted kernel's bit for bit and the oracle's (hit ids exact), pixel queries of a
few waves return the counted walk's bits, and the profiling variant's triangle-iteration and
inside-test counts are the ones recorded before the loop was restructured
(tests/golden/leaf_loop_work.json).  The host twin is tests/test_leaf_loop_host.py.

Scenes: `mixed` is a box with a pyramid roof whose 14 triangles interleave twin pairs, single
axis-plane triangles of all three axes and tilted triangles, so that consecutive iterations change
axis and enter and leave the general arm; cubes stand beside it."""
import ctypes
import json
import os

import numpy as np
import pytest

import query_cases as qc
from conftest import GOLDEN
from kernel_recipes import DOWN45, M_AXIS, M_BRUTE, M_PROF, M_STATS
from twin import Twin, assert_frames_equal, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
QKEYS = ("t", "inst", "tri", "uv")
SIZE = (64, 48)
DOWN90 = (0.70710678, 0.0, 0.0, 0.70710678)       # forward (0, 0, 1) turned straight down
WORK_GOLDEN = os.path.join(GOLDEN, "leaf_loop_work.json")
WORK_SPP = 2


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def fast_counted_oracle(s, o, oracle, spp, ctx, axis=True):
    """fast frame == counted frame (bits) == oracle (the parity bar); the fast kernel is an AXIS
    kernel (or, axis=False, is not).  Returns the counted frame."""
    fast = s.render(spp=spp, want=WANT, stats=False)
    assert bool(s.last_trace()["mode"] & M_AXIS) == axis, (ctx, s.last_trace())
    full = s.render(spp=spp, want=WANT, stats=True)
    assert s.last_trace()["mode"] & M_STATS, ctx
    for k in WANT:
        assert np.array_equal(bits(fast[k]), bits(full[k])), (ctx, k, int((bits(fast[k]) != bits(full[k])).sum()))
    assert_frames_equal(fast, orc_render(oracle, o, spp=spp), ctx=ctx)
    return full


def pixel_waves(s, o, oracle, pix, ctx):
    """A pixel batch of a few waves through rt_query: the fast walk's t, inst, tri, u, v are the
    counted walk's bits, and the ids are the oracle's primary hits at those pixels."""
    q = s.query(pixels=pix, want=QKEYS)
    qs = s.query(pixels=pix, want=QKEYS, stats=True)
    for k in QKEYS:
        assert np.array_equal(bits(q[k]), bits(qs[k])), (ctx, k)
    of = orc_render(oracle, o, spp=1, want=("hit_inst", "hit_tri"))
    assert np.array_equal(q["inst"], of["hit_inst"][pix[:, 1], pix[:, 0]]), ctx
    assert np.array_equal(q["tri"], of["hit_tri"][pix[:, 1], pix[:, 0]]), ctx
    return q


# ---- scenes -------------------------------------------------------------------------------------
def _materials(rt):
    m = rt.material
    return (m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.6, 0.3, 0.1, 1), Ks=(0.3, 0.3, 0.3, 1), alpha=4.0),
            m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.2, 0.5, 0.6, 1), Ks=(0.4, 0.4, 0.4, 1), Kr=(0.5, 0.5, 0.5, 1), alpha=6.0))


MIXED_ORDER = ("CGA", "AGE",      # -x: a twin pair
               "AEP",             # roof (tilted)
               "DBH",             # +x, first half: single (the next triangle lies on another axis)
               "DAB", "CAD",      # -z: a twin pair
               "BFH",             # +x, second half: single
               "EFP", "FBP",      # roof, twice
               "GCD", "DHG",      # -y: a twin pair
               "GHE",             # +z, first half: single
               "BAP",             # roof
               "EHF")             # +z, second half: single, last of the list
MIXED_AXES = (0, 0, 3, 0, 2, 2, 0, 3, 3, 1, 1, 2, 3, 2)


def _mixed_mesh(b, scale, mat):
    c = dict(A=(-.5, .5, -.5), B=(.5, .5, -.5), C=(-.5, -.5, -.5), D=(.5, -.5, -.5),
             E=(-.5, .5, .5), F=(.5, .5, .5), G=(-.5, -.5, .5), H=(.5, -.5, .5), P=(0.0, 1.0, 0.0))
    v = {k: b.add_vertex(*[scale * x for x in p]) for k, p in c.items()}
    mesh = b.create_mesh()
    for tri in MIXED_ORDER:
        b.add_triangle(mesh, v[tri[0]], v[tri[1]], v[tri[2]], mat)
    return mesh


def _finish(b, cam_pos, cam_quat, depth=2, lights=True):
    if lights:
        b.add_point_light((0.5, 6.0, -2.0), (1.0, 1.0, 1.0, 1.0))
        b.add_directional_light((0.3, -1.0, 0.8), (0.6, 0.6, 0.5, 1.0))
    b.finish(SIZE[0], SIZE[1], 60.0, 100.0, cam_pos=cam_pos, cam_quat=cam_quat, dist_atten=(0.1, 0.05, 0.01),
             ambience=(0.3, 0.3, 0.3, 1.0), depth=depth)
    return b.gpu, b.orc


def mixed_scene(rt, oracle, rotated=False):
    """Six roofed boxes and six cubes on a 4 x 3 board, a mirror material on every other one."""
    b = Twin(rt, oracle)
    matte, shiny = _materials(rt)
    meshes = [_mixed_mesh(b, 0.8, matte), b.build_cube(0.7, shiny), _mixed_mesh(b, 0.6, shiny), b.build_cube(0.9, matte)]
    for k in range(12):
        x, z = k % 4, k // 4
        quat = (0.0, 0.38268343, 0.0, 0.92387953) if rotated and k == 5 else (0, 0, 0, 1)
        b.set_trans(b.add_trans(meshes[(k + z) % 4]), pos=(-1.8 + 1.2 * x, 0.1 * (k % 3), -0.2 + 1.2 * z), quat=quat)
    return _finish(b, (0.1, 4.2, -3.4), DOWN45)


@pytest.fixture(scope="module")
def mixed(gpu, oracle):
    return mixed_scene(gpu, oracle)


def cubes_scene(rt, oracle, places, cam_pos, cam_quat, scales=(1.0,), depth=2, lights=True):
    b = Twin(rt, oracle)
    mats = _materials(rt)
    meshes = [b.build_cube(sc, mats[k % 2]) for k, sc in enumerate(scales)]
    for k, (mesh, pos) in enumerate(places):
        b.set_trans(b.add_trans(meshes[mesh]), pos=pos)
    return _finish(b, cam_pos, cam_quat, depth=depth, lights=lights)


# ---- 1. one mesh of every kind of triangle --------------------------------------------------------
def test_mixed_triangle_list(gpu, oracle, mixed):
    s, o = mixed
    ax = list(MIXED_AXES)
    assert any(ax[i] != ax[i + 1] for i in range(13)) and ax.count(3) == 4 and {0, 1, 2} <= set(ax)
    full = fast_counted_oracle(s, o, oracle, 2, "mixed")
    hit = full["hit_inst"] >= 0
    assert 0.3 < hit.mean() < 1.0
    # tilted and axis-plane triangles of the roofed boxes are both in the frame
    assert s.info()["n_tris"] == 2 * 14 + 2 * 12
    seen = set(int(t) for t in np.unique(full["hit_tri"][hit]))
    roof = {k * 26 + i for k in (0, 1) for i, a in enumerate(MIXED_AXES) if a == 3}     # meshes 0 and 2: 14 + 12 apart
    walls = {k * 26 + i for k in (0, 1) for i, a in enumerate(MIXED_AXES) if a != 3}
    assert len(seen & roof) >= 4 and len(seen & walls) >= 4, sorted(seen)


# ---- 2. waves whose lanes disagree ----------------------------------------------------------------
def test_lanes_disagree_on_a_twins_plane_time(gpu, oracle):
    """Two cubes, the near one covering the left half of the far one as seen from the camera: in a
    wave across the near cube's silhouette, the lanes that hit it hold a t_best below the far
    faces' plane times, the others do not -- the far twins' skip is taken only when no lane passes.
    Pixel queries of the waves across the silhouette, and whole frames."""
    s, o = cubes_scene(gpu, oracle, [(0, (-0.5, 0.0, 0.0)), (0, (0.3, 0.2, 1.6))], (0.0, 1.2, -4.0), (0.1305262, 0.0, 0.0, 0.9914449))
    full = fast_counted_oracle(s, o, oracle, 1, "silhouette")
    hi = full["hit_inst"]
    assert (hi == 0).sum() > 100 and (hi == 1).sum() > 50
    # rows through both cubes: 64-pixel batches (one wave each) that hold both instances and the sky
    rows = [y for y in range(SIZE[1]) if {0, 1} <= set(hi[y].tolist())]
    assert len(rows) >= 3
    pix = np.array([(x, y) for y in rows[:3] for x in range(SIZE[0])], np.int32)
    q = pixel_waves(s, o, oracle, pix, "silhouette rows")
    for w in range(3):
        assert {0, 1} <= set(q["inst"][64 * w:64 * w + 64].tolist())


def test_one_lane_alone_is_a_candidate(gpu, oracle):
    """A cube smaller than a pixel on one pixel's ray: of its wave, that lane alone passes the
    in-plane reject (the others' crossings lie within `win` of the triangle, outside its box)."""
    px, py = 37, 20
    b = Twin(gpu, oracle)
    matte, shiny = _materials(gpu)
    tiny, big = b.build_cube(0.01, shiny), b.build_cube(1.0, matte)
    b.set_trans(b.add_trans(big), pos=(-1.5, -1.0, 3.0))
    k = b.add_trans(tiny)
    s, o = _finish(b, (0.0, 0.5, -2.0), (0, 0, 0, 1))
    ray = qc.camera_rays(s.export("camera"), np.array([(px, py)], np.int32))[0]
    pos = [float(ray[i] + np.float32(2.5) * ray[3 + i]) for i in range(3)]
    s.set_trans(k, pos=pos)
    o.set_trans(k, pos=pos)
    full = fast_counted_oracle(s, o, oracle, 1, "tiny cube")
    assert (full["hit_inst"] == k).sum() == 1 and full["hit_inst"][py, px] == k
    y0 = py - py % 4
    pix = np.array([(x, y) for y in range(y0, y0 + 4) for x in range(32, 48)], np.int32)      # one wave around the pixel
    q = pixel_waves(s, o, oracle, pix, "tiny cube, one wave")
    assert (q["inst"] == k).sum() == 1


# ---- 3. cameras on face planes and edges ----------------------------------------------------------
D1 = float(np.sqrt(2.0))           # a unit cube's longest triangle edge: off = 1e-4 D, win = 1e3 D
ON_PLANES = [
    ("top face plane", (0.0, 0.5, -3.0)),
    ("top face plane, inside off", (0.0, 0.5 + 0.5e-4 * D1, -3.0)),
    ("top face plane, below, inside off", (0.0, 0.5 - 0.5e-4 * D1, -3.0)),
    ("top face plane, past off", (0.0, 0.5 + 2e-4 * D1, -3.0)),
    ("side face plane", (0.5, 0.2, -3.0)),
    ("edge line", (0.5, 0.5, -3.0)),
    ("edge line of the far cube, beside the near one", (1.7, 0.7, -3.0)),
    ("front face plane", (-2.0, 0.1, -0.5)),
]


@pytest.mark.parametrize("name,cam", ON_PLANES, ids=[n for n, _ in ON_PLANES])
def test_cameras_on_face_planes_and_edges(gpu, oracle, name, cam):
    """The eye in a face's plane (plane time 0, or a crossing within `off` of the plane) and on an
    edge's line: rays graze the faces, crossings fall just outside the triangles' boxes (the
    reject window 0 < e <= win, |p_ax - a_ax| <= off) and on their edges."""
    quat = (0, 0, 0, 1) if cam[2] < -1 else (0.0, 0.70710678, 0.0, 0.70710678)      # along +z, or along +x
    s, o = cubes_scene(gpu, oracle, [(0, (0.0, 0.0, 0.0)), (0, (1.2, 0.2, 1.5)), (0, (-1.0, 0.5, 3.0))], cam, quat)
    full = fast_counted_oracle(s, o, oracle, 2, name)
    assert (full["hit_inst"] >= 0).sum() > 50


# ---- 4. ties --------------------------------------------------------------------------------------
def test_rays_through_a_faces_diagonal(gpu, oracle):
    """Straight down on a cube from above its centre: the pixels with |x - W/2| == |y - H/2| look
    along a diagonal of the top face; on the face's own diagonal both twins are hit at the same t
    and the first of the list wins (the strict < against t_best)."""
    s, o = cubes_scene(gpu, oracle, [(0, (0.0, 0.0, 0.0)), (0, (10.0, -2.0, 0.0))], (0.0, 3.0, 0.0), DOWN90, depth=0)
    full = fast_counted_oracle(s, o, oracle, 1, "diagonal")
    W, H = SIZE
    y, x = np.mgrid[0:H, 0:W]
    tri, hit = full["hit_tri"], full["hit_inst"] >= 0
    ids = sorted(int(t) for t in np.unique(tri[hit]))
    assert len(ids) == 2 and ids[1] == ids[0] + 1          # the top face's twins
    for sign in (1, -1):
        d = hit & ((x - W // 2) == sign * (y - H // 2))
        assert d.sum() >= 8
        both = set(tri[d].tolist())
        if both == {ids[0]}:
            break
    else:
        raise AssertionError("no diagonal on which the first twin wins every pixel")
    q = pixel_waves(s, o, oracle, np.stack([x[d], y[d]], axis=1).astype(np.int32), "diagonal pixels")
    assert set(q["tri"].tolist()) == {ids[0]}


def test_two_coincident_cubes(gpu, oracle):
    """Two instances of one cube in one place (every hit a tie between them) beside a third."""
    s, o = cubes_scene(gpu, oracle, [(0, (0.0, 0.0, 0.0)), (0, (0.0, 0.0, 0.0)), (0, (1.4, 0.3, 0.8))],
                       (0.3, 2.5, -3.0), DOWN45)
    full = fast_counted_oracle(s, o, oracle, 2, "coincident")
    assert (full["hit_inst"] >= 0).sum() > 200
    assert ((full["hit_inst"] == 0) | (full["hit_inst"] == 1)).sum() > 100


# ---- 5. the other loops and variants ----------------------------------------------------------------
def test_rotated_instance_takes_the_filtered_loop(gpu, oracle):
    s, o = mixed_scene(gpu, oracle, rotated=True)
    full = fast_counted_oracle(s, o, oracle, 2, "rotated", axis=False)
    assert (full["hit_inst"] == 5).sum() > 20


def test_brute_force_frame(gpu, oracle, mixed):
    s, o = mixed
    fast = s.render(spp=2, want=WANT, stats=False, use_bvh=False)
    assert s.last_trace()["mode"] & M_BRUTE and s.last_trace()["mode"] & M_AXIS
    full = s.render(spp=2, want=WANT, stats=True, use_bvh=False)
    for k in WANT:
        assert np.array_equal(bits(fast[k]), bits(full[k])), k
    assert_frames_equal(fast, orc_render(oracle, o, spp=2, use_bvh=0), ctx="brute")


def _prof_counts(rt, s, spp):
    """tools/tri_work.py's counters of one frame of the profiling variant (rt_experiment 6)."""
    L = rt.lib()
    L.rt_experiment.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                ctypes.c_void_p]
    c = np.zeros(64, np.uint64)
    ms = ctypes.c_double()
    rt._check(L.rt_experiment(s._h, 6, spp, 1, ctypes.byref(ms), c.ctypes.data))
    names = {0: "queries", 2: "leaf_lanes", 4: "wave_queries", 5: "pair_steps", 6: "leaf_visits", 7: "tri_iters",
             13: "inside_tests_wave", 14: "inside_tests_lanes"}
    return {v: int(c[k]) for k, v in names.items()}


def test_profiling_variant_frame_and_counts(gpu, oracle, mixed):
    """The profiling variant renders the fast frame, and on this scene its triangle iterations
    and inside tests (wave level and lane level) are the ones recorded from the loop's earlier
    form: the same tests run, the twin skip included."""
    s, o = mixed
    fast = s.render(spp=WORK_SPP, want=("rgba",), stats=False)
    w, rgba = s.frame_work(spp=WORK_SPP, compact=False, want_rgba=True)
    assert s.last_trace()["mode"] & M_PROF
    assert np.array_equal(rgba, fast["rgba"])
    got = _prof_counts(gpu, s, WORK_SPP)
    print("leaf loop work:", json.dumps(got))
    assert got["tri_iters"] == w["tri_iters"] and got["leaf_visits"] == w["leaf_visits"]
    want = json.load(open(WORK_GOLDEN))
    assert got["inside_tests_wave"] > 0 and got["tri_iters"] > got["inside_tests_wave"]
    for k in ("queries", "leaf_lanes", "wave_queries", "pair_steps", "leaf_visits", "tri_iters", "inside_tests_wave",
              "inside_tests_lanes"):
        assert got[k] == want[k], (k, got[k], want[k])
