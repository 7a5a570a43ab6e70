"""The unit-length fast path of the trace and query kernels (rt_math.h unit_len_rcp; rt_kernels.hip
dir_pre, hit_normal, the reflection child's ray): one wave vote per chain, on its first squared
length (unit_head), between the closed forms and the generic sqrt / division chain.  Frames of the fast kernel equal the counted
kernel's bit for bit and the oracle's (twin.assert_frames_equal), on frames where every wave
takes the fast form (cube worlds: primary, reflection and both lights' shadow queries), where a
wave must take the generic one (interpolated normals of a mesh with unequal vertex normals), and
where both alternate.  The host twin is tests/test_unitlen_host.py."""
import numpy as np
import pytest

from conftest import scene_path
from twin import Twin, assert_frames_equal, mirror_camera, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
QALL = ("t", "inst", "tri", "uv", "normal", "hit", "rays_out")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def fast_counted_oracle(s, o, oracle, spp, ctx):
    """fast frame == counted frame (bits) == oracle (the parity bar); returns the counted frame."""
    fast = s.render(spp=spp, want=WANT, stats=False)
    full = s.render(spp=spp, want=WANT, stats=True)
    for k in WANT:
        assert np.array_equal(bits(fast[k]), bits(full[k])), (ctx, k)
    assert_frames_equal(fast, orc_render(oracle, o, spp=spp), ctx=ctx)
    return full


def query_fast_counted_oracle(s, o, oracle, ctx):
    """rt_query's pixel mode (the same dir_pre and hit_normal): fast == counted bit for bit,
    ids == the oracle's primary hits."""
    W, H = s.width, s.height
    pix = np.stack(np.meshgrid(np.arange(W), np.arange(H)), axis=-1).reshape(-1, 2).astype(np.int32)
    q = s.query(pixels=pix, want=QALL)
    qs = s.query(pixels=pix, want=QALL, stats=True)
    for k in QALL:
        assert np.array_equal(bits(q[k]), bits(qs[k])), (ctx, k)
    of = orc_render(oracle, o, spp=1, want=("hit_inst", "hit_tri"))
    assert np.array_equal(q["inst"], of["hit_inst"].ravel()), ctx
    assert np.array_equal(q["tri"], of["hit_tri"].ravel()), ctx
    return q


@pytest.mark.parametrize("w,h,spp", [(96, 64, 8), (160, 120, 1)])
def test_cube_world_frames(gpu, oracle, w, h, spp):
    """world8_stress (identity poses, equal vertex normals, mirrors, a point and a directional
    light): every chain of every wave is inside the window."""
    s = gpu.Scene.load_json(scene_path("world8_stress"), w, h)
    o = oracle.load(scene_path("world8_stress"), w, h)
    info = s.info()
    assert info["n_lights"] == 2 and info["depth"] > 0
    full = fast_counted_oracle(s, o, oracle, spp, (w, h, spp))
    assert 0.1 < (full["hit_inst"] >= 0).mean() < 1.0                # cubes and sky
    if (w, h) == (96, 64):
        q = query_fast_counted_oracle(s, o, oracle, "pixel query")
        hit = q["hit"] != 0
        n = q["normal"][hit].astype(np.float64)
        assert hit.sum() > 500 and np.abs((n * n).sum(axis=1) - 1.0).max() < 1e-6


def test_axis_aligned_camera(gpu, oracle):
    """The camera looks exactly along +z from inside and in front of the cube field: the centre
    column and row carry zero direction components (+0 and -0 squares in the lengths, NaN lanes of
    axis_inv), next to ordinary rays."""
    s = gpu.Scene.load_json(scene_path("world8_stress"), 160, 120)
    o = oracle.load(scene_path("world8_stress"), 160, 120)
    for pos in ([0.5, 3.0, -12.0], [0.4995, 3.4995, -8.0]):
        s.set_camera(pos, [0.0, 0.0, 0.0, 1.0])
        mirror_camera(s, o)
        rays = s.query(pixels=[(80, 60), (80, 7), (3, 60)], want=("rays_out",))["rays_out"]
        assert rays[0, 3] == 0.0 and rays[0, 4] == 0.0 and rays[1, 3] == 0.0 and rays[2, 4] == 0.0
        full = fast_counted_oracle(s, o, oracle, 2, pos)
        assert (full["hit_inst"] >= 0).mean() > 0.05, pos


# ---- built scenes: meshes whose vertex normals differ ------------------------------------------
def _octahedron(b, r, mat):
    """Eight faces on six shared vertices: the generated vertex normals are the axes, every face
    interpolates between three different ones (|n| down to 1/sqrt(3): far outside the window)."""
    v = [b.add_vertex(*p) for p in ((r, 0, 0), (-r, 0, 0), (0, r, 0), (0, -r, 0), (0, 0, r), (0, 0, -r))]
    m = b.create_mesh()
    for i, j, k in ((0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)):
        b.add_triangle(m, v[i], v[j], v[k], mat)
    return m


def _built(rt, oracle, size, with_cubes):
    b = Twin(rt, oracle)
    m = rt.material
    shiny = m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.2, 0.5, 0.6, 1), Ks=(0.4, 0.4, 0.4, 1), Kr=(0.5, 0.5, 0.5, 1), alpha=6.0)
    matte = m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.6, 0.3, 0.1, 1), Ks=(0.3, 0.3, 0.3, 1), alpha=4.0)
    octa = _octahedron(b, 0.45, shiny)
    cube = b.build_cube(0.6, matte) if with_cubes else None
    mirror = b.build_cube(0.6, shiny) if with_cubes else None
    for k in range(24):                                    # a 6 x 4 field, 0.8 apart: neighbours differ
        x, z = k % 6, k // 6
        mesh = octa if (not with_cubes or (x + z) % 2 == 0) else (cube if k % 3 else mirror)
        b.set_trans(b.add_trans(mesh), pos=(-2.0 + 0.8 * x, 0.15 * (k % 3), -0.4 + 0.8 * z), quat=(0, 0, 0, 1))
    b.add_point_light((0.5, 6.0, -2.0), (1.0, 1.0, 1.0, 1.0))
    b.add_directional_light((0.0, -1.0, 1.0), (0.6, 0.6, 0.5, 1.0))
    b.finish(size[0], size[1], 60.0, 100.0, cam_pos=(0.1, 4.0, -3.6), cam_quat=(0.3826834, 0.0, 0.0, 0.9238795),
             dist_atten=(0.1, 0.05, 0.01), ambience=(0.3, 0.3, 0.3, 1.0), depth=2)
    return b.gpu, b.orc


@pytest.mark.parametrize("with_cubes", [False, True], ids=["octahedra", "octahedra_and_cubes"])
def test_interpolated_normals_take_the_generic_chain(gpu, oracle, with_cubes):
    """Octahedra alone: every wave with a hit fails hit_normal's vote.
    Octahedra and cubes on a checkerboard seen at 64 x 48: most 4 x 2 pixel groups straddle both,
    so waves of either kind, and waves voting the generic chain for a few lanes, alternate."""
    size = (64, 48)
    s, o = _built(gpu, oracle, size, with_cubes)
    full = fast_counted_oracle(s, o, oracle, 2, with_cubes)
    q = query_fast_counted_oracle(s, o, oracle, with_cubes)
    hit = q["hit"] != 0
    assert hit.sum() > 600
    # octahedron faces show by normals that vary over the face, cube faces by one normal each
    inst, tri, nrm = q["inst"][hit], q["tri"][hit], q["normal"][hit]
    varying = flat = 0
    for key in {(int(i), int(t)) for i, t in zip(inst, tri)}:
        n = nrm[(inst == key[0]) & (tri == key[1])]
        if len(n) >= 2:
            if np.ptp(n, axis=0).max() > 1e-3:
                varying += 1
            elif np.ptp(n, axis=0).max() == 0.0:
                flat += 1
    assert varying >= 10                                   # interpolated normals: the generic chain ran
    if with_cubes:
        assert flat >= 10                                  # cube faces: one normal per face
        hi = full["hit_inst"].reshape(size[1], size[0])
        groups = hi.reshape(size[1] // 2, 2, size[0] // 4, 4).transpose(0, 2, 1, 3).reshape(-1, 8)
        mixed = sum(1 for g in groups if len({int(i) for i in g if i >= 0}) >= 2)
        assert mixed >= 20                                 # groups seeing more than one instance
