"""The unit-length closed forms of the shading steps' chains in the trace kernels (rt_kernels.hip
trace_sample: the hit's unit normal, the light step's |dtl| / phong reflection / shadow-ray
constructor, the reflection step's reflect; rt_math.h reflect_unit, reflect_pre_unit), each on one
wave vote, and cast_local's general-pose arm as a compile-time choice (AXIS kernels) or a kept arm
(the others).  Device KATs run the voted forms on waves of unit, non-unit and mixed lanes against
the generic functions; frames of the fast kernel equal the counted kernel's bit for bit and the
oracle's where every light-step vote passes (a point light), fails (a directional light) and
alternates (both), and with a rotated instance (no AXIS kernel).  The host twin is
tests/test_unitlen_shade_host.py."""
import numpy as np
import pytest

from conftest import scene_path
from test_gpu_unitlen import _octahedron
from twin import Twin, assert_frames_equal, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
N = 4096
f32 = np.float32


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


# ---- device KATs -------------------------------------------------------------------------------
def _dot(a, b):                                            # rt_math.h dot: 0 + x x + y y + z z, in f32
    s = np.zeros(len(a), f32)
    for k in range(3):
        s = (s + a[:, k] * b[:, k]).astype(f32)
    return s


def _vectors(seed):
    """4,096 vectors = 64 waves of 64 consecutive elements: waves 0-15 unit (a few ulps), 16-31
    anything but unit (scaled, zero, near zero), 32-63 unit with 1-32 lanes that are not, so that
    the closed arm, the generic arm and a vote failed by a few lanes all run.  Some unit lanes sit
    at the edges of the vote's window."""
    g = np.random.default_rng(seed)
    v = g.standard_normal((N, 3)).astype(f32)
    v[::7, 0] = 0.0
    v[::11, 1] = -0.0
    v[5::16] = np.eye(3, dtype=f32)[g.integers(0, 3, len(v[5::16]))] * f32(-1.0)
    n = np.sqrt(_dot(v, v))
    v = (v / n[:, None]).astype(f32)
    # waves 8-11: heads spread inside unit_head's window (|v|^2 - 1 = k 2^-24 within 2^-16, less
    # 8 x 2^-24 of rounding room); waves 12-15: across both of its edges, so a few lanes fail the vote
    k = np.zeros(N)
    k[8 * 64:12 * 64] = g.integers(-248, 249, 4 * 64)
    k[12 * 64:16 * 64] = g.integers(-300, 301, 4 * 64)
    v = (v * (f32(1.0) + k.astype(f32) * f32(2.0 ** -25))[:, None]).astype(f32)
    scale = np.exp2(g.uniform(-20.0, 20.0, N)).astype(f32)
    scale[np.abs(scale - 1.0) < 1e-3] = f32(2.0)
    off = np.zeros(N, bool)
    off[16 * 64:32 * 64] = True
    for w in range(32, 64):
        lanes = g.choice(64, size=w - 31, replace=False)
        off[w * 64 + lanes] = True
    v[off] = (v[off] * scale[off, None]).astype(f32)
    zero = np.flatnonzero(off)[::9]
    v[zero] = 0.0
    tiny = np.flatnonzero(off)[4::9]
    v[tiny] = (v[tiny] * f32(1e-30)).astype(f32)
    return v, off


def test_kat_normalized_and_len(gpu):
    v, off = _vectors(1)
    assert off[:1024].sum() == 0 and off[1024:2048].all() and 0 < off[2048:].sum() < 2048
    got = gpu.kat_device("normalized_unit", v)
    assert np.array_equal(bits(got), bits(gpu.kat_device("normalize3", v)))
    s = _dot(v, v)
    ln = gpu.kat_device("sqrt_cr", s.reshape(-1, 1))
    rc = gpu.kat_device("rcp_cr", ln)
    got = gpu.kat_device("unit_len_rcp", v)
    assert np.array_equal(bits(got[:, 0]), bits(ln[:, 0]))
    ok = ln[:, 0] > 0                                      # (1 / 0: the kernel never uses it)
    assert np.array_equal(bits(got[ok, 1]), bits(rc[ok, 0]))
    unit = np.abs(s.astype(np.float64) - 1.0) <= 2.0 ** -16
    assert unit[:1024].mean() > 0.8 and (ln[unit, 0] > 0.99).all()


def test_kat_reflect(gpu):
    d, off_d = _vectors(2)
    n, off_n = _vectors(3)
    n[2048:] = np.roll(n[2048:], 64 * 16, axis=0)         # mixed waves of d meet other mixed waves of n
    got = gpu.kat_device("reflect_unit", d, n)
    want = gpu.kat_device("reflect", d, n)
    assert np.array_equal(bits(got), bits(want))
    assert np.isfinite(want[:1024]).all() and np.abs(np.sqrt(_dot(want[:1024], want[:1024])) - 1.0).max() < 1e-3


def test_kat_reflect_pre(gpu):
    """phong's reflection: reflect_pre(d_len, dn, nn) with its one normalisation voted."""
    dn, _ = _vectors(4)
    nn, _ = _vectors(5)
    nn[1024:2048] = _vectors(6)[0][:1024]                  # unit normals against non-unit directions too
    g = np.random.default_rng(7)
    dl = np.where(g.random(N) < 0.5, 1.0, np.exp2(g.uniform(-3, 3, N))).astype(f32).reshape(-1, 1)
    got = gpu.kat_device("reflect_pre_unit", dn, nn, dl)
    c = _dot(dn, nn)
    proj = (nn * c[:, None]).astype(f32)
    w = (dn - (proj * f32(2.0)).astype(f32)).astype(f32)
    with np.errstate(all="ignore"):
        want = (gpu.kat_device("normalize3", w) * dl).astype(f32)
    fin = np.isfinite(w).all(axis=1)                       # (overflowed products: no reference to compare)
    assert fin.mean() > 0.9
    assert np.array_equal(bits(got[fin]), bits(want[fin]))


# ---- frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,spp", [(96, 64, 8), (160, 120, 1)])
def test_cube_world_frames(gpu, oracle, w, h, spp):
    """world8_stress (a point light, a directional light, mirrors; identity poses: the AXIS kernel
    without a general-pose arm; the counted kernel keeps the arm and never enters it)."""
    s = gpu.Scene.load_json(scene_path("world8_stress"), w, h)
    o = oracle.load(scene_path("world8_stress"), w, h)
    info = s.info()
    assert info["n_lights"] == 2 and info["depth"] > 0
    full = fast_counted_oracle(s, o, oracle, spp, (w, h, spp))
    assert 0.1 < (full["hit_inst"] >= 0).mean() < 1.0


def _built(rt, oracle, lights, rotated=False):
    """A 6 x 4 checkerboard of octahedra (interpolated normals: the hit's vote fails), matte cubes
    and mirror cubes under the given lights."""
    b = Twin(rt, oracle)
    m = rt.material
    shiny = m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.2, 0.5, 0.6, 1), Ks=(0.4, 0.4, 0.4, 1), Kr=(0.5, 0.5, 0.5, 1), alpha=6.0)
    matte = m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.6, 0.3, 0.1, 1), Ks=(0.3, 0.3, 0.3, 1), alpha=4.0)
    octa = _octahedron(b, 0.45, shiny)
    cube = b.build_cube(0.6, matte)
    mirror = b.build_cube(0.6, shiny)
    for k in range(24):
        x, z = k % 6, k // 6
        mesh = octa if (x + z) % 2 == 0 else (cube if k % 3 else mirror)
        quat = (0, 0, 0, 1)
        if rotated and k in (7, 9, 14):                    # a mirror cube, a matte cube, an octahedron
            quat = {7: (0.0, 0.3826834, 0.0, 0.9238795), 9: (0.1825742, 0.3651484, 0.5477226, 0.7302967),
                    14: (0.5, 0.5, 0.5, 0.5)}[k]
        b.set_trans(b.add_trans(mesh), pos=(-2.0 + 0.8 * x, 0.15 * (k % 3), -0.4 + 0.8 * z), quat=quat)
    if "point" in lights:
        b.add_point_light((0.5, 6.0, -2.0), (1.0, 1.0, 1.0, 1.0))
    if "directional" in lights:
        b.add_directional_light((0.0, -1.0, 1.0), (0.6, 0.6, 0.5, 1.0))
    b.finish(64, 48, 60.0, 100.0, cam_pos=(0.1, 4.0, -3.6), cam_quat=(0.3826834, 0.0, 0.0, 0.9238795),
             dist_atten=(0.1, 0.05, 0.01), ambience=(0.3, 0.3, 0.3, 1.0), depth=2)
    return b.gpu, b.orc


@pytest.mark.parametrize("lights", [("point",), ("directional",), ("point", "directional")],
                         ids=["point", "directional", "both"])
def test_light_step_votes(gpu, oracle, lights):
    """A point light alone: |dtl|^2 is 1 to a few ulps in every lane, all three votes of the light
    step pass.  A directional light alone: |dtl|^2 = 2, the length vote fails in every wave while
    the other two chains still run closed.  Both: lanes of a wave reach the two lights at different
    times (mirror children, misses), so the length vote alternates."""
    s, o = _built(gpu, oracle, lights)
    assert s.info()["n_lights"] == len(lights)
    full = fast_counted_oracle(s, o, oracle, 2, lights)
    assert (full["hit_inst"] >= 0).mean() > 0.2
    lit = np.asarray(full["radiance"], np.float64).reshape(-1, 4)[:, :3]
    assert (lit > 0.35).mean() > 0.01                      # beyond the ambient term: the lights' terms count


def test_rotated_instances_take_the_general_pose_arm(gpu, oracle):
    """Three rotated instances: no AXIS kernel, cast_local's general-pose arm runs in the fast and
    the counted kernel, and hit_normal's generic chain for their hits."""
    s, o = _built(gpu, oracle, ("point", "directional"), rotated=True)
    full = fast_counted_oracle(s, o, oracle, 2, "rotated")
    hit = set(int(i) for i in np.unique(full["hit_inst"]) if i >= 0)
    assert {7, 9, 14} <= hit                               # the rotated instances are seen
