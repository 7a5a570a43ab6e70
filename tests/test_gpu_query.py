"""Ray queries (rt_query, Scene.query / query_device / pick, rtracer --pick) on the GPU: the closest
hit of caller-supplied rays is the reference's cast_ray -- the oracle's primary hit ids by pixel,
its counters for the counted walk -- whatever the packet a ray travels in, the kernel form (small,
persistent, tree in LDS or global memory, ordered tree, heap, brute force, counted) and the
pointers' side (host, device); values against the reference's own arithmetic; tmax and occlusion;
rejected rays; far axis-parallel rays; and the scene's frame state left alone.

"The same ray" (cases 2, 3, 6).  The kernel normalises every caller direction as rmath::Ray does, and
that normalisation is not idempotent in float32: a unit vector whose squared length rounds below 1
comes back changed in its last bit.  So a ray fed back from rays_out is the same ray only where the
kernel traced the same bits.  The reference result of a caller ray is therefore the origin / dir
query of the whole frame in pixel order (coherent packets, same normalisation); it is tied to the
pixel-mode result on every ray whose fed-back direction is a fixed point of the normalisation
(bit for bit there, and those must be a good part of the frame), and every packet shape, form and
pointer side must reproduce it bit for bit on every ray."""
import os
import subprocess

import numpy as np
import pytest

import query_cases as qc
from conftest import ROOT, scene_path
from kernel_recipes import DOWN45, build_scene
from test_gpu_large import _world
from twin import Twin, assert_frames_equal, orc_render

pytestmark = pytest.mark.gpu
ALL = ("t", "inst", "tri", "uv", "normal", "hit", "rays_out")
CLI = os.path.join(ROOT, "gpu-ray-tracer_amd", "rtracer")
U = 2.0 ** -24                      # float32 unit roundoff


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, keys=ALL, ctx=""):
    for k in keys:
        assert np.array_equal(bits(got[k]), bits(want[k])), (ctx, k, int((bits(got[k]) != bits(want[k])).reshape(len(want[k]), -1).any(axis=1).sum()))


def take(res, idx, keys=ALL):
    return {k: res[k][idx] for k in keys}


def assert_ids_match_oracle(q, of, ctx):
    inst, tri = of["hit_inst"].ravel(), of["hit_tri"].ravel()
    assert np.array_equal(q["inst"], inst), (ctx, int((q["inst"] != inst).sum()))
    assert np.array_equal(q["tri"], tri), (ctx, int((q["tri"] != tri).sum()))
    assert np.array_equal(q["hit"] != 0, inst >= 0), ctx             # the miss pixels match
    assert np.isposinf(q["t"][inst < 0]).all() and np.isfinite(q["t"][inst >= 0]).all(), ctx


# ---- scenes -------------------------------------------------------------------------------------
def _w8(rt, oracle, camera=qc.VALUES_CAMERA):
    W, H = qc.VALUES_SIZE
    s = rt.Scene.load_json(scene_path(qc.VALUES_SCENE), W, H)
    o = oracle.load(scene_path(qc.VALUES_SCENE), W, H)
    if camera:
        s.set_camera(*camera)
        o.set_camera(*s.camera())
    return s, o


def _cubes(rt, oracle, size, places, lights=True, depth=2, cam=((0.1, 4.5, -4.2), DOWN45)):
    """A Twin-built scene of unit cubes at (pos, quat) places."""
    b = Twin(rt, oracle)
    m = rt.material
    meshes = [b.build_cube(1.0, m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.6, 0.3, 0.1, 1), Ks=(0.3, 0.3, 0.3, 1), alpha=4.0)),
              b.build_cube(0.7, m(Ka=(0.1, 0.1, 0.1, 1), Kd=(0.2, 0.5, 0.2, 1), Kr=(0.5, 0.5, 0.5, 1)))]
    for k, (pos, quat) in enumerate(places):
        b.set_trans(b.add_trans(meshes[k % 2]), pos=pos, quat=quat)
    if lights:
        b.add_point_light((0.5, 6.0, -2.0), (1.0, 1.0, 1.0, 1.0))
    b.finish(size[0], size[1], 60.0, 100.0, cam_pos=cam[0], cam_quat=cam[1], dist_atten=(0.1, 0.05, 0.01),
             ambience=(0.3, 0.3, 0.3, 1.0), depth=depth)
    return b.gpu, b.orc


def _rotated12(rt, oracle, size):
    """12 cubes, every one rotated: no identity pose, so neither distance pruning nor the axis-plane path applies."""
    rng = np.random.default_rng(7)
    places = []
    for k in range(12):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        places.append(((-2.4 + 1.6 * (k % 4), 0.2 * (k % 3), -0.5 + 1.6 * (k // 4)), tuple(float(x) for x in q)))
    return _cubes(rt, oracle, size, places)


def _large(rt, oracle, tmp_path, size):
    path = _world(tmp_path, 32, 2, 4.0)                            # > 2048 leaves: the tree stays in global memory
    s, o = rt.Scene.load_json(path, *size), oracle.load(path, *size)
    assert s.info()["n_instances"] >= 2049
    _, q = s.camera()
    s.set_camera([0.0, float(s.camera()[0][1]), -8.0], q)
    o.set_camera(*s.camera())
    return s, o


SCENES = {
    # name: (size, use_bvh, builder(rt, oracle, tmp_path, size))
    "world8_stress": (qc.VALUES_SIZE, True, lambda rt, oracle, tmp, size: _w8(rt, oracle)),
    "world8_stress_own_camera": (qc.VALUES_SIZE, True, lambda rt, oracle, tmp, size: _w8(rt, oracle, None)),
    "world1_brute": ((64, 48), False, lambda rt, oracle, tmp, size: (rt.Scene.load_json(scene_path("world1"), *size),
                                                                     oracle.load(scene_path("world1"), *size))),
    "rotated12": ((64, 48), True, lambda rt, oracle, tmp, size: _rotated12(rt, oracle, size)),
    "one": ((64, 48), True, lambda rt, oracle, tmp, size: build_scene("one", size, rt, oracle, tmp)),
    "two": ((64, 48), True, lambda rt, oracle, tmp, size: build_scene("two", size, rt, oracle, tmp)),
    "chain": ((64, 48), True, lambda rt, oracle, tmp, size: build_scene("chain", size, rt, oracle, tmp)),
    "large": ((64, 48), True, _large),
}


# ---- 1. oracle parity by pixel ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_pixel_queries_match_the_oracle(gpu, oracle, tmp_path, monkeypatch, name):
    size, use_bvh, make = SCENES[name]
    s, o = make(gpu, oracle, tmp_path, size)
    pix = qc.all_pixels(*size)
    of = orc_render(oracle, o, use_bvh=int(use_bvh), spp=1, want=("hit_inst", "hit_tri"))
    assert (of["hit_inst"] >= 0).any(), "the frame needs hits"
    q = s.query(pixels=pix, use_bvh=use_bvh, want=ALL)
    assert_ids_match_oracle(q, of, name)
    # the camera's rays, restated
    assert np.array_equal(bits(q["rays_out"]), bits(qc.camera_rays(s.export("camera"), pix))), name
    # once with stats: the counted reference walk finds the same triangles with the same bits
    qs = s.query(pixels=pix, use_bvh=use_bvh, want=ALL, stats=True)
    assert_same(qs, q, ctx=name + " counted")
    assert qs["stats"]["rays"] == len(pix)
    # the persistent form (one block per CU; the scene image in LDS when it fits) against the small one
    monkeypatch.setenv("RT_QUERY_FORM", "persistent")
    assert_same(s.query(pixels=pix, use_bvh=use_bvh, want=ALL), q, ctx=name + " persistent")
    assert_same(s.query(pixels=pix, use_bvh=use_bvh, want=ALL, stats=True), q, ctx=name + " persistent counted")
    monkeypatch.setenv("RT_QUERY_FORM", "small")
    assert_same(s.query(pixels=pix, use_bvh=use_bvh, want=ALL, rebuild_bvh=False), q, ctx=name + " small, BVH kept")


@pytest.mark.parametrize("use_bvh", [True, False])
def test_counted_query_equals_the_oracles_counters(gpu, oracle, use_bvh):
    """depth = 0 and no lights: the oracle's frame is one cast_ray per pixel, so its four counters
    are the counted query's."""
    size = (64, 48)
    places = [((-0.7, 0.0, 0.0), (0, 0, 0, 1)), ((0.9, 0.5, 1.4), (0, 0, 0, 1)), ((-2.0, 0.3, 1.0), (0, 0, 0, 1)),
              ((2.2, 0.0, 0.4), (0.0, 0.38268343, 0.0, 0.92387953)), ((0.2, 1.1, 2.8), (0, 0, 0, 1))]
    s, o = _cubes(gpu, oracle, size, places, lights=False, depth=0)
    of = orc_render(oracle, o, use_bvh=int(use_bvh), spp=1, want=("hit_inst", "hit_tri"))
    q = s.query(pixels=qc.all_pixels(*size), use_bvh=use_bvh, want=ALL, stats=True)
    assert_ids_match_oracle(q, of, "counted")
    st = q["stats"]
    assert (st["rays"], st["nodes"], st["leaves"], st["tri_tests"]) == tuple(int(x) for x in of["stats"])
    assert st["rays"] == size[0] * size[1]


# ---- shared: world8_stress, its pixel-mode result and the permuted caller rays --------------------------
class W8:
    pass


@pytest.fixture(scope="module")
def w8(gpu, oracle):
    c = W8()
    c.s, c.o = _w8(gpu, oracle)
    c.pix = qc.all_pixels(*qc.VALUES_SIZE)
    c.pixel = c.s.query(pixels=c.pix, want=ALL)                       # case 1's result
    c.rays = c.pixel["rays_out"].copy()
    # the reference result of the caller rays: origin / dir mode, whole frame, pixel order
    c.ref = c.s.query(origins=c.rays[:, 0:3], dirs=c.rays[:, 3:6], want=ALL)
    c.perm = np.random.default_rng(qc.PERM_SEED).permutation(len(c.pix))[:-qc.DROPPED]
    assert len(c.perm) % 64 != 0
    c.o_p, c.d_p = c.rays[c.perm, 0:3].copy(), c.rays[c.perm, 3:6].copy()
    c.want = take(c.ref, c.perm)
    return c


# ---- 2. incoherent packets ---------------------------------------------------------------------------
def test_caller_rays_tie_to_the_pixel_result(w8):
    """Where the fed-back direction is a fixed point of the normalisation the origin / dir query traced
    the pixel's own ray, and every output is the pixel-mode result bit for bit."""
    same = (bits(w8.ref["rays_out"]) == bits(w8.rays)).all(axis=1)
    print("fixed points of the normalisation: %d of %d" % (same.sum(), len(same)))
    assert same.mean() >= 0.25                                        # (a floor for the tie to mean something, not a tolerance)
    assert_same(take(w8.ref, same), take(w8.pixel, same), ctx="pixel vs caller rays")
    # the others were renormalised by an ulp: still the same triangle almost everywhere, the same t to float accuracy
    ids = (w8.ref["inst"] == w8.pixel["inst"]) & (w8.ref["tri"] == w8.pixel["tri"])
    assert np.abs(w8.ref["rays_out"] - w8.rays).max() <= 4 * U
    h = ids & (w8.pixel["inst"] >= 0)
    assert np.allclose(w8.ref["t"][h], w8.pixel["t"][h], rtol=1e-5, atol=0)


def test_permuted_rays_give_each_rays_result(w8):
    a = w8.s.query(origins=w8.o_p, dirs=w8.d_p, want=ALL)
    assert_same(a, w8.want, ctx="permuted")
    assert (a["hit"] != 0).sum() > 1000 and (a["hit"] == 0).sum() > 100


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_short_batches(w8, n):
    a = w8.s.query(origins=w8.o_p[:n], dirs=w8.d_p[:n], want=ALL)
    assert_same(a, take(w8.want, slice(0, n)), ctx="n = %d" % n)


def test_a_frame_sized_batch_takes_the_persistent_form_by_itself(w8):
    """172 copies of the permuted list: past 2^20 rays, where the plan picks the persistent form."""
    reps, keys = 172, ("t", "inst", "tri", "hit")
    assert reps * len(w8.perm) >= 1 << 20
    a = w8.s.query(origins=np.tile(w8.o_p, (reps, 1)), dirs=np.tile(w8.d_p, (reps, 1)), want=keys)
    n = len(w8.perm)
    for k in keys:
        assert np.array_equal(bits(a[k]).reshape(reps, n), np.broadcast_to(bits(w8.want[k]), (reps, n))), k


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_direction_length_does_not_matter(w8, scale):
    """The kernel normalises: the traced direction moves by rounding only (the scaling's, the
    length's, the reciprocal's and the product's: under 8 u per component of a unit vector), the
    accepted triangle is the same and t agrees to the project's float tolerance."""
    a = w8.s.query(origins=w8.o_p, dirs=(np.float32(scale) * w8.d_p).astype(np.float32), want=ALL)
    assert np.abs(a["rays_out"][:, 3:6] - w8.want["rays_out"][:, 3:6]).max() <= 8 * U
    assert np.array_equal(a["rays_out"][:, 0:3], w8.want["rays_out"][:, 0:3])
    for k in ("inst", "tri", "hit"):
        assert np.array_equal(a[k], w8.want[k]), (k, int((a[k] != w8.want[k]).sum()))
    h = a["inst"] >= 0
    assert np.allclose(a["t"][h], w8.want["t"][h], rtol=1e-5, atol=0)
    # (barycentrics: the direction's 8 u x t <= 30 over an edge >= 1 moves them by 2e-5, beside their own float32 noise)
    assert np.abs(a["uv"][h] - w8.want["uv"][h]).max() <= 1e-4


# ---- 3. variants agree -------------------------------------------------------------------------------
def test_counted_and_device_pointer_runs_are_bit_identical(w8, monkeypatch):
    import torch
    counted = w8.s.query(origins=w8.o_p, dirs=w8.d_p, want=ALL, stats=True)
    assert_same(counted, w8.want, ctx="counted")
    assert counted["stats"]["rays"] == len(w8.perm)
    n = len(w8.perm)
    for form in ("small", "persistent"):
        monkeypatch.setenv("RT_QUERY_FORM", form)
        for stats in (False, True):
            dev = "cuda"
            o_d, d_d = torch.from_numpy(w8.o_p).to(dev), torch.from_numpy(w8.d_p).to(dev)
            out = {k: torch.full((n, c) if c > 1 else (n,), 77, dtype={np.float32: torch.float32, np.int32: torch.int32,
                                                                     np.uint8: torch.uint8}[dt], device=dev)
                   for k, (c, dt) in gpu_outputs().items()}
            torch.cuda.synchronize()
            st = w8.s.query_device(n, origin_ptr=o_d.data_ptr(), dir_ptr=d_d.data_ptr(), stats=stats,
                                   **{k + "_ptr": v.data_ptr() for k, v in out.items()})
            got = {k: v.cpu().numpy() for k, v in out.items()}
            assert_same(got, w8.want, ctx="device pointers, %s, stats %d" % (form, stats))
            if stats:
                assert {k: st[k] for k in ("rays", "nodes", "leaves", "tri_tests")} == \
                       {k: counted["stats"][k] for k in ("rays", "nodes", "leaves", "tri_tests")}


def gpu_outputs():
    import rtamd
    return rtamd.QUERY_OUTPUTS


# ---- 4. values -----------------------------------------------------------------------------------------
def test_values_against_the_references_arithmetic(w8, oracle):
    """t, u, v of the hit rays against float64 values recomputed from the exported scene, with the
    reference's own arithmetic on the world-space triangle (oracle.kat("tri_hit")) as the yardstick:
    its worst deviation e_ref is the float32 noise floor, the GPU must stay within 4 e_ref.
    Measured on MI355X: see DESIGN.md section 3.5."""
    a = w8.want
    h = a["inst"] >= 0
    arrays = w8.s.arrays()
    rays, inst, tri = a["rays_out"][h], a["inst"][h], a["tri"][h]
    keep, e_ref, (t64, u64, v64) = qc.kat_yardstick(oracle, arrays, rays, inst, tri)
    assert (~keep).sum() <= qc.KAT_MISS_CAP * h.sum(), (int((~keep).sum()), int(h.sum()))
    dev = np.stack([np.abs(a["t"][h] - t64) / np.maximum(1.0, np.abs(t64)), np.abs(a["uv"][h][:, 0] - u64),
                    np.abs(a["uv"][h][:, 1] - v64)])[:, keep]
    print("values: %d rays, e_ref %.4g, GPU worst %.4g (t %.4g, u %.4g, v %.4g)"
          % (keep.sum(), e_ref, dev.max(), dev[0].max(), dev[1].max(), dev[2].max()))
    assert dev.max() <= 4 * e_ref, (float(dev.max()), e_ref)
    # the normal: unit length, the interpolated vertex normal
    nrm = a["normal"][h].astype(np.float64)
    assert np.abs(np.linalg.norm(nrm, axis=1) - 1.0).max() <= 1e-5
    assert np.abs(nrm - qc.normals64(arrays, inst, tri, u64, v64)).max() <= 1e-5
    assert not a["normal"][~h].any() and not a["uv"][~h].any()         # a miss: zeros


# ---- 5. tmax and occlusion -----------------------------------------------------------------------------
def _tmax_for(t):
    k = np.arange(len(t)) % 4
    return np.select([k == 0, k == 1, k == 2], [np.float32(0.5) * t, t, np.nextafter(t, np.float32(np.inf))],
                     np.float32(np.inf)).astype(np.float32), k


def test_tmax_and_occlusion(w8, monkeypatch):
    t = w8.want["t"]
    tmax, k = _tmax_for(t)
    expect = (w8.want["inst"] >= 0) & (k >= 2)                         # a hit exactly when t < tmax
    assert expect.sum() > 500 and ((w8.want["inst"] >= 0) & ~expect).sum() > 500
    c = w8.s.query(origins=w8.o_p, dirs=w8.d_p, tmax=tmax, want=ALL)
    assert np.array_equal(c["hit"] != 0, expect)
    assert_same(take(c, expect), take(w8.want, expect), ctx="hits under tmax")
    assert np.isposinf(c["t"][~expect]).all() and (c["inst"][~expect] == -1).all() and (c["tri"][~expect] == -1).all()
    for form in ("small", "persistent"):
        monkeypatch.setenv("RT_QUERY_FORM", form)
        for what, kw in (("ordered tree", {}), ("brute force", dict(use_bvh=False)), ("counted heap walk", dict(stats=True))):
            a = w8.s.query(origins=w8.o_p, dirs=w8.d_p, tmax=tmax, any_hit=True, want=("hit",), **kw)
            assert np.array_equal(a["hit"] != 0, expect), (form, what, int(((a["hit"] != 0) != expect).sum()))
    a = w8.s.query(origins=w8.o_p, dirs=w8.d_p, any_hit=True, want=("hit",))        # no tmax: any hit at all
    assert np.array_equal(a["hit"], w8.want["hit"])


def test_occlusion_on_the_heap_form(gpu, oracle, tmp_path, monkeypatch):
    """A scene without a usable ordered tree (the chain: deeper than the traversal's stack) runs the
    uncounted heap kernels; the occlusion booleans are the closest-hit query's."""
    size = (64, 48)
    s, _ = build_scene("chain", size, gpu, None, tmp_path)
    pix = qc.all_pixels(*size)
    base = s.query(pixels=pix, want=ALL)
    tmax, k = _tmax_for(base["t"])
    expect = (base["inst"] >= 0) & (k >= 2)
    assert expect.sum() > 50
    for form in ("small", "persistent"):
        monkeypatch.setenv("RT_QUERY_FORM", form)
        c = s.query(pixels=pix, tmax=tmax, want=("hit", "t"))
        assert np.array_equal(c["hit"] != 0, expect), form
        a = s.query(pixels=pix, tmax=tmax, any_hit=True, want=("hit",))
        assert np.array_equal(a["hit"] != 0, expect), form


# ---- 6. hostile rays --------------------------------------------------------------------------------------
def test_rejected_rays_miss_and_leave_their_wave_alone(w8, monkeypatch):
    """Lanes 0-2 are rejected (zero direction, NaN origin, infinite direction component): a miss each.
    Lane 3's direction (1e-30, 1, 0) is finite and nonzero, so it is traced -- its x component is
    below 2^-64, where the filtered slab test must hand over to the exact one -- from above the
    world, pointing up: a miss by geometry, on every form.  The other 60 lanes keep their results."""
    o, d = w8.o_p[:64].copy(), w8.d_p[:64].copy()
    d[0] = 0.0
    o[1, 1] = np.nan
    d[2, 0] = np.inf
    o[3], d[3] = (0.3, 50.0, 0.2), (1e-30, 1.0, 0.0)
    for form in ("small", "persistent"):
        monkeypatch.setenv("RT_QUERY_FORM", form)
        for what, kw in (("ordered tree", {}), ("counted heap walk", dict(stats=True)), ("brute force", dict(use_bvh=False))):
            a = w8.s.query(origins=o, dirs=d, want=ALL, **kw)
            ctx = "%s, %s" % (form, what)
            assert not a["hit"][:4].any() and np.isposinf(a["t"][:4]).all(), ctx
            assert (a["inst"][:4] == -1).all() and (a["tri"][:4] == -1).all(), ctx
            assert not a["uv"][:4].any() and not a["normal"][:4].any(), ctx
            assert_same(take(a, slice(4, 64)), take(w8.want, slice(4, 64)), ctx=ctx)
            if "stats" in a:
                assert a["stats"]["rays"] == 61                        # the rejected rays were never traced
            h = a["hit"].astype(bool)
            occ = w8.s.query(origins=o, dirs=d, any_hit=True, want=("hit",), **kw)
            assert np.array_equal(occ["hit"].astype(bool), h), ctx
    # the same tiny-component direction pointing down at the world from above: the exact test's hit is brute force's
    o2 = np.tile(np.float32([0.3, 50.0, 0.2]), (3, 1)) + np.float32([[0, 0, 0], [1, 0, 1], [-2, 0, 2]])
    d2 = np.tile(np.float32([1e-30, -1.0, 0.0]), (3, 1))
    a, b = w8.s.query(origins=o2, dirs=d2, want=ALL), w8.s.query(origins=o2, dirs=d2, want=ALL, use_bvh=False)
    assert a["hit"].all()
    assert_same(a, b, ctx="tiny direction component")
    assert_same(w8.s.query(origins=o2, dirs=d2, want=ALL, stats=True), b, ctx="tiny direction component, counted")


def test_zero_component_rays_at_box_faces(w8, monkeypatch):
    """Rays with one or two zero direction components whose constant coordinate lies on, just inside
    and just outside the cubes' side faces (the cube world's faces are at integers + 0.5), from near
    and from 3000 units away: the ordered-tree kernels cut such a ray's zero axes with a slack formed
    from its own origin; the counted heap walk and brute force have no cut.  Every output agrees bit
    for bit."""
    eps = np.float32([0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 3e-4, -3e-4, 1e-3, -1e-3, 0.02, -0.02, 0.25])
    o, d = [], []
    for far in (0.0, 3000.0):
        for face in (-2.5, -0.5, 0.5, 1.5):
            for e in eps:
                for other in (-1.3, 0.1, 0.77):
                    o.append((face + e, 14.0 + far, other)); d.append((0.0, -1.0, 0.0))          # straight down
                    o.append((face + e, 14.0 + far, other - 3.0 - 0.75 * far)); d.append((0.0, -0.8, 0.6))   # d.x = 0
                    o.append((other - 3.0 - 0.75 * far, 14.0 + far, face + e)); d.append((0.6, -0.8, 0.0))   # d.z = 0
                    o.append((-9.0 - far, 0.5 + e + (face + 2.5), other)); d.append((1.0, 0.0, 0.0))          # along x at a top face
    o, d = np.float32(o), np.float32(d)
    base = w8.s.query(origins=o, dirs=d, want=ALL, stats=True)          # the reference's walk: same leaf order, no cut
    assert 0.2 < (base["hit"] != 0).mean() < 1.0
    for form in ("small", "persistent"):
        monkeypatch.setenv("RT_QUERY_FORM", form)
        assert_same(w8.s.query(origins=o, dirs=d, want=ALL), base, ctx="ordered tree, " + form)
        occ = w8.s.query(origins=o, dirs=d, any_hit=True, want=("hit",))
        assert np.array_equal(occ["hit"], base["hit"]), form
    # brute force visits the instances in index order: on a face two cubes share it may accept the
    # other cube's triangle at the same distance, so only the boolean and the distance are compared
    br = w8.s.query(origins=o, dirs=d, want=ALL, use_bvh=False)
    assert np.array_equal(br["hit"], base["hit"])
    h = base["hit"] != 0
    assert np.allclose(br["t"][h], base["t"][h], rtol=1e-5, atol=0)


def test_far_axis_parallel_rays_hit_the_oracles_instance(gpu, oracle):
    """Rays with two zero direction components from 1e4 units away: the expected instance is the
    oracle's, through a camera placed at the ray's origin (identity orientation: its centre pixel's
    ray is exactly +z).  Pure translations, where a shortcut assuming a nearby camera would apply."""
    W, H = 8, 8
    places = [((float(x), float(y), float(z)), (0, 0, 0, 1)) for x in (-2, 0, 2) for y in (-1, 1) for z in (0, 2)]
    origins = [(0.0, 1.0, -1e4), (2.2, -1.1, -1e4), (-2.0, 0.8, -1e4), (0.0, 0.0, -1e4), (1.0, 1.0, -1e4), (-1.7, -0.9, -1e4)]
    s, o = _cubes(gpu, oracle, (W, H), places, cam=(origins[0], (0, 0, 0, 1)))
    exp_inst, exp_tri = [], []
    for p in origins:
        o.set_camera(np.float32(p), np.float32((0, 0, 0, 1)))
        of = orc_render(oracle, o, spp=1, want=("hit_inst", "hit_tri"))
        exp_inst.append(int(of["hit_inst"][H // 2, W // 2]))
        exp_tri.append(int(of["hit_tri"][H // 2, W // 2]))
    assert sorted(set(exp_inst))[0] == -1 and len(set(exp_inst)) >= 4   # hits on several cubes, and a miss between them
    d = np.tile(np.float32([0, 0, 1]), (len(origins), 1))
    for kw in ({}, dict(use_bvh=False), dict(stats=True)):
        a = s.query(origins=np.float32(origins), dirs=d, want=ALL, **kw)
        assert a["inst"].tolist() == exp_inst and a["tri"].tolist() == exp_tri, kw
        occ = s.query(origins=np.float32(origins), dirs=d, any_hit=True, want=("hit",), **kw)
        assert (occ["hit"] != 0).tolist() == [i >= 0 for i in exp_inst], kw
    # and by pixel, from the product camera itself placed there
    for p, ei, et in zip(origins, exp_inst, exp_tri):
        s.set_camera(p, (0, 0, 0, 1))
        r = s.query(pixels=[(W // 2, H // 2)], want=ALL)
        assert np.array_equal(r["rays_out"][0], np.float32(list(p) + [0, 0, 1]))
        assert (int(r["inst"][0]), int(r["tri"][0])) == (ei, et)


# ---- 7. state -------------------------------------------------------------------------------------------------
def test_queries_leave_the_frame_state_alone(gpu, oracle):
    import torch
    s, o = _w8(gpu, oracle)
    W, H = qc.VALUES_SIZE
    pix = qc.all_pixels(W, H)
    of = orc_render(oracle, o, spp=1)
    first = s.render(spp=1, want=("rgba", "radiance", "hit_inst", "hit_tri"), stats=False)
    lt = s.last_trace()
    q0 = s.query(pixels=pix, want=ALL)
    s.query(pixels=pix, want=ALL, stats=True)
    s.query(pixels=pix[:1], any_hit=True, want=("hit",), use_bvh=False)
    assert s.last_trace() == lt                                        # no trace kernel was launched
    fr = s.render(spp=1, want=("rgba", "radiance", "hit_inst", "hit_tri"), stats=False)
    assert_frames_equal(fr, of, ctx="frame after queries")
    assert np.array_equal(fr["rgba"], first["rgba"])
    assert s.last_trace() == lt
    # between the frames of a four-slot pipeline
    s.set_frame_slots(4)
    streams = [torch.cuda.Stream() for _ in range(4)]
    bufs = [torch.zeros(H * W, dtype=torch.int32, device="cuda") for _ in range(8)]
    torch.cuda.synchronize()
    for k in range(8):
        s.render_device(spp=1, compact=False, rgba_ptr=bufs[k].data_ptr(), stream=streams[k % 4].cuda_stream, sync=False)
        if k in (1, 2, 5):
            assert_same(s.query(pixels=pix, want=ALL, rebuild_bvh=(k != 2)), q0, ctx="between frames, after frame %d" % k)
    torch.cuda.synchronize()
    for k in range(8):
        assert np.array_equal(bufs[k].cpu().numpy().view(np.uint32).reshape(H, W), first["rgba"]), k


# ---- 8. pick ------------------------------------------------------------------------------------------------------
def test_pick_and_the_cli_agree_with_the_frame(gpu):
    W, H = 160, 90
    s = gpu.Scene.load_json(scene_path("world8_stress"), W, H)
    fr = s.render(spp=1, want=("hit_inst", "hit_tri"), stats=False)
    ys, xs = np.nonzero(fr["hit_inst"] >= 0)
    hx, hy = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])
    ys, xs = np.nonzero(fr["hit_inst"] < 0)
    sx, sy = int(xs[len(xs) // 2]), int(ys[len(ys) // 2])
    inst, tri, t = s.pick(hx, hy)
    assert (inst, tri) == (int(fr["hit_inst"][hy, hx]), int(fr["hit_tri"][hy, hx])) and 0 < t < np.inf
    assert s.pick(sx, sy) == (-1, -1, np.inf)
    for flags in ([], ["-r"]):
        r = subprocess.run([CLI, "-c", scene_path("world8_stress"), "--width", str(W), "--height", str(H), "--pick",
                            "%d,%d" % (hx, hy)] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == "pick %d %d inst %d tri %d t %.9g\n" % (hx, hy, inst, tri, t), r.stdout
    r = subprocess.run([CLI, "-c", scene_path("world8_stress"), "--width", str(W), "--height", str(H), "--pick",
                        "%d,%d" % (sx, sy)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == "pick %d %d miss\n" % (sx, sy), (r.stdout, r.stderr)
    r = subprocess.run([CLI, "-c", scene_path("world8_stress"), "--width", str(W), "--height", str(H), "--pick",
                        "%d,%d" % (W, 0)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "outside the canvas" in r.stderr


# ---- 9. host staging ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["origin_dir", "pixels"])
def test_host_staging_matches_device_pointers(gpu, mode):
    """Host-pointer batches through the entries' staging (rt_query with every output, rt_shade with
    radiance, rgba and rays_out) against the same batches on device pointers, element for element.
    n = 1, 65, 3 on a scene whose stagings no call has touched: each entry's first allocation, its
    growth, then a smaller batch in the larger image; the two entries alternate, so a staging they
    shared by mistake would show.  The rays come from a second scene object, and the reference calls
    use device pointers, which stage nothing."""
    import torch
    tdt = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8, np.uint32: torch.int32}
    W = H = 16
    s = gpu.Scene.load_json(scene_path("world1"), W, H)
    pix_all = qc.all_pixels(W, H)
    rays = gpu.Scene.load_json(scene_path("world1"), W, H).query(pixels=pix_all, want=("rays_out",))["rays_out"]

    def device_outputs(n, table):
        return {k: torch.full((n, c) if c > 1 else (n,), 77, dtype=tdt[dt], device="cuda") for k, (c, dt) in table.items()}

    def to_numpy(out, table):
        return {k: v.cpu().numpy().view(table[k][1]) for k, v in out.items()}

    for n in (1, 65, 3):
        idx = (np.arange(n) * 7 + n) % (W * H)                     # pixels all over the canvas, another set each time
        if mode == "pixels":
            host_in = dict(pixels=pix_all[idx])
            dev_t = {"pixel": torch.from_numpy(np.ascontiguousarray(pix_all[idx], dtype=np.int32)).cuda()}
            q_in = {}
        else:
            host_in = dict(origins=rays[idx, :3], dirs=rays[idx, 3:] * np.float32(2.5))
            dev_t = {"origin": torch.from_numpy(np.ascontiguousarray(host_in["origins"])).cuda(),
                     "dir": torch.from_numpy(np.ascontiguousarray(host_in["dirs"])).cuda()}
            tmax = np.linspace(0.5, 40.0, n, dtype=np.float32)     # some rays cut short, some not
            q_in = dict(tmax=tmax)
            dev_t["tmax"] = torch.from_numpy(tmax).cuda()
        ptrs = {k + "_ptr": v.data_ptr() for k, v in dev_t.items()}
        # rt_query
        out = device_outputs(n, gpu.QUERY_OUTPUTS)
        torch.cuda.synchronize()
        s.query_device(n, **ptrs, **{k + "_ptr": v.data_ptr() for k, v in out.items()})
        want = to_numpy(out, gpu.QUERY_OUTPUTS)
        assert_same(s.query(want=ALL, **host_in, **q_in), want, ctx="rt_query, %s, n = %d" % (mode, n))
        # rt_shade
        ptrs.pop("tmax_ptr", None)
        out = device_outputs(n, gpu.SHADE_OUTPUTS)
        torch.cuda.synchronize()
        s.shade_device(n, **ptrs, **{k + "_ptr": v.data_ptr() for k, v in out.items()})
        want = to_numpy(out, gpu.SHADE_OUTPUTS)
        assert_same(s.shade(want=tuple(gpu.SHADE_OUTPUTS), **host_in), want, keys=tuple(gpu.SHADE_OUTPUTS),
                    ctx="rt_shade, %s, n = %d" % (mode, n))
