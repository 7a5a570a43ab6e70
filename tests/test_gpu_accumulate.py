"""Progressive refinement on the GPU (rt_accumulate): samples added call by call give, after n of
them, the frame of rt_render(spp = n) and of the oracle's orc_render(spp = n) -- RGBA8 equal in
every byte, radiance within the project's 1e-5 relative bound, sample 0's hit ids equal -- on

  stress       world8_stress 96 x 64 with the BVH (reflective: the NS = 0 fast kernel, the sky pre-pass)
  world1_brute world1 64 x 48, brute force (refractive)
  media        the media scene of tests/integrator_cases.py, 48 x 32, depth 9
  stress_odd   world8_stress 50 x 37: neither a multiple of the 8-pixel group nor of a 16-byte
               row piece (the fold's tail block, partial groups)

and: batching, the restarts (camera, instance, environment, textures, restart = 1, reset),
independence from rt_render / rt_update_scene and from frames in flight, host against device
pointers, the launch record, RT_ERR_STATE on a split scene, and the CLI's --accumulate.
The oracle's frames are rendered once per (case, n) and shared, never written to.  The host twin
is tests/test_accumulate_host.py."""
import os
import subprocess

import numpy as np
import pytest

import integrator_cases as ic
from conftest import ROOT, scene_path
from twin import Twin, assert_frames_equal, mirror_camera, orc_render

pytestmark = pytest.mark.gpu
WANT = ("rgba", "radiance", "hit_inst", "hit_tri")
CLI = os.path.join(ROOT, "gpu-ray-tracer_amd", "rtracer")
# case -> (scene, W, H, use_bvh)
CASES = {"stress": ("world8_stress", 96, 64, True), "world1_brute": ("world1", 64, 48, False),
         "media": (None, ic.SIZE[0], ic.SIZE[1], True), "stress_odd": ("world8_stress", 50, 37, True)}
N_PREFIX = 9


def make(gpu, oracle, case):
    """A fresh (product scene, oracle scene, use_bvh) of the case."""
    name, w, h, bvh = CASES[case]
    if name is None:
        t = Twin(gpu, oracle)
        ic.build(t, "media", depth=9)
        return t.gpu, t.orc, bvh
    return gpu.Scene.load_json(scene_path(name), w, h), oracle.load(scene_path(name), w, h), bvh


@pytest.fixture(scope="module")
def frames(gpu, oracle):
    """The oracle's frame of `case` in its initial state at spp = n."""
    cache, scenes = {}, {}

    def get(case, n):
        if (case, n) not in cache:
            if case not in scenes:
                scenes[case] = make(gpu, oracle, case)[1]
            cache[case, n] = orc_render(oracle, scenes[case], spp=n, use_bvh=int(CASES[case][3]))
        return cache[case, n]
    return get


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b, keys=WANT):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


@pytest.mark.parametrize("case", list(CASES))
def test_prefix_parity(gpu, oracle, frames, case):
    """One sample per call up to n = 9; after every call the frame is the oracle's and the
    product's own at spp = n.  Every pixel is compared.
    Beyond the project bar, the radiance equals render(spp=n)'s bit for bit: the fold performs
    the one-shot kernel's float32 additions in its order and resolves with its mean (rt_accum.h),
    and the 1-spp kernel computes sample k with the bits the n-spp launch of the same kernel
    family gives it, so nothing is left to differ.  The 1e-5 bound alone lets a resolve that
    multiplies by 1.0f / n pass at n = 3, 5, 6, 7, 9 (one rounding, no byte of these frames
    flips: profiles/accumulate/teeth.txt)."""
    s, _, bvh = make(gpu, oracle, case)
    bit_equal = []
    for n in range(1, N_PREFIX + 1):
        fr = s.accumulate(samples=1, use_bvh=bvh, want=WANT)
        assert fr["n"] == n and s.accumulated[0] == n, (case, n, fr["n"], s.accumulated)
        assert_frames_equal(fr, frames(case, n), ctx=("accumulate", case, n), max_pm1=0)
        own = s.render(spp=n, use_bvh=bvh, want=WANT, stats=False)
        assert_frames_equal(fr, own, ctx=("accumulate vs render", case, n), max_pm1=0)
        bit_equal.append(bool(np.array_equal(bits(fr["radiance"]), bits(own["radiance"]))))
    print("radiance bit-equal to render(spp=n), n = 1..%d: %s %s" % (N_PREFIX, case, bit_equal))
    assert all(bit_equal), (case, bit_equal)
    assert s.accumulated == (N_PREFIX, CASES[case][1], CASES[case][2], 0)


def test_batching(gpu, oracle, frames):
    """samples = 5 in one call is five calls of one, bit for bit."""
    a, _, bvh = make(gpu, oracle, "stress_odd")
    b, _, _ = make(gpu, oracle, "stress_odd")
    one = a.accumulate(samples=5, want=WANT)
    for _ in range(5):
        five = b.accumulate(samples=1, want=WANT)
    assert one["n"] == five["n"] == 5
    assert same_bits(one, five)
    assert_frames_equal(one, frames("stress_odd", 5), ctx="batch of 5", max_pm1=0)
    # and a batch on top of single samples: 5 + 4 = 9
    nine = a.accumulate(samples=4, want=WANT)
    assert nine["n"] == 9
    assert_frames_equal(nine, frames("stress_odd", 9), ctx="5 + 4", max_pm1=0)


def _four(s, **kw):
    fr = s.accumulate(samples=4, want=WANT, **kw)
    assert fr["n"] == 4
    return fr


def _restarted(s, oracle, o, restarts, ctx, **kw):
    """The next call starts again: n = 1, the oracle's 1-spp frame of the new state, one more restart."""
    fr = s.accumulate(want=WANT, **kw)
    assert fr["n"] == 1, (ctx, fr["n"])
    assert s.accumulated[0] == 1 and s.accumulated[3] == restarts, (ctx, s.accumulated)
    assert_frames_equal(fr, orc_render(oracle, o, spp=1), ctx=ctx, max_pm1=0)
    return fr


def test_restarts(gpu, oracle, frames):
    s, o, _ = make(gpu, oracle, "stress_odd")
    f4 = _four(s)
    assert_frames_equal(f4, frames("stress_odd", 4), ctx="before the restarts", max_pm1=0)
    # a camera move
    s.translate_camera([0.4, -0.2, 0.7])
    mirror_camera(s, o)
    f1 = _restarted(s, oracle, o, 1, "camera")
    assert not np.array_equal(f1["rgba"], frames("stress_odd", 1)["rgba"])
    # one instance moved
    assert s.accumulate(samples=3)["n"] == 4
    inst = s.export("instances")
    pos = inst[3][4:7] + np.array([0.25, 0.5, -0.25], np.float32)
    s.set_trans(3, pos=pos)
    o.set_trans(3, pos=pos)
    _restarted(s, oracle, o, 2, "set_trans")
    # the environment (depth)
    s.accumulate(samples=3)
    depth = s.info()["depth"]
    s.set_env(depth=depth - 1 if depth > 0 else 1)
    o.set_env(depth=depth - 1 if depth > 0 else 1)
    _restarted(s, oracle, o, 3, "set_env")
    # restart = 1 and rt_accumulate_reset, nothing changed
    s.accumulate(samples=3)
    _restarted(s, oracle, o, 4, "restart=True", restart=True)
    s.accumulate(samples=3)
    s.accumulate_reset()
    assert s.accumulated[0] == 0 and s.accumulated[3] == 5
    _restarted(s, oracle, o, 5, "accumulate_reset")
    s.accumulate_reset()
    s.accumulate_reset()                                       # nothing held: no restart counted
    assert s.accumulated[3] == 6


def test_textures_flag_restarts(gpu, oracle):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_atlas
    w, h = 50, 37
    s = gpu.Scene.load_json(scene_path("world8_stress_tex"), w, h)
    s.load_atlas()
    o = oracle.load(scene_path("world8_stress_tex"), w, h)
    o.set_atlas(make_atlas.atlas())
    plain = _four(s)
    assert_frames_equal(plain, orc_render(oracle, o, spp=4), ctx="textures off", max_pm1=0)
    o.set_textures(True)
    tex = _restarted(s, oracle, o, 1, "textures on", textures=True)
    assert not np.array_equal(tex["rgba"], plain["rgba"])
    for n in (2, 3):
        fr = s.accumulate(want=WANT, textures=True)
        assert fr["n"] == n
    assert_frames_equal(fr, orc_render(oracle, o, spp=3), ctx="textures on, 3 samples", max_pm1=0)
    # a new atlas restarts too
    a = make_atlas.atlas().copy()
    a[..., 0] = 255 - a[..., 0]
    s.set_atlas(a)
    o.set_atlas(a)
    _restarted(s, oracle, o, 2, "atlas", textures=True)


def test_bvh_switches_do_not_restart(gpu, oracle, frames):
    s, _, _ = make(gpu, oracle, "stress_odd")
    s.accumulate(samples=2)
    s.accumulate(use_bvh=False)
    s.accumulate(rebuild_bvh=False)
    fr = s.accumulate(use_bvh=False, want=WANT)
    assert fr["n"] == 5 and s.accumulated[3] == 0
    assert_frames_equal(fr, frames("stress_odd", 5), ctx="brute force in the middle", max_pm1=0)


def test_independent_of_render_and_update_scene(gpu, oracle, frames):
    a, _, _ = make(gpu, oracle, "stress_odd")
    b, _, _ = make(gpu, oracle, "stress_odd")
    r1 = b.render(spp=1, want=WANT, stats=False)
    b.update_scene()
    canvas = b.canvas().copy()
    for n in range(1, 5):
        fa = a.accumulate(want=WANT)
        ra = a.render(spp=1, want=WANT, stats=False)           # between the calls
        assert same_bits(ra, r1), n
        a.update_scene()
        assert np.array_equal(a.canvas(), canvas), n
        assert a.accumulated[0] == n and a.accumulated[3] == 0
        fb = b.accumulate(want=WANT)                           # nothing in between but the first two frames
        assert fa["n"] == fb["n"] == n
        assert same_bits(fa, fb), n
    assert_frames_equal(fa, frames("stress_odd", 4), ctx="with renders in between", max_pm1=0)


def test_with_frames_in_flight(gpu, oracle, frames):
    import torch
    s, _, _ = make(gpu, oracle, "stress")
    w, h = CASES["stress"][1:3]
    s.set_frame_slots(4)
    streams = [torch.cuda.Stream() for _ in range(4)]
    bufs = [torch.zeros((h, w), dtype=torch.int32, device="cuda") for _ in range(8)]
    for n in (1, 2, 3):
        for k, buf in enumerate(bufs):                         # frames in flight on other streams
            s.render_device(spp=4, rgba_ptr=buf.data_ptr(), stream=streams[k % 4].cuda_stream)
        fr = s.accumulate(want=WANT)
        assert fr["n"] == n
        assert_frames_equal(fr, frames("stress", n), ctx=("frames in flight", n), max_pm1=0)
    torch.cuda.synchronize()
    ref = frames("stress", 4)["rgba"].astype(np.uint32)
    for buf in bufs:
        assert np.array_equal(buf.cpu().numpy().view(np.uint32), ref)


def test_host_and_device_pointers_agree(gpu, oracle):
    import torch
    a, _, _ = make(gpu, oracle, "stress_odd")
    b, _, _ = make(gpu, oracle, "stress_odd")
    w, h = CASES["stress_odd"][1:3]
    rgba = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    rad = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    hi = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    ht = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    for n in (1, 2, 3):
        host = a.accumulate(want=WANT)
        got = b.accumulate_device(rgba_ptr=rgba.data_ptr(), radiance_ptr=rad.data_ptr(), hit_inst_ptr=hi.data_ptr(),
                                  hit_tri_ptr=ht.data_ptr())
        assert got == host["n"] == n
        dev = {"rgba": rgba.cpu().numpy(), "radiance": rad.cpu().numpy(), "hit_inst": hi.cpu().numpy(), "hit_tri": ht.cpu().numpy()}
        assert same_bits(host, dev), n
    # one output alone
    only = b.accumulate_device(radiance_ptr=rad.data_ptr())
    assert only == 4
    assert np.array_equal(bits(rad.cpu().numpy()), bits(a.accumulate(want=("radiance",))["radiance"]))


@pytest.mark.parametrize("case", ("stress", "world1_brute", "media"))
def test_launch_record(gpu, oracle, case):
    """A call's launches are the spp = 1 kernel render(spp=1) uses on that scene."""
    s, _, bvh = make(gpu, oracle, case)
    s.render(spp=1, use_bvh=bvh, stats=False)
    ref = s.last_trace()
    s.render(spp=16, use_bvh=bvh, stats=True)                  # another kernel in between
    assert s.last_trace() != ref
    s.accumulate(samples=2, use_bvh=bvh)
    assert s.last_trace() == ref, (case, s.last_trace(), ref)


def test_split_scene_is_refused(gpu):
    s = gpu.Scene.load_json(scene_path("world8"), 64, 48)
    assert s.accumulate()["n"] == 1
    s.set_devices([0], 2)
    with pytest.raises(gpu.RtError) as e:
        s.accumulate()
    assert e.value.code == gpu.RT_ERR_STATE
    assert s.accumulated[0] == 1
    s.set_devices([0], 1)
    assert s.accumulate()["n"] == 2


def test_errors_with_a_device(gpu):
    s = gpu.Scene.load_json(scene_path("world8_stress_tex"), 32, 24)
    with pytest.raises(gpu.RtError) as e:                      # textures without an atlas
        s.accumulate(textures=True)
    assert e.value.code == gpu.RT_ERR_STATE
    with pytest.raises(gpu.RtError) as e:
        s.accumulate(want=())
    assert e.value.code == gpu.RT_ERR_ARG
    with pytest.raises(gpu.RtError) as e:
        s.accumulate(samples=0)
    assert e.value.code == gpu.RT_ERR_ARG
    assert s.accumulate()["n"] == 1                            # the scene stays usable
    with pytest.raises(gpu.RtError) as e:
        s.accumulate(samples=65536)                            # 1 held + 65536
    assert e.value.code == gpu.RT_ERR_LIMIT
    assert s.accumulated[0] == 1


def _ppm(path):
    return open(path, "rb").read()


def test_cli_accumulate(tmp_path):
    a, b = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm")
    base = [CLI, "-c", scene_path("world8_stress"), "--width", "96", "--height", "64"]
    ra = subprocess.run(base + ["--accumulate", "4", "-b", "--out", a], capture_output=True, text=True, timeout=120)
    assert ra.returncode == 0, ra.stderr
    assert ra.stdout.count("Sample ") == 4 and "Sample 4: " in ra.stdout and "Accumulated 4 samples" in ra.stdout
    rb = subprocess.run(base + ["--spp", "4", "-b", "--out", b], capture_output=True, text=True, timeout=120)
    assert rb.returncode == 0, rb.stderr
    assert _ppm(a) == _ppm(b) and len(_ppm(a)) > 96 * 64 * 3
    assert subprocess.run(base + ["--accumulate", "0"], capture_output=True, text=True, timeout=120).returncode == 2
