"""rt_shade without a GPU.

The argument checks, which come before any device work, each with its status, on a host-only scene
(RT_ERR_NODEV only after they pass); rt_shade_opts_default's values; shade_plan (csrc/rt_plan.h)
compiled for the host: the tree form by query_plan's rule, the NS = 0 kernels for all-opaque scenes
only, 256-thread blocks over ceil(n / 256) blocks; and the header's symbols against rtamd.SYMBOLS.
The GPU twin is tests/test_gpu_shade.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import shade_cases as sc
from conftest import ROOT, scene_path
from test_abi import declared_symbols


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = str(tmp_path_factory.mktemp("shade_plan") / "shade_plan_host")
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math",
                    "-fno-slp-vectorize", "-I", os.path.join(ROOT, "gpu-ray-tracer_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shade_plan_host.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)

    def run(n, use_bvh=1, n_leaf=64, ftree=1, refractive=0, depth=2, tex=0):
        out = subprocess.run([exe] + [str(a) for a in (n, use_bvh, n_leaf, ftree, refractive, depth, tex)], check=True,
                             capture_output=True, text=True).stdout.split()
        return dict(zip(("tree", "ns_bucket", "tex", "block", "blocks", "ns"), (int(x) for x in out)))
    return run


def test_tree_form_is_query_plans_rule(plan):
    assert plan(6144)["tree"] == sc.ORDERED
    assert plan(6144, ftree=0)["tree"] == sc.HEAP                  # one leaf, or a tree too deep for the fast traversal
    assert plan(6144, use_bvh=0)["tree"] == sc.BRUTE
    assert plan(6144, n_leaf=0)["tree"] == sc.BRUTE


@pytest.mark.parametrize("depth", (0, 1, 2, 9))
def test_frame_stack_bucket(plan, depth):
    """NS = 0 only without a refractive material, at any depth; with one, the generic depth -- a depth-0
    scene with refraction included (shade_shortcuts: the NS = 0 kernels assume no refraction)."""
    p = plan(6144, refractive=0, depth=depth)
    assert (p["ns"], p["ns_bucket"]) == (0, 0)
    p = plan(6144, refractive=1, depth=depth)
    assert p["ns"] == max(depth, 1) and p["ns_bucket"] == sc.NG
    assert plan(6144, tex=1)["tex"] == 1 and plan(6144)["tex"] == 0


@pytest.mark.parametrize("n", sc.PLAN_N)
def test_grid_covers_the_batch(plan, n):
    for kw in ({}, dict(ftree=0), dict(use_bvh=0), dict(refractive=1, tex=1)):
        p = plan(n, **kw)
        assert p["block"] == 256                                   # the small form only
        assert p["blocks"] == (n + 255) // 256 and p["blocks"] >= 1
        assert 256 * p["blocks"] >= n > 256 * (p["blocks"] - 1)


def test_header_symbols_listed(rt):
    assert declared_symbols() == sorted(rt.SYMBOLS)
    assert {"rt_shade", "rt_shade_opts_default", "rt_shade_last"} <= set(rt.SYMBOLS)
    L = ctypes.CDLL(rt.LIB_PATH)
    assert all(hasattr(L, n) for n in ("rt_shade", "rt_shade_opts_default", "rt_shade_last"))


def test_opts_default(rt):
    o = rt.ShadeOpts()
    ctypes.memset(ctypes.byref(o), 0xff, ctypes.sizeof(o))
    rt.lib().rt_shade_opts_default(ctypes.byref(o))
    assert (o.n, o.sample, o.use_bvh, o.rebuild_bvh, o.textures, o.order, o.host) == (0, 0, 1, 1, 0, rt.RT_QUERY_ORDER_CALLER, 0)
    assert (o.origin, o.dir, o.pixel, o.radiance, o.rgba, o.rays_out) == (None,) * 6
    rt.lib().rt_shade_opts_default(None)                           # a null pointer is ignored


def test_argument_checks_come_first(rt):
    """Every argument error with its status on a host-only scene; a valid call reaches the device
    question only after them."""
    L = rt.lib()
    W, H = 16, 12
    s = rt.Scene.load_json(scene_path("world1"), W, H)
    n = 5
    org, dirs = np.zeros((n, 3), np.float32), np.tile(np.float32([0, 0, 1]), (n, 1))
    pix = np.int32([[0, 0], [15, 11], [3, 4], [0, 11], [15, 0]])
    rad, rgba, rays = np.zeros((n, 4), np.float32), np.zeros(n, np.uint32), np.zeros((n, 6), np.float32)

    def opts(**kw):
        o = rt.ShadeOpts()
        L.rt_shade_opts_default(ctypes.byref(o))
        o.n, o.host = n, 1
        o.origin, o.dir, o.radiance = org.ctypes.data, dirs.ctypes.data, rad.ctypes.data
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(**kw):
        return L.rt_shade(s._h, ctypes.byref(opts(**kw)))

    by_pixel = dict(origin=None, dir=None, pixel=pix.ctypes.data)
    assert L.rt_shade(s._h, None) == rt.RT_ERR_ARG
    assert L.rt_shade(None, ctypes.byref(opts())) == rt.RT_ERR_ARG
    assert call(n=-1) == rt.RT_ERR_ARG
    assert call(origin=None, dir=None) == rt.RT_ERR_ARG            # neither pixel nor origin and dir
    assert call(dir=None) == rt.RT_ERR_ARG and call(origin=None) == rt.RT_ERR_ARG
    assert call(pixel=pix.ctypes.data) == rt.RT_ERR_ARG            # pixel together with both
    assert call(pixel=pix.ctypes.data, dir=None) == rt.RT_ERR_ARG and call(pixel=pix.ctypes.data, origin=None) == rt.RT_ERR_ARG
    assert call(sample=-1, **by_pixel) == rt.RT_ERR_ARG
    assert call(radiance=None) == rt.RT_ERR_ARG
    assert b"no output" in L.rt_last_error()
    for order in (-1, 2):
        assert call(order=order) == rt.RT_ERR_ARG
    for bad in ((-1, 0), (0, -1), (W, 0), (0, H)):                 # host pixels are checked against the canvas
        p = pix.copy()
        p[3] = bad
        assert call(origin=None, dir=None, pixel=p.ctypes.data) == rt.RT_ERR_ARG
        assert b"pixel 3 is outside" in L.rt_last_error()
    assert call(sample=65536, **by_pixel) == rt.RT_ERR_LIMIT
    assert call(n=2 ** 31, order=rt.RT_QUERY_ORDER_SORTED, host=0) == rt.RT_ERR_LIMIT
    assert call(n=256 * (2 ** 31 - 1) + 1, host=0) == rt.RT_ERR_LIMIT   # more rays than the grid's blocks hold
    assert b"256" in L.rt_last_error()
    assert call(textures=1) == rt.RT_ERR_STATE                     # no atlas
    assert b"atlas" in L.rt_last_error()
    # argument errors outrank the limits, the limits the state
    assert call(sample=65536, radiance=None, **by_pixel) == rt.RT_ERR_ARG
    assert call(sample=65536, textures=1, **by_pixel) == rt.RT_ERR_LIMIT
    # n = 0: nothing to do, with or without a device
    assert call(n=0) == rt.RT_OK
    assert not rad.any()
    v = np.zeros(8, np.int32)
    assert L.rt_shade_last(s._h, v.ctypes.data) == rt.RT_ERR_STATE  # no shade call has launched
    assert L.rt_shade_last(None, v.ctypes.data) == rt.RT_ERR_ARG
    if rt.device_count() == 0:                                     # (with a device: tests/test_gpu_shade.py)
        for kw in ({}, by_pixel, dict(sample=65535, **by_pixel), dict(rgba=rgba.ctypes.data, rays_out=rays.ctypes.data),
                   dict(order=rt.RT_QUERY_ORDER_SORTED)):
            assert call(**kw) == rt.RT_ERR_NODEV, kw
        with pytest.raises(rt.RtError) as e:
            s.shade(pixels=pix)
        assert e.value.code == rt.RT_ERR_NODEV
        assert L.rt_shade_last(s._h, v.ctypes.data) == rt.RT_ERR_STATE
    with pytest.raises(rt.RtError) as e:
        s.shade()
    assert e.value.code == rt.RT_ERR_ARG
