"""The C ABI's argument and state checks that run before a device is needed, as a table of calls:
tests/golden/make_golden.py records what each returns (tests/golden/abi_errors.json) and
tests/test_abi_errors.py replays them.  Every call is otherwise valid, so that only the named
check can fire.  `run(rt, cases)` makes the calls on a 16x16 world1 scene (and on a scene that
rt_builder_finish never finished) and returns [{entry, case, code, message}]; message is None
where the call returns RT_OK (rt_last_error keeps an earlier call's text then)."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 16
NAN, INF = float("nan"), float("inf")


class _Ctx:
    """The library, the finished scene's handle `h`, an unfinished scene's `u`, and buffers that
    outlive the calls."""

    def __init__(self, rt):
        self.rt, self.L = rt, rt.lib()
        vp, ip = ctypes.c_void_p, ctypes.c_int
        self.L.rt_experiment.argtypes = [vp, ip, ip, ip, ctypes.POINTER(ctypes.c_double), vp]
        self.scene = rt.Scene.load_json(os.path.join(ROOT, "scenes", "world1.json"), W, H)
        self.unfinished = rt.Scene.create()
        self.h, self.u = self.scene._h, self.unfinished._h
        self.keep = []

    def buf(self, n, dtype=np.float32, fill=0):
        a = np.full(n, fill, dtype)
        self.keep.append(a)
        return a.ctypes.data_as(ctypes.c_void_p)

    def close(self):
        self.scene.close()
        self.unfinished.close()


def _render(c, null=False, unfinished=False, **kw):
    o = c.rt.RenderOpts()
    c.L.rt_render_opts_default(ctypes.byref(o))
    o.rgba, o.host_outputs = c.buf(W * H, np.uint32), 1
    for k, v in kw.items():
        setattr(o, k, v)
    return c.L.rt_render(c.u if unfinished else c.h, None if null else ctypes.byref(o), None)


def _accumulate(c, null=False, output=True, **kw):
    o = c.rt.AccumOpts()
    c.L.rt_accum_opts_default(ctypes.byref(o))
    o.host_outputs = 1
    if output:
        o.rgba = c.buf(W * H, np.uint32)
    for k, v in kw.items():
        setattr(o, k, v)
    n = ctypes.c_int(0)
    return c.L.rt_accumulate(c.h, None if null else ctypes.byref(o), ctypes.byref(n))


def _occlusion(c, null=False, output=True, **kw):
    o = c.rt.OcclusionOpts()
    c.L.rt_occlusion_opts_default(ctypes.byref(o))
    o.host_outputs = 1
    if output:
        o.visibility = c.buf(W * H)
    for k, v in kw.items():
        setattr(o, k, v)
    n = ctypes.c_int(0)
    return c.L.rt_occlusion(c.h, None if null else ctypes.byref(o), ctypes.byref(n))


def _query(c, null=False, n=1, rays=True, pixel=None, dir=True, outputs=("t",), **kw):
    """One host ray from the camera's side towards the scene, closest hit into `t`, unless told otherwise."""
    o = c.rt.QueryOpts()
    c.L.rt_query_opts_default(ctypes.byref(o))
    o.n, o.host = n, 1
    if rays:
        o.origin = c.buf(3)
        if dir:
            o.dir = c.buf(3, fill=1)
    if pixel is not None:
        o.pixel = c.buf(2, np.int32)
        c.keep[-1][:] = pixel
    for k in outputs:
        comps, dt = c.rt.QUERY_OUTPUTS[k]
        setattr(o, k, c.buf(comps, dt))
    for k, v in kw.items():
        setattr(o, k, v)
    return c.L.rt_query(c.h, None if null else ctypes.byref(o), None)


def _frame_work(c, **kw):
    o = c.rt.RenderOpts()
    c.L.rt_render_opts_default(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    w = c.rt.Work()
    return c.L.rt_frame_work(c.h, ctypes.byref(o), ctypes.byref(w))


def _experiment(c, which):
    ms = ctypes.c_double()
    return c.L.rt_experiment(c.h, which, 1, 1, ctypes.byref(ms), c.buf(22, np.uint64))


def _kat(c, op, n):
    return c.L.rt_kat_device(op, n, c.buf(3), None, None, c.buf(3), None, None)


# (entry, case, call).  CASES need no device anywhere: they run on every machine.
CASES = [
    ("rt_render", "null opts", lambda c: _render(c, null=True)),
    ("rt_render", "spp = 0", lambda c: _render(c, spp=0)),
    ("rt_accumulate", "null opts", lambda c: _accumulate(c, null=True)),
    ("rt_accumulate", "samples = 0", lambda c: _accumulate(c, samples=0)),
    ("rt_accumulate", "no output", lambda c: _accumulate(c, output=False)),
    ("rt_occlusion", "null opts", lambda c: _occlusion(c, null=True)),
    ("rt_occlusion", "samples = 0", lambda c: _occlusion(c, samples=0)),
    ("rt_occlusion", "radius = 0", lambda c: _occlusion(c, radius=0.0)),
    ("rt_occlusion", "bias = -1", lambda c: _occlusion(c, bias=-1.0)),
    ("rt_occlusion", "bias = inf", lambda c: _occlusion(c, bias=INF)),
    ("rt_occlusion", "no output", lambda c: _occlusion(c, output=False)),
    ("rt_query", "null opts", lambda c: _query(c, null=True)),
    ("rt_query", "n = -1", lambda c: _query(c, n=-1)),
    ("rt_query", "n = 0", lambda c: _query(c, n=0)),
    ("rt_query", "both pixel and origin", lambda c: _query(c, pixel=(1, 1))),
    ("rt_query", "origin without dir", lambda c: _query(c, dir=False)),
    ("rt_query", "any_hit without hit", lambda c: _query(c, any_hit=1)),
    ("rt_query", "no output", lambda c: _query(c, outputs=())),
    ("rt_query", "host = 1 with pixel (16, 0)", lambda c: _query(c, rays=False, pixel=(16, 0))),
    ("rt_accumulate_set_adaptive", "mode 2", lambda c: c.L.rt_accumulate_set_adaptive(c.h, 2, 0.03125)),
    ("rt_accumulate_set_adaptive", "threshold -1", lambda c: c.L.rt_accumulate_set_adaptive(c.h, 1, -1.0)),
    ("rt_accumulate_set_adaptive", "threshold NaN", lambda c: c.L.rt_accumulate_set_adaptive(c.h, 1, NAN)),
    ("rt_query_set_order", "mode 7", lambda c: c.L.rt_query_set_order(c.h, 7)),
    ("rt_ao_direction", "k = 1024", lambda c: c.L.rt_ao_direction(1024, c.buf(3))),
    ("rt_debug_cast", "pixel (16, 0)", lambda c: c.L.rt_debug_cast(c.h, 16, 0, ctypes.create_string_buffer(256), 256)),
    ("rt_frame_work", "spp = 65", lambda c: _frame_work(c, spp=65)),
    ("rt_experiment", "which = 0", lambda c: _experiment(c, 0)),
    ("rt_kat_device", "unknown op", lambda c: _kat(c, b"no_such_op", 1)),
    ("rt_kat_device", "n = 0", lambda c: _kat(c, b"cross", 0)),
    ("rt_query_last", "before any rt_query", lambda c: c.L.rt_query_last(c.h, c.buf(8, np.int32), c.buf(6), None, 0)),
    ("rt_occlusion_rays", "before any rt_occlusion", lambda c: c.L.rt_occlusion_rays(c.h, 0, c.buf(W * H * 6), W * H * 6)),
    ("rt_render", "unfinished scene", lambda c: _render(c, unfinished=True)),
]

# What a machine without a device answers: a valid call stops at the upload (RT_ERR_NODEV), and no
# trace launch has happened.  (Where a device exists, creating the scene renders a warm frame, so
# rt_scene_last_trace has a launch to report there: the case belongs here.)
CASES_NO_DEVICE = [
    ("rt_scene_last_trace", "before any trace launch", lambda c: c.L.rt_scene_last_trace(c.h, c.buf(8, np.int32))),
    ("rt_accumulate", "valid call, no device", lambda c: _accumulate(c)),
    ("rt_occlusion", "valid call, no device", lambda c: _occlusion(c)),
    ("rt_query", "valid call, no device", lambda c: _query(c)),
]


def run(rt, cases):
    c = _Ctx(rt)
    try:
        out = []
        for entry, case, call in cases:
            code = int(call(c))
            msg = None if code == rt.RT_OK else c.L.rt_last_error().decode()
            out.append({"entry": entry, "case": case, "code": code, "message": msg})
        return out
    finally:
        c.close()
