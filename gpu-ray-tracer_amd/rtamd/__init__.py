"""rtamd — Python host side of the MI355X ray-tracing core.

Thin ctypes binding over the C ABI in include/rt_amd.h (librt_amd.so, built by
``make -C gpu-ray-tracer_amd``).  There is no CPU fallback: if the library or a
gfx950 device is missing, the calls raise.

Mirrors the reference's render-path API (wtzhang23/gpu-ray-tracer):
  Scene.load_json(path)          ~ procedural::gpu::generate (cube_world.h:20-23)
  Scene.builder(...) methods     ~ rtracer::SceneBuilder (scene_builder.h:29-117)
  Scene.update_scene(kd, opt)    ~ rtracer::gpu::update_scene (raytracer.h:18-22)
  Scene.debug_cast(x, y)         ~ rtracer::gpu::debug_cast (raytracer.h:21)
  Scene.render(...)              the spp / row-slice / device-output extension
  Scene.query(...) / pick(x, y)  closest hit or occlusion of caller-supplied rays (rt_query; the
                                 reference's cast_ray, scene.cu:42-73, which it never exposes)
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
LIB_PATH = os.environ.get("RTAMD_LIB", os.path.join(PKG, "librt_amd.so"))

RT_OK, RT_ERR_ARG, RT_ERR_IO, RT_ERR_PARSE, RT_ERR_HIP, RT_ERR_STATE, RT_ERR_NODEV, RT_ERR_LIMIT = 0, -1, -2, -3, -4, -5, -6, -7
EXPORTS = {"vertices": 0, "normals": 1, "tris": 2, "materials": 3, "instances": 4, "inst_mesh": 5,
           "lights": 6, "camera": 7, "env": 8, "texcoords": 9}
# RT_EXPORT_BVH_* (test hook): the tree the most recent frame's BVH build left on the device
BVH_EXPORTS = {"bvh_info": 11, "bvh_pairs": 12, "bvh_leaf_inst": 13, "bvh_fnode": 14}
BVH_INFO_KEYS = ("n_leaf", "n_inst", "n_real", "fdepth", "ftree", "form", "slot")

# Every symbol include/rt_amd.h declares (checked by tests/test_abi.py).
SYMBOLS = [
    "rt_abi_version", "rt_last_error", "rt_device_count", "rt_set_device", "rt_scene_load_json", "rt_scene_create",
    "rt_scene_free", "rt_builder_add_vertex", "rt_builder_create_mesh", "rt_builder_add_triangle",
    "rt_builder_add_trans", "rt_builder_set_trans", "rt_builder_build_cube", "rt_builder_add_point_light",
    "rt_builder_add_directional_light", "rt_builder_finish", "rt_scene_info", "rt_scene_export", "rt_camera_get",
    "rt_camera_set", "rt_camera_translate", "rt_camera_rotate", "rt_camera_axes", "rt_env_set",
    "rt_render_opts_default", "rt_render", "rt_update_scene", "rt_canvas_read", "rt_canvas_host_ptr",
    "rt_canvas_get_color", "rt_debug_cast", "rt_kat_device", "rt_spp_offset", "rt_timing_collect",
    "rt_builder_add_triangle_tex", "rt_builder_build_cube_tex", "rt_scene_set_atlas", "rt_scene_load_atlas",
    "rt_scene_atlas_info", "rt_scene_set_frame_slots", "rt_scene_set_overlap", "rt_frame_work",
    "rt_scene_set_devices", "rt_profile_marker", "rt_host_alloc", "rt_host_free", "rt_copy_to_host_async",
    "rt_copy_engines_warm", "rt_scene_last_trace", "rt_query_opts_default", "rt_query",
    "rt_query_set_order", "rt_query_last", "rt_shade_opts_default", "rt_shade", "rt_shade_last",
    "rt_accum_opts_default", "rt_accumulate", "rt_accumulate_reset", "rt_accumulate_info",
    "rt_accumulate_set_adaptive", "rt_accumulate_adaptive_info", "rt_accumulate_pass_fill", "rt_accumulate_pass_read",
    "rt_scene_history_info",
    "rt_occlusion_opts_default", "rt_occlusion", "rt_occlusion_reset", "rt_occlusion_info", "rt_ao_direction",
    "rt_occlusion_rays", "rt_occlusion_set_pattern", "rt_occlusion_set_filter", "rt_occlusion_config",
    "rt_occlusion_filter_timing",
    "rt_occlusion_set_history", "rt_occlusion_history_info", "rt_occlusion_history_weights", "rt_occlusion_history_timing",
    "rt_scene_set_shadow_hints", "rt_scene_shadow_hints_fill", "rt_scene_shadow_hint_code",
    "rt_scene_shadow_hint_counters", "rt_scene_shadow_hints_read",
    "rt_scene_set_near_first", "rt_scene_near_first_counters",
]
RT_NEAR_FIRST_OFF, RT_NEAR_FIRST_ON, RT_NEAR_FIRST_PROFILE = 0, 1, 2
RT_QUERY_ORDER_CALLER, RT_QUERY_ORDER_SORTED = 0, 1
RT_ADAPTIVE_THRESHOLD_DEFAULT = 8.0 / 255.0
RT_AO_MAX_SAMPLES, RT_AO_BIAS_DEFAULT = 1024, 1e-3
RT_AO_PATTERN_SHARED, RT_AO_PATTERN_INTERLEAVED = 0, 1
RT_AO_INTERLEAVED_MAX_SAMPLES = RT_AO_MAX_SAMPLES // 16
RT_AO_FILTER_NORMAL_DEFAULT, RT_AO_FILTER_PLANE_DEFAULT = 0.9, 1e-2
RT_AO_HISTORY_DEFAULT = 32
AO_PATTERNS = {"shared": RT_AO_PATTERN_SHARED, "interleaved": RT_AO_PATTERN_INTERLEAVED}
OCCL_MAPS = {-1: None, 0: "row", 1: "tile", 2: "class"}     # rt_occlusion_config's out4[3]


class RtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rt error %d: %s" % (code, msg))
        self.code = code


class RenderOpts(ctypes.Structure):
    _fields_ = [("spp", ctypes.c_int), ("use_bvh", ctypes.c_int), ("rebuild_bvh", ctypes.c_int),
                ("row0", ctypes.c_int), ("row_step", ctypes.c_int), ("compact", ctypes.c_int),
                ("kernel_dim", ctypes.c_int), ("stream", ctypes.c_void_p), ("rgba", ctypes.c_void_p),
                ("radiance", ctypes.c_void_p), ("hit_inst", ctypes.c_void_p), ("hit_tri", ctypes.c_void_p),
                ("sync", ctypes.c_int), ("host_outputs", ctypes.c_int), ("timing", ctypes.c_int),
                ("textures", ctypes.c_int)]


class AccumOpts(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_int), ("use_bvh", ctypes.c_int), ("rebuild_bvh", ctypes.c_int),
                ("textures", ctypes.c_int), ("restart", ctypes.c_int), ("host_outputs", ctypes.c_int),
                ("rgba", ctypes.c_void_p), ("radiance", ctypes.c_void_p), ("hit_inst", ctypes.c_void_p),
                ("hit_tri", ctypes.c_void_p)]


class OcclusionOpts(ctypes.Structure):
    _fields_ = [("samples", ctypes.c_int), ("radius", ctypes.c_float), ("bias", ctypes.c_float),
                ("use_bvh", ctypes.c_int), ("rebuild_bvh", ctypes.c_int), ("restart", ctypes.c_int),
                ("host_outputs", ctypes.c_int),
                ("visibility", ctypes.c_void_p), ("occluded", ctypes.c_void_p), ("rgba", ctypes.c_void_p)]


class QueryOpts(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("origin", ctypes.c_void_p), ("dir", ctypes.c_void_p), ("tmax", ctypes.c_void_p),
                ("pixel", ctypes.c_void_p), ("use_bvh", ctypes.c_int), ("rebuild_bvh", ctypes.c_int),
                ("any_hit", ctypes.c_int), ("host", ctypes.c_int),
                ("t", ctypes.c_void_p), ("inst", ctypes.c_void_p), ("tri", ctypes.c_void_p), ("uv", ctypes.c_void_p),
                ("normal", ctypes.c_void_p), ("hit", ctypes.c_void_p), ("rays_out", ctypes.c_void_p)]


# rt_query's outputs: name -> (components per ray, dtype)
QUERY_OUTPUTS = {"t": (1, np.float32), "inst": (1, np.int32), "tri": (1, np.int32), "uv": (2, np.float32),
                 "normal": (3, np.float32), "hit": (1, np.uint8), "rays_out": (6, np.float32)}


class ShadeOpts(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int64), ("origin", ctypes.c_void_p), ("dir", ctypes.c_void_p), ("pixel", ctypes.c_void_p),
                ("sample", ctypes.c_int), ("use_bvh", ctypes.c_int), ("rebuild_bvh", ctypes.c_int),
                ("textures", ctypes.c_int), ("order", ctypes.c_int), ("host", ctypes.c_int),
                ("radiance", ctypes.c_void_p), ("rgba", ctypes.c_void_p), ("rays_out", ctypes.c_void_p)]


# rt_shade's outputs: name -> (components per ray, dtype)
SHADE_OUTPUTS = {"radiance": (4, np.float32), "rgba": (1, np.uint32), "rays_out": (6, np.float32)}
SHADE_TREES = {0: "ordered", 1: "heap", 2: "brute"}         # rt_shade_last's TREE


class Stats(ctypes.Structure):
    _fields_ = [("rays", ctypes.c_uint64), ("nodes", ctypes.c_uint64), ("leaves", ctypes.c_uint64),
                ("tri_tests", ctypes.c_uint64), ("bvh_ms", ctypes.c_double), ("trace_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Work(ctypes.Structure):
    _fields_ = [("queries", ctypes.c_uint64), ("wave_queries", ctypes.c_uint64), ("pair_steps", ctypes.c_uint64),
                ("leaf_visits", ctypes.c_uint64), ("leaf_lanes", ctypes.c_uint64), ("tri_iters", ctypes.c_uint64),
                ("scene_bytes", ctypes.c_uint64),
                # query occupancy (ABI 3)
                ("lanes_primary", ctypes.c_uint64), ("lanes_secondary", ctypes.c_uint64),
                ("lanes_shadow", ctypes.c_uint64), ("lanes_unlit", ctypes.c_uint64),
                ("live_wave_queries", ctypes.c_uint64), ("live_lanes", ctypes.c_uint64),
                ("hist_wave_queries", ctypes.c_uint64 * 8), ("hist_pair_steps", ctypes.c_uint64 * 8),
                ("hist_leaf_visits", ctypes.c_uint64 * 8)]

    def as_dict(self):
        d = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            d[k] = [int(x) for x in v] if k.startswith("hist_") else int(v)
        return d


_lib = None


def lib():
    """Load librt_amd.so (once).  If torch is already imported, the library binds to
    torch's HIP runtime (same soname), so device pointers/streams are shared."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtError(RT_ERR_STATE, "librt_amd.so not built (%s): run `make -C gpu-ray-tracer_amd`" % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH)
    vp, ip, fp = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float)
    L.rt_last_error.restype = ctypes.c_char_p
    L.rt_scene_load_json.argtypes = [ctypes.c_char_p, ip, ip, ctypes.POINTER(vp)]
    L.rt_scene_create.argtypes = [ctypes.c_char_p, ctypes.POINTER(vp)]
    L.rt_scene_free.argtypes = [vp]
    L.rt_builder_add_vertex.argtypes = [vp, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ip)]
    L.rt_builder_create_mesh.argtypes = [vp, vp, vp, ctypes.POINTER(ip)]
    L.rt_builder_add_triangle.argtypes = [vp, ip, ip, ip, ip, vp]
    L.rt_builder_add_trans.argtypes = [vp, ip, ctypes.POINTER(ip)]
    L.rt_builder_set_trans.argtypes = [vp, ip, vp, vp]
    L.rt_builder_build_cube.argtypes = [vp, ctypes.c_float, vp, ctypes.POINTER(ip)]
    L.rt_builder_build_cube_tex.argtypes = [vp, ctypes.c_float, vp, vp, ctypes.POINTER(ip)]
    L.rt_builder_add_triangle_tex.argtypes = [vp, ip, ip, ip, ip, vp, vp]
    L.rt_scene_set_atlas.argtypes = [vp, vp, ip, ip]
    L.rt_scene_load_atlas.argtypes = [vp, ctypes.c_char_p]
    L.rt_scene_atlas_info.argtypes = [vp, vp]
    L.rt_builder_add_point_light.argtypes = [vp, vp, vp]
    L.rt_builder_add_directional_light.argtypes = [vp, vp, vp]
    L.rt_builder_finish.argtypes = [vp, ip, ip, ctypes.c_float, ctypes.c_float, vp, vp, vp, vp, ip]
    L.rt_scene_info.argtypes = [vp, vp]
    L.rt_scene_export.argtypes = [vp, ip, vp, ctypes.c_int64]
    L.rt_camera_get.argtypes = [vp, vp, vp]
    L.rt_camera_set.argtypes = [vp, vp, vp]
    L.rt_camera_translate.argtypes = [vp, vp]
    L.rt_camera_rotate.argtypes = [vp, vp]
    L.rt_camera_axes.argtypes = [vp, vp, vp, vp]
    L.rt_env_set.argtypes = [vp, vp, vp, ip]
    L.rt_render_opts_default.argtypes = [ctypes.POINTER(RenderOpts)]
    L.rt_render_opts_default.restype = None
    L.rt_render.argtypes = [vp, ctypes.POINTER(RenderOpts), ctypes.POINTER(Stats)]
    L.rt_update_scene.argtypes = [vp, ip, ip]
    L.rt_canvas_read.argtypes = [vp, vp, ctypes.c_int64]
    L.rt_canvas_host_ptr.argtypes = [vp]
    L.rt_canvas_host_ptr.restype = vp
    L.rt_canvas_get_color.argtypes = [vp, ip, ip, vp]
    L.rt_debug_cast.argtypes = [vp, ip, ip, ctypes.c_char_p, ctypes.c_int64]
    L.rt_kat_device.argtypes = [ctypes.c_char_p, ip, vp, vp, vp, vp, vp, vp]
    L.rt_spp_offset.argtypes = [ip, fp, fp]
    L.rt_set_device.argtypes = [ip]
    L.rt_timing_collect.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ip)]
    L.rt_device_count.argtypes = [ctypes.POINTER(ip)]
    L.rt_scene_set_frame_slots.argtypes = [vp, ip]
    L.rt_scene_set_overlap.argtypes = [vp, ip]
    L.rt_frame_work.argtypes = [vp, ctypes.POINTER(RenderOpts), ctypes.POINTER(Work)]
    L.rt_scene_set_devices.argtypes = [vp, vp, ip, ip]
    L.rt_scene_last_trace.argtypes = [vp, vp]
    if hasattr(L, "rt_scene_set_shadow_hints"):  # (absent from libraries before the occluder hints: A/B runs)
        L.rt_scene_set_shadow_hints.argtypes = [vp, ip]
        L.rt_scene_shadow_hints_fill.argtypes = [vp, ctypes.c_int32]
        L.rt_scene_shadow_hint_code.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_int32)]
        L.rt_scene_shadow_hint_counters.argtypes = [vp, vp]
        L.rt_scene_shadow_hints_read.argtypes = [vp, vp, ctypes.c_int64]
    if hasattr(L, "rt_scene_set_near_first"):   # (absent from libraries before nearer-child-first: A/B runs)
        L.rt_scene_set_near_first.argtypes = [vp, ip]
        L.rt_scene_near_first_counters.argtypes = [vp, vp]
    L.rt_query_opts_default.argtypes = [ctypes.POINTER(QueryOpts)]
    L.rt_query_opts_default.restype = None
    L.rt_query.argtypes = [vp, ctypes.POINTER(QueryOpts), ctypes.POINTER(Stats)]
    if hasattr(L, "rt_accumulate"):             # (absent from libraries before progressive refinement: A/B runs)
        L.rt_accum_opts_default.argtypes = [ctypes.POINTER(AccumOpts)]
        L.rt_accum_opts_default.restype = None
        L.rt_accumulate.argtypes = [vp, ctypes.POINTER(AccumOpts), ctypes.POINTER(ip)]
        L.rt_accumulate_reset.argtypes = [vp]
        L.rt_accumulate_info.argtypes = [vp, vp]
    if hasattr(L, "rt_accumulate_set_adaptive"):   # (absent from libraries before adaptive refinement: A/B runs)
        L.rt_accumulate_set_adaptive.argtypes = [vp, ip, ctypes.c_float]
        L.rt_accumulate_adaptive_info.argtypes = [vp, vp, fp, vp, ctypes.c_int64]
        L.rt_accumulate_pass_fill.argtypes = [vp, ctypes.c_uint32]
        L.rt_accumulate_pass_read.argtypes = [vp, vp, ctypes.c_int64]
        L.rt_scene_history_info.argtypes = [vp, vp]
    if hasattr(L, "rt_occlusion"):              # (absent from libraries before the occlusion pass: A/B runs)
        L.rt_occlusion_opts_default.argtypes = [ctypes.POINTER(OcclusionOpts)]
        L.rt_occlusion_opts_default.restype = None
        L.rt_occlusion.argtypes = [vp, ctypes.POINTER(OcclusionOpts), ctypes.POINTER(ip)]
        L.rt_occlusion_reset.argtypes = [vp]
        L.rt_occlusion_info.argtypes = [vp, vp]
        L.rt_ao_direction.argtypes = [ip, vp]
        L.rt_occlusion_rays.argtypes = [vp, ip, vp, ctypes.c_int64]
    if hasattr(L, "rt_occlusion_set_pattern"):  # (absent from libraries before the interleaved pattern: A/B runs)
        L.rt_occlusion_set_pattern.argtypes = [vp, ip]
        L.rt_occlusion_set_filter.argtypes = [vp, ip, ctypes.c_float, ctypes.c_float]
        L.rt_occlusion_config.argtypes = [vp, vp, vp]
        L.rt_occlusion_filter_timing.argtypes = [vp, ip, ctypes.POINTER(ctypes.c_float)]
    if hasattr(L, "rt_occlusion_set_history"):  # (absent from libraries before the history: A/B runs)
        L.rt_occlusion_set_history.argtypes = [vp, ip, ip, ctypes.c_float, ctypes.c_float]
        L.rt_occlusion_history_info.argtypes = [vp, vp, vp]
        L.rt_occlusion_history_weights.argtypes = [vp, vp, ctypes.c_int64]
        L.rt_occlusion_history_timing.argtypes = [vp, ip, vp]
    if hasattr(L, "rt_query_set_order"):        # (absent from libraries before the coherence sort: A/B runs)
        L.rt_query_set_order.argtypes = [vp, ip]
        L.rt_query_last.argtypes = [vp, vp, vp, vp, ctypes.c_int64]
    if hasattr(L, "rt_shade"):                  # (absent from libraries before rt_shade: A/B runs)
        L.rt_shade_opts_default.argtypes = [ctypes.POINTER(ShadeOpts)]
        L.rt_shade_opts_default.restype = None
        L.rt_shade.argtypes = [vp, ctypes.POINTER(ShadeOpts)]
        L.rt_shade_last.argtypes = [vp, vp]
    if hasattr(L, "rt_profile_marker"):         # (absent from libraries older than ABI 3's round 5: A/B runs)
        L.rt_profile_marker.argtypes = [ip, vp]
    if hasattr(L, "rt_copy_to_host_async"):     # ABI 4
        L.rt_host_alloc.argtypes = [ctypes.c_int64, ctypes.POINTER(vp)]
        L.rt_host_free.argtypes = [vp]
        L.rt_copy_to_host_async.argtypes = [vp, vp, ctypes.c_int64, vp]
        L.rt_copy_engines_warm.argtypes = [ctypes.POINTER(vp), ip]
    _lib = L
    return L


def _check(code):
    if code != RT_OK:
        raise RtError(code, lib().rt_last_error().decode(errors="replace"))


def _f(a, n=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if n is not None:
        assert a.size == n, (a.size, n)
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _ray_inputs(o, who, origins, dirs, pixels):
    """A batch of caller rays into o.pixel / o.origin / o.dir (QueryOpts, ShadeOpts): its size n and
    the arrays the pointers refer to, for the caller to keep alive across the call."""
    given = [(k, np.ascontiguousarray(a, dtype=dt).reshape(-1, c))
             for k, a, dt, c in (("pixel", pixels, np.int32, 2), ("origin", origins, np.float32, 3), ("dir", dirs, np.float32, 3))
             if a is not None]
    if not given:
        raise RtError(RT_ERR_ARG, who + ": give origins and dirs, or pixels")
    n = given[-1][1].shape[0]
    assert all(a.shape[0] == n for _, a in given), "origins and dirs differ in length"
    for k, a in given:
        setattr(o, k, _ptr(a))
    return n, [a for _, a in given]


def _ray_outputs(o, n, want, table):
    """A zeroed array per name in `want`, shaped by `table` (QUERY_OUTPUTS, SHADE_OUTPUTS), bound to o's field of that name."""
    out = {}
    for k in want:
        c, dt = table[k]
        out[k] = np.zeros((n, c) if c > 1 else (n,), dt)
        setattr(o, k, _ptr(out[k]))
    return out


def device_count():
    n = ctypes.c_int()
    _check(lib().rt_device_count(ctypes.byref(n)))
    return n.value


def set_device(d):
    _check(lib().rt_set_device(int(d)))


def spp_offset(k):
    dx, dy = ctypes.c_float(), ctypes.c_float()
    _check(lib().rt_spp_offset(k, ctypes.byref(dx), ctypes.byref(dy)))
    return dx.value, dy.value


def ao_direction(k):
    """Entry k of rt_occlusion's direction table, float32[3] (rt_ao_direction)."""
    d = np.zeros(3, np.float32)
    _check(lib().rt_ao_direction(int(k), _ptr(d)))
    return d


def profile_marker(tag, stream=None):
    """An empty marker kernel of `tag` workgroups on `stream` (an int hipStream_t, None = the
    default stream): tools/pmc_step.py finds a timed region between two markers."""
    if hasattr(lib(), "rt_profile_marker"):
        _check(lib().rt_profile_marker(int(tag), stream))


class HostBuffer:
    """Pinned host memory from rt_host_alloc (hipHostMalloc), viewed as a torch / numpy array.
    The frame's host copy lands here through a copy engine (copy_to_host_async)."""

    def __init__(self, shape, dtype=np.int32):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = ctypes.c_void_p()
        _check(lib().rt_host_alloc(self.nbytes, ctypes.byref(p)))
        self.ptr = p.value
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * self.nbytes).from_address(self.ptr)) \
            .view(self.dtype).reshape(self.shape)

    def tensor(self):
        import torch
        return torch.from_numpy(self.array)

    def free(self):
        if self.ptr:
            self.array = None
            _check(lib().rt_host_free(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def copy_to_host_async(host_ptr, dev_ptr, nbytes, stream=None):
    """Device -> pinned-host copy on a DMA copy engine, enqueued on `stream` (an int
    hipStream_t; None = the null stream).  No CU is used (rt_copy_to_host_async)."""
    _check(lib().rt_copy_to_host_async(host_ptr, dev_ptr, int(nbytes), stream))


def copy_engines_warm(streams):
    """Start the SDMA engines a host-copy pipeline will use: one gated copy from each of
    `streams` (int hipStream_t handles; rt_copy_engines_warm)."""
    arr = (ctypes.c_void_p * len(streams))(*streams)
    _check(lib().rt_copy_engines_warm(arr, len(streams)))


def material(Ke=(0, 0, 0, 0), Ka=(0, 0, 0, 0), Kd=(0, 0, 0, 0), Ks=(0, 0, 0, 0), Kt=(0, 0, 0, 0), Kr=(0, 0, 0, 0),
             alpha=0.0, eta=1.0):
    """material26 record (material.h:14-31)."""
    return np.array(list(Ke) + list(Ka) + list(Kd) + list(Ks) + list(Kt) + list(Kr) + [alpha, eta], np.float32)


class Scene:
    """A scene resident on one GPU (renv::gpu::Scene equivalent)."""

    def __init__(self, handle):
        self._h = handle
        self._info = None

    # ---- creation ----
    @classmethod
    def load_json(cls, path, width=0, height=0):
        h = ctypes.c_void_p()
        _check(lib().rt_scene_load_json(os.fspath(path).encode(), int(width), int(height), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def create(cls, atlas=""):
        h = ctypes.c_void_p()
        _check(lib().rt_scene_create(atlas.encode(), ctypes.byref(h)))
        return cls(h)

    def close(self):
        if self._h:
            lib().rt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- SceneBuilder ----
    def add_vertex(self, x, y, z):
        i = ctypes.c_int()
        _check(lib().rt_builder_add_vertex(self._h, x, y, z, ctypes.byref(i)))
        return i.value

    def create_mesh(self, pos=(0, 0, 0), quat=(0, 0, 0, 1)):
        i = ctypes.c_int()
        _check(lib().rt_builder_create_mesh(self._h, _ptr(_f(pos, 3)), _ptr(_f(quat, 4)), ctypes.byref(i)))
        return i.value

    def add_triangle(self, mesh, i0, i1, i2, mat):
        _check(lib().rt_builder_add_triangle(self._h, mesh, i0, i1, i2, _ptr(_f(mat, 26))))

    def add_trans(self, mesh):
        i = ctypes.c_int()
        _check(lib().rt_builder_add_trans(self._h, mesh, ctypes.byref(i)))
        return i.value

    def set_trans(self, t, pos=None, quat=None):
        _check(lib().rt_builder_set_trans(self._h, t, _ptr(None if pos is None else _f(pos, 3)),
                                          _ptr(None if quat is None else _f(quat, 4))))

    def build_cube(self, scale, mat, tile=None):
        """tile=(tx, ty, size): every face mapped onto that atlas square (textured mode)."""
        i = ctypes.c_int()
        if tile is None:
            _check(lib().rt_builder_build_cube(self._h, scale, _ptr(_f(mat, 26)), ctypes.byref(i)))
        else:
            _check(lib().rt_builder_build_cube_tex(self._h, scale, _ptr(_f(mat, 26)), _ptr(_f(tile, 3)),
                                                   ctypes.byref(i)))
        return i.value

    def add_triangle_tex(self, mesh, i0, i1, i2, mat, tex6):
        _check(lib().rt_builder_add_triangle_tex(self._h, mesh, i0, i1, i2, _ptr(_f(mat, 26)), _ptr(_f(tex6, 6))))

    # ---- texture atlas (textured shading mode) ----
    def load_atlas(self, path=None):
        _check(lib().rt_scene_load_atlas(self._h, None if path is None else path.encode()))

    def set_atlas(self, rgba8):
        a = np.ascontiguousarray(rgba8, dtype=np.uint8)
        assert a.ndim == 3 and a.shape[2] == 4
        _check(lib().rt_scene_set_atlas(self._h, _ptr(a), a.shape[1], a.shape[0]))

    def atlas(self):
        """The loaded atlas as (H, W, 4) uint8 (empty array if none)."""
        a = self.atlas_info()
        out = np.zeros((a["height"], a["width"], 4), np.uint8)
        if out.size:
            _check(lib().rt_scene_export(self._h, 10, _ptr(out), out.nbytes))
        return out

    def atlas_info(self):
        v = np.zeros(3, np.int32)
        _check(lib().rt_scene_atlas_info(self._h, _ptr(v)))
        return {"width": int(v[0]), "height": int(v[1]), "loaded": bool(v[2])}

    def add_point_light(self, pos, col):
        _check(lib().rt_builder_add_point_light(self._h, _ptr(_f(pos, 3)), _ptr(_f(col, 4))))

    def add_directional_light(self, d, col):
        _check(lib().rt_builder_add_directional_light(self._h, _ptr(_f(d, 3)), _ptr(_f(col, 4))))

    def finish(self, width, height, fov, unit, cam_pos=(0, 0, 0), cam_quat=(0, 0, 0, 1), dist_atten=(0, 0, 0),
               ambience=(0, 0, 0, 0), depth=0):
        _check(lib().rt_builder_finish(self._h, width, height, fov, unit, _ptr(_f(cam_pos, 3)), _ptr(_f(cam_quat, 4)),
                                       _ptr(_f(dist_atten, 3)), _ptr(_f(ambience, 4)), depth))
        self._info = None

    # ---- introspection ----
    def info(self):
        if self._info is None:
            c = np.zeros(10, np.int32)
            _check(lib().rt_scene_info(self._h, _ptr(c)))
            keys = ["W", "H", "n_vertices", "n_tris", "n_meshes", "n_instances", "n_lights", "n_point", "depth", "n_mats"]
            self._info = dict(zip(keys, [int(x) for x in c]))
        return self._info

    @property
    def width(self):
        return self.info()["W"]

    @property
    def height(self):
        return self.info()["H"]

    def export(self, what):
        """Host copies of the scene arrays.  "bvh_info" (a dict of BVH_INFO_KEYS), "bvh_pairs"
        ([n_leaf, 12] float32), "bvh_leaf_inst" ([n_leaf] int32) and "bvh_fnode" ([n_real - 1, 16]
        float32; words 12..15 are int32 refs) read the tree the most recent frame's BVH build left
        on the device (RT_EXPORT_BVH_*, a test hook); RT_ERR_STATE before any build."""
        if what in BVH_EXPORTS:
            v = np.zeros(8, np.int32)
            _check(lib().rt_scene_export(self._h, BVH_EXPORTS["bvh_info"], _ptr(v), v.nbytes))
            b = dict(zip(BVH_INFO_KEYS, (int(x) for x in v)))
            if what == "bvh_info":
                return b
            shp, dt = {"bvh_pairs": ((b["n_leaf"], 12), np.float32), "bvh_leaf_inst": ((b["n_leaf"],), np.int32),
                       "bvh_fnode": ((max(b["n_real"] - 1, 0), 16), np.float32)}[what]
            a = np.zeros(shp, dt)
            _check(lib().rt_scene_export(self._h, BVH_EXPORTS[what], _ptr(a), a.nbytes))
            return a
        i = self.info()
        shapes = {"vertices": ((i["n_vertices"], 3), np.float32), "normals": ((i["n_vertices"], 3), np.float32),
                  "tris": ((i["n_tris"], 4), np.int32), "materials": ((i["n_mats"], 26), np.float32),
                  "instances": ((i["n_instances"], 7), np.float32), "inst_mesh": ((i["n_instances"],), np.int32),
                  "lights": ((i["n_lights"], 8), np.float32), "camera": ((21,), np.float32), "env": ((7,), np.float32),
                  "texcoords": ((i["n_tris"], 7), np.float32)}
        shp, dt = shapes[what]
        a = np.zeros(shp, dt)
        _check(lib().rt_scene_export(self._h, EXPORTS[what], _ptr(a), a.nbytes))
        return a

    def arrays(self):
        return {k: self.export(k) for k in EXPORTS}

    # ---- camera / env ----
    def camera(self):
        p, q = np.zeros(3, np.float32), np.zeros(4, np.float32)
        _check(lib().rt_camera_get(self._h, _ptr(p), _ptr(q)))
        return p, q

    def set_camera(self, pos=None, quat=None):
        _check(lib().rt_camera_set(self._h, _ptr(None if pos is None else _f(pos, 3)),
                                   _ptr(None if quat is None else _f(quat, 4))))

    def translate_camera(self, d):
        _check(lib().rt_camera_translate(self._h, _ptr(_f(d, 3))))

    def rotate_camera(self, dq):
        _check(lib().rt_camera_rotate(self._h, _ptr(_f(dq, 4))))

    def camera_axes(self):
        r, u, f = np.zeros(3, np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
        _check(lib().rt_camera_axes(self._h, _ptr(r), _ptr(u), _ptr(f)))
        return r, u, f

    def set_env(self, ambience=None, dist_atten=None, depth=None):
        d = self.info()["depth"] if depth is None else depth
        _check(lib().rt_env_set(self._h, _ptr(None if ambience is None else _f(ambience, 4)),
                                _ptr(None if dist_atten is None else _f(dist_atten, 3)), int(d)))
        self._info = None

    # ---- rendering ----
    def render(self, spp=1, use_bvh=True, rebuild_bvh=True, row0=0, row_step=1, compact=False,
               want=("rgba",), stats=True, textures=False):
        """Render to host numpy arrays (outputs staged through device buffers)."""
        W, H = self.width, self.height
        rows = len(range(row0, H, row_step)) if compact else H
        o = RenderOpts()
        lib().rt_render_opts_default(ctypes.byref(o))
        o.spp, o.use_bvh, o.rebuild_bvh, o.row0, o.row_step, o.compact = spp, int(use_bvh), int(rebuild_bvh), row0, row_step, int(compact)
        o.host_outputs, o.sync, o.textures = 1, 1, int(textures)
        out = {}
        if "rgba" in want:
            out["rgba"] = np.zeros((rows, W), np.uint32)
            o.rgba = _ptr(out["rgba"])
        if "radiance" in want:
            out["radiance"] = np.zeros((rows, W, 4), np.float32)
            o.radiance = _ptr(out["radiance"])
        if "hit_inst" in want:
            out["hit_inst"] = np.full((rows, W), -1, np.int32)
            o.hit_inst = _ptr(out["hit_inst"])
        if "hit_tri" in want:
            out["hit_tri"] = np.full((rows, W), -1, np.int32)
            o.hit_tri = _ptr(out["hit_tri"])
        st = Stats()
        _check(lib().rt_render(self._h, ctypes.byref(o), ctypes.byref(st) if stats else None))
        if stats:
            out["stats"] = st.as_dict()
        return out

    def render_device(self, spp=1, use_bvh=True, rebuild_bvh=True, row0=0, row_step=1, compact=True,
                      rgba_ptr=None, radiance_ptr=None, hit_inst_ptr=None, hit_tri_ptr=None, stream=None,
                      sync=False, stats=False, timing=False, textures=False):
        """Render into caller-owned DEVICE buffers (e.g. torch tensors' data_ptr())."""
        o = RenderOpts()
        lib().rt_render_opts_default(ctypes.byref(o))
        o.spp, o.use_bvh, o.rebuild_bvh, o.row0, o.row_step, o.compact = spp, int(use_bvh), int(rebuild_bvh), row0, row_step, int(compact)
        o.rgba, o.radiance, o.hit_inst, o.hit_tri = rgba_ptr, radiance_ptr, hit_inst_ptr, hit_tri_ptr
        o.stream, o.sync, o.host_outputs, o.timing, o.textures = stream, int(sync), 0, int(timing), int(textures)
        st = Stats()
        _check(lib().rt_render(self._h, ctypes.byref(o), ctypes.byref(st) if stats else None))
        return st.as_dict() if stats else None

    # ---- progressive refinement (rt_accumulate) ----
    def _accum_opts(self, samples, restart, use_bvh, rebuild_bvh, textures):
        o = AccumOpts()
        lib().rt_accum_opts_default(ctypes.byref(o))
        o.samples, o.restart, o.use_bvh, o.rebuild_bvh, o.textures = int(samples), int(restart), int(use_bvh), int(rebuild_bvh), int(textures)
        return o

    def accumulate(self, samples=1, restart=False, use_bvh=True, rebuild_bvh=True, textures=False, want=("rgba",)):
        """Add `samples` samples per pixel to the scene's running sums and return the frame of all
        the samples held, as host numpy arrays, plus "n", their number: the frame render(spp=n)
        returns.  The sums start again by themselves when the camera, an instance, the environment,
        the atlas or `textures` changed (rt_accumulate); hit_inst / hit_tri are sample 0's."""
        W, H = self.width, self.height
        o = self._accum_opts(samples, restart, use_bvh, rebuild_bvh, textures)
        o.host_outputs = 1
        out = {}
        if "rgba" in want:
            out["rgba"] = np.zeros((H, W), np.uint32)
            o.rgba = _ptr(out["rgba"])
        if "radiance" in want:
            out["radiance"] = np.zeros((H, W, 4), np.float32)
            o.radiance = _ptr(out["radiance"])
        if "hit_inst" in want:
            out["hit_inst"] = np.full((H, W), -1, np.int32)
            o.hit_inst = _ptr(out["hit_inst"])
        if "hit_tri" in want:
            out["hit_tri"] = np.full((H, W), -1, np.int32)
            o.hit_tri = _ptr(out["hit_tri"])
        n = ctypes.c_int(0)
        _check(lib().rt_accumulate(self._h, ctypes.byref(o), ctypes.byref(n)))
        out["n"] = n.value
        return out

    def accumulate_device(self, samples=1, restart=False, use_bvh=True, rebuild_bvh=True, textures=False,
                          rgba_ptr=None, radiance_ptr=None, hit_inst_ptr=None, hit_tri_ptr=None):
        """accumulate into caller-owned DEVICE buffers (e.g. torch tensors' data_ptr()), complete on
        return; returns the number of samples held."""
        o = self._accum_opts(samples, restart, use_bvh, rebuild_bvh, textures)
        o.rgba, o.radiance, o.hit_inst, o.hit_tri = rgba_ptr, radiance_ptr, hit_inst_ptr, hit_tri_ptr
        n = ctypes.c_int(0)
        _check(lib().rt_accumulate(self._h, ctypes.byref(o), ctypes.byref(n)))
        return n.value

    def accumulate_reset(self):
        """Drop the accumulated samples (rt_accumulate_reset)."""
        _check(lib().rt_accumulate_reset(self._h))

    @property
    def accumulated(self):
        """(samples held, W, H, restarts so far) (rt_accumulate_info)."""
        a = np.zeros(4, np.int32)
        _check(lib().rt_accumulate_info(self._h, _ptr(a)))
        return tuple(int(x) for x in a)

    def set_accumulate_adaptive(self, on=True, threshold=RT_ADAPTIVE_THRESHOLD_DEFAULT):
        """Adaptive refinement (rt_accumulate_set_adaptive): after sample 0, accumulate() traces and
        folds further samples only for the tiles that have an edge at `threshold`; the other
        tiles keep the 1-spp frame.  Changing the mode or the threshold drops the samples held."""
        _check(lib().rt_accumulate_set_adaptive(self._h, 1 if on else 0, float(threshold)))

    def accumulate_tiles(self):
        """The adaptive mode's state (rt_accumulate_adaptive_info): {"mode", "threshold", "tile": (w, h),
        "need": bool[n_ty, n_tx] or None before a mask exists, "needed": tiles needed (-1: no mask),
        "traced": tiles the last pass's trace launch was given}."""
        o = np.zeros(8, np.int32)
        thr = ctypes.c_float()
        _check(lib().rt_accumulate_adaptive_info(self._h, _ptr(o), ctypes.byref(thr), None, 0))
        need = np.zeros((int(o[4]), int(o[3])), np.uint8)
        r = lib().rt_accumulate_adaptive_info(self._h, _ptr(o), None, _ptr(need), need.size)
        if r != RT_ERR_STATE:                                      # (RT_ERR_STATE: no mask yet)
            _check(r)
        need = need.astype(bool) if r == RT_OK else None
        return {"mode": int(o[0]), "threshold": float(thr.value), "tile": (int(o[1]), int(o[2])), "need": need,
                "needed": int(o[5]), "traced": int(o[6])}

    def _history_info(self):
        """Test hook: the current frame slot's scheduling-history state (rt_scene_history_info), a tuple of 12."""
        a = np.zeros(12, np.int32)
        _check(lib().rt_scene_history_info(self._h, _ptr(a)))
        return tuple(int(x) for x in a)

    def _accumulate_pass_fill(self, bits):
        """Test hook: the pass buffer filled with a 32-bit pattern (rt_accumulate_pass_fill)."""
        _check(lib().rt_accumulate_pass_fill(self._h, int(bits) & 0xffffffff))

    def _accumulate_pass_read(self):
        """Test hook: the pass buffer, (H, W, 4) float32 (rt_accumulate_pass_read)."""
        a = np.zeros((self.height, self.width, 4), np.float32)
        _check(lib().rt_accumulate_pass_read(self._h, _ptr(a), a.size))
        return a

    # ---- ambient occlusion (rt_occlusion) ----
    def _occlusion_opts(self, samples, radius, bias, restart, use_bvh, rebuild_bvh):
        o = OcclusionOpts()
        lib().rt_occlusion_opts_default(ctypes.byref(o))
        o.samples, o.radius, o.bias = int(samples), float(radius), float(bias)
        o.restart, o.use_bvh, o.rebuild_bvh = int(restart), int(use_bvh), int(rebuild_bvh)
        return o

    def occlusion(self, samples=1, radius=float("inf"), bias=RT_AO_BIAS_DEFAULT, restart=False, want=("visibility",),
                  use_bvh=True, rebuild_bvh=True):
        """Add `samples` occlusion directions per pixel and return the estimate over all the samples
        held, as host numpy arrays named in `want` ("visibility" float32, "occluded" int32, "rgba"
        uint32, each (H, W)), plus "n", their number.  The accumulation starts again by itself when
        the camera, an instance, `radius` or `bias` changed (rt_occlusion)."""
        W, H = self.width, self.height
        o = self._occlusion_opts(samples, radius, bias, restart, use_bvh, rebuild_bvh)
        o.host_outputs = 1
        out = {}
        for k, dt in (("visibility", np.float32), ("occluded", np.int32), ("rgba", np.uint32)):
            if k in want:
                out[k] = np.zeros((H, W), dt)
                setattr(o, k, _ptr(out[k]))
        n = ctypes.c_int(0)
        _check(lib().rt_occlusion(self._h, ctypes.byref(o), ctypes.byref(n)))
        out["n"] = n.value
        return out

    def occlusion_device(self, samples=1, radius=float("inf"), bias=RT_AO_BIAS_DEFAULT, restart=False, use_bvh=True,
                         rebuild_bvh=True, visibility_ptr=None, occluded_ptr=None, rgba_ptr=None):
        """occlusion into caller-owned DEVICE buffers (e.g. torch tensors' data_ptr()), complete on
        return; returns the number of samples held."""
        o = self._occlusion_opts(samples, radius, bias, restart, use_bvh, rebuild_bvh)
        o.visibility, o.occluded, o.rgba = visibility_ptr, occluded_ptr, rgba_ptr
        n = ctypes.c_int(0)
        _check(lib().rt_occlusion(self._h, ctypes.byref(o), ctypes.byref(n)))
        return n.value

    def occlusion_reset(self):
        """Drop the occlusion samples held (rt_occlusion_reset)."""
        _check(lib().rt_occlusion_reset(self._h))

    @property
    def occlusion_info(self):
        """(samples held, W, H, restarts so far) (rt_occlusion_info)."""
        a = np.zeros(4, np.int32)
        _check(lib().rt_occlusion_info(self._h, _ptr(a)))
        return tuple(int(x) for x in a)

    def set_occlusion_pattern(self, pattern):
        """"shared" (every pixel's sample k uses table entry k) or "interleaved" (entry 16 k + the
        pixel's class (x & 3) + 4 (y & 3); at most 64 samples).  A change drops the samples held
        (rt_occlusion_set_pattern)."""
        _check(lib().rt_occlusion_set_pattern(self._h, AO_PATTERNS[pattern] if isinstance(pattern, str) else int(pattern)))

    def set_occlusion_filter(self, on=True, normal_min=RT_AO_FILTER_NORMAL_DEFAULT, plane_tol=RT_AO_FILTER_PLANE_DEFAULT):
        """The filtered resolve on or off: visibility and rgba averaged over the taps of a 4 x 4
        window that lie on the centre's surface; the counts stay raw and nothing restarts
        (rt_occlusion_set_filter)."""
        _check(lib().rt_occlusion_set_filter(self._h, int(on), float(normal_min), float(plane_tol)))

    @property
    def occlusion_config(self):
        """{"pattern": "shared" | "interleaved", "filter": bool, "capacity": samples the pattern can
        hold, "map": "row" | "tile" | "class" of the last call or None, "normal_min", "plane_tol"}
        (rt_occlusion_config)."""
        a, f = np.zeros(4, np.int32), np.zeros(2, np.float32)
        _check(lib().rt_occlusion_config(self._h, _ptr(a), _ptr(f)))
        return {"pattern": "interleaved" if a[0] == RT_AO_PATTERN_INTERLEAVED else "shared", "filter": bool(a[1]),
                "capacity": int(a[2]), "map": OCCL_MAPS[int(a[3])], "normal_min": float(f[0]), "plane_tol": float(f[1])}

    def filter_timing(self, on=True):
        """Measurement hook: time occl_filter_kernel's dispatch of later filtered calls with start/stop
        events (or stop); returns the last timed dispatch's ms, < 0: none yet (rt_occlusion_filter_timing)."""
        ms = ctypes.c_float(-1.0)
        _check(lib().rt_occlusion_filter_timing(self._h, int(on), ctypes.byref(ms)))
        return ms.value

    def set_occlusion_history(self, on=True, max_history=RT_AO_HISTORY_DEFAULT, normal_min=RT_AO_FILTER_NORMAL_DEFAULT,
                              plane_tol=RT_AO_FILTER_PLANE_DEFAULT):
        """Keep the samples across camera moves: a call that finds only the camera changed seeds every
        pixel from the previous frame by reprojection (at most max_history samples carried) instead
        of starting again.  A change of `on` or `max_history` drops the samples held
        (rt_occlusion_set_history)."""
        _check(lib().rt_occlusion_set_history(self._h, int(on), int(max_history), float(normal_min), float(plane_tol)))

    @property
    def occlusion_history(self):
        """{"on", "max_history", "moves", "cursor": samples traced since the last drop, "n": samples
        since the last move or drop, "weighted": a move since the last drop, "normal_min", "plane_tol"}
        (rt_occlusion_history_info)."""
        a, f = np.zeros(8, np.int32), np.zeros(2, np.float32)
        _check(lib().rt_occlusion_history_info(self._h, _ptr(a), _ptr(f)))
        return {"on": bool(a[0]), "max_history": int(a[1]), "moves": int(a[2]), "cursor": int(a[3]), "n": int(a[4]),
                "weighted": bool(a[5]), "normal_min": float(f[0]), "plane_tol": float(f[1])}

    def _occlusion_history_weights(self):
        """Test hook: the per-pixel history weight n_h, (H, W) int32 (rt_occlusion_history_weights)."""
        a = np.zeros((self.height, self.width), np.int32)
        _check(lib().rt_occlusion_history_weights(self._h, _ptr(a), a.size))
        return a

    def history_timing(self, on=True):
        """Measurement hook: time the reproject and the per-pixel resolve dispatches of later calls
        by events; returns their last (reproject ms, resolve ms), < 0: none yet
        (rt_occlusion_history_timing)."""
        ms = np.full(2, -1.0, np.float32)
        _check(lib().rt_occlusion_history_timing(self._h, int(on), _ptr(ms)))
        return float(ms[0]), float(ms[1])

    def _occlusion_rays(self, k):
        """Test hook: the rays sample k traces for the current accumulation, (H, W, 6) float32:
        origin and raw direction, zeros where the primary misses (rt_occlusion_rays)."""
        a = np.zeros((self.height, self.width, 6), np.float32)
        _check(lib().rt_occlusion_rays(self._h, int(k), _ptr(a), a.size))
        return a

    def frame_work(self, spp=1, row0=0, row_step=1, compact=True, want_rgba=False):
        """What the fast kernels do for this frame (rt_frame_work): queries issued after the
        exact skips, wave-level traversal steps.  want_rgba: also the profiling frame itself,
        returned as (work, rgba)."""
        o = RenderOpts()
        lib().rt_render_opts_default(ctypes.byref(o))
        o.spp, o.row0, o.row_step, o.compact = spp, row0, row_step, int(compact)
        rgba = None
        if want_rgba:
            rows = len(range(row0, self.height, row_step)) if compact else self.height
            rgba = np.zeros((rows, self.width), np.uint32)
            o.rgba, o.host_outputs = _ptr(rgba), 1
        w = Work()
        _check(lib().rt_frame_work(self._h, ctypes.byref(o), ctypes.byref(w)))
        return (w.as_dict(), rgba) if want_rgba else w.as_dict()

    # ---- ray queries (rt_query) ----
    def set_query_order(self, mode):
        """RT_QUERY_ORDER_CALLER (0, default) or RT_QUERY_ORDER_SORTED (1): whether query / query_device
        sort a batch into coherent waves on the device before tracing it (rt_query_set_order).  The
        results are the same arrays either way; sorting pays for itself on incoherent batches."""
        _check(lib().rt_query_set_order(self._h, int(mode)))
        self._query_order = int(mode)

    def _query(self, o, st, reorder):
        """rt_query; reorder=True: in RT_QUERY_ORDER_SORTED for this call, the scene's mode restored after it."""
        before = getattr(self, "_query_order", RT_QUERY_ORDER_CALLER)
        if reorder:
            self.set_query_order(RT_QUERY_ORDER_SORTED)
        try:
            _check(lib().rt_query(self._h, ctypes.byref(o), ctypes.byref(st) if st is not None else None))
            if o.n > 0:                                        # (n = 0 returns before any launch)
                self._last_query_n = int(o.n)
        finally:
            if reorder:
                self.set_query_order(before)

    def query_last(self, want_order=False):
        """The scene's most recent rt_query (rt_query_last): its kernel's TREE / LDS / ANY / STATS, whether
        the ordered kernel ran, the form, the grid, whether the batch was sorted, and the keys' box;
        want_order: also "order", the sorted batch's ray order (None if it was not sorted)."""
        v, b = np.zeros(8, np.int32), np.zeros(6, np.float32)
        _check(lib().rt_query_last(self._h, _ptr(v), _ptr(b), None, 0))
        keys = ["tree", "lds", "any_hit", "counted", "ordered", "persistent", "blocks", "sorted"]
        d = dict(zip(keys, [int(x) for x in v]))
        d["bounds"] = b
        if want_order:
            d["order"] = None
            if d["sorted"]:
                n = getattr(self, "_last_query_n", 0)          # (the batch size of this object's last query)
                order = np.zeros(max(1, n), np.uint32)
                _check(lib().rt_query_last(self._h, None, None, _ptr(order), n))
                d["order"] = order[:n]
        return d

    def query(self, origins=None, dirs=None, pixels=None, tmax=None, any_hit=False, use_bvh=True, rebuild_bvh=True,
              want=("t", "inst", "tri"), stats=False, reorder=False):
        """Closest hit (or, any_hit, occlusion) of caller-supplied rays: origins / dirs (n, 3), or
        pixels (n, 2) for the camera's sample-0 rays.  Returns a dict of numpy arrays, one per
        name in `want` (QUERY_OUTPUTS; any_hit: "hit" and "rays_out" only), plus "stats" on request.
        reorder=True: this call runs in RT_QUERY_ORDER_SORTED (set_query_order), whatever the scene's mode."""
        o = QueryOpts()
        lib().rt_query_opts_default(ctypes.byref(o))
        n, keep = _ray_inputs(o, "query", origins, dirs, pixels)
        if tmax is not None:
            keep.append(_f(np.broadcast_to(np.asarray(tmax, np.float32), (n,)), n))
            o.tmax = _ptr(keep[-1])
        o.n, o.use_bvh, o.rebuild_bvh, o.any_hit, o.host = n, int(use_bvh), int(rebuild_bvh), int(any_hit), 1
        out = _ray_outputs(o, n, want, QUERY_OUTPUTS)
        st = Stats()
        self._query(o, st if stats else None, reorder)
        if stats:
            out["stats"] = st.as_dict()
        return out

    def query_device(self, n, origin_ptr=None, dir_ptr=None, pixel_ptr=None, tmax_ptr=None, any_hit=False, use_bvh=True,
                     rebuild_bvh=True, t_ptr=None, inst_ptr=None, tri_ptr=None, uv_ptr=None, normal_ptr=None,
                     hit_ptr=None, rays_out_ptr=None, stats=False, reorder=False):
        """rt_query on caller-owned DEVICE buffers (e.g. torch tensors' data_ptr()): float32
        origins / dirs / tmax, int32 pixels and ids, uint8 hit.  Returns when the results are written.
        reorder: as query's."""
        o = QueryOpts()
        lib().rt_query_opts_default(ctypes.byref(o))
        o.n, o.origin, o.dir, o.pixel, o.tmax = int(n), origin_ptr, dir_ptr, pixel_ptr, tmax_ptr
        o.use_bvh, o.rebuild_bvh, o.any_hit, o.host = int(use_bvh), int(rebuild_bvh), int(any_hit), 0
        o.t, o.inst, o.tri, o.uv, o.normal, o.hit, o.rays_out = t_ptr, inst_ptr, tri_ptr, uv_ptr, normal_ptr, hit_ptr, rays_out_ptr
        st = Stats()
        self._query(o, st if stats else None, reorder)
        return st.as_dict() if stats else None

    # ---- shading caller-supplied rays (rt_shade) ----
    def shade(self, origins=None, dirs=None, pixels=None, sample=0, textures=False, use_bvh=True, rebuild_bvh=True,
              reorder=False, want=("radiance",)):
        """What each ray sees (rt_shade): the integrator's radiance along caller-supplied rays, origins /
        dirs (n, 3), or along the camera's rays of sample `sample` of pixels (n, 2).  Returns a dict of
        numpy arrays, one per name in `want` (SHADE_OUTPUTS).  reorder=True: this call sorts the batch
        into coherent waves on the device first (RT_QUERY_ORDER_SORTED); the arrays are the same."""
        o = ShadeOpts()
        lib().rt_shade_opts_default(ctypes.byref(o))
        n, keep = _ray_inputs(o, "shade", origins, dirs, pixels)
        o.n, o.sample, o.textures, o.use_bvh, o.rebuild_bvh = n, int(sample), int(textures), int(use_bvh), int(rebuild_bvh)
        o.order, o.host = (RT_QUERY_ORDER_SORTED if reorder else RT_QUERY_ORDER_CALLER), 1
        out = _ray_outputs(o, n, want, SHADE_OUTPUTS)
        _check(lib().rt_shade(self._h, ctypes.byref(o)))
        return out

    def shade_device(self, n, origin_ptr=None, dir_ptr=None, pixel_ptr=None, sample=0, textures=False, use_bvh=True,
                     rebuild_bvh=True, reorder=False, radiance_ptr=None, rgba_ptr=None, rays_out_ptr=None):
        """rt_shade on caller-owned DEVICE buffers (e.g. torch tensors' data_ptr()): float32 origins /
        dirs / radiance / rays_out, int32 pixels, uint32 rgba.  Returns when the results are written."""
        o = ShadeOpts()
        lib().rt_shade_opts_default(ctypes.byref(o))
        o.n, o.origin, o.dir, o.pixel, o.sample = int(n), origin_ptr, dir_ptr, pixel_ptr, int(sample)
        o.textures, o.use_bvh, o.rebuild_bvh, o.host = int(textures), int(use_bvh), int(rebuild_bvh), 0
        o.order = RT_QUERY_ORDER_SORTED if reorder else RT_QUERY_ORDER_CALLER
        o.radiance, o.rgba, o.rays_out = radiance_ptr, rgba_ptr, rays_out_ptr
        _check(lib().rt_shade(self._h, ctypes.byref(o)))

    def shade_last(self):
        """The scene's most recent rt_shade (rt_shade_last): its kernel's NS / TREE / TEX, whether the
        batch was sorted, the grid and the batch size."""
        v = np.zeros(8, np.int32)
        _check(lib().rt_shade_last(self._h, _ptr(v)))
        return dict(zip(["ns", "tree", "tex", "sorted", "blocks", "n"], [int(x) for x in v[:6]]))

    def pick(self, x, y):
        """The instance under pixel (x, y): (inst, tri, t) of the camera's sample-0 ray, or
        (-1, -1, inf) for the sky."""
        r = self.query(pixels=[(int(x), int(y))])
        return int(r["inst"][0]), int(r["tri"][0]), float(r["t"][0])

    def last_trace(self):
        """The trace kernel of the scene's most recent trace launch (rt_scene_last_trace)."""
        v = np.zeros(8, np.int32)
        _check(lib().rt_scene_last_trace(self._h, _ptr(v)))
        keys = ["ns_bucket", "lds", "mode", "shm", "part_k", "sky", "sky_brute", "ftree"]
        return dict(zip(keys, [int(x) for x in v]))

    def set_shadow_hints(self, on):
        """Shadow-query occluder hints on (default) or off: the frame is the same either way
        (rt_scene_set_shadow_hints)."""
        _check(lib().rt_scene_set_shadow_hints(self._h, 1 if on else 0))

    def shadow_hints_fill(self, value):
        """Test hook: every entry of the hint table set to `value` (any int32), counters zeroed."""
        _check(lib().rt_scene_shadow_hints_fill(self._h, ctypes.c_int32(int(value) & 0xffffffff).value))

    def shadow_hint_code(self, inst):
        """Test hook: the table value naming instance `inst`'s leaf in the last built ordered tree (0: none)."""
        c = ctypes.c_int32()
        _check(lib().rt_scene_shadow_hint_code(self._h, int(inst), ctypes.byref(c)))
        return c.value

    def shadow_hints(self):
        """Test hook: the hint table, [n_inst, 16, 4] int32 (instance, triangle & 15, light & 3)."""
        n = self.shadow_hint_counters()["entries"]
        v = np.zeros(n, np.int32)
        _check(lib().rt_scene_shadow_hints_read(self._h, _ptr(v), n))
        return v.reshape(-1, 16, 4)

    def shadow_hint_counters(self):
        """Counters since the last fill: shadow wave queries of the hinted kernels, those given a
        seed, those ended by the seed; `entries`: the table's size (0: the scene has none)."""
        v = np.zeros(4, np.uint64)
        _check(lib().rt_scene_shadow_hint_counters(self._h, _ptr(v)))
        return dict(zip(("queries", "seeded", "ended", "entries"), [int(x) for x in v]))

    def set_near_first(self, mode):
        """Nearer child first in closest-hit queries: 0 off, 1 on (default), 2 on and in the
        profiling variant too; the frame is the same either way (rt_scene_set_near_first)."""
        _check(lib().rt_scene_set_near_first(self._h, int(mode)))

    def near_first_counters(self):
        """Counters since the last shadow_hints_fill: wave queries walked near-first, those walked
        again in the fixed order, pair steps that swapped."""
        v = np.zeros(3, np.uint64)
        _check(lib().rt_scene_near_first_counters(self._h, _ptr(v)))
        return dict(zip(("queries", "reruns", "swaps"), [int(x) for x in v]))

    def set_devices(self, devices, n_ranks=None):
        """Split every whole frame row-cyclically over `devices` from this process (n_ranks
        slices, RCCL gather to devices[0]; rt_scene_set_devices).  [d], 1 = back to one GPU."""
        d = np.ascontiguousarray(devices, np.int32)
        _check(lib().rt_scene_set_devices(self._h, _ptr(d), int(d.size), int(n_ranks or d.size)))

    def set_frame_slots(self, n):
        """1 (default) to 8: consecutive frames rotate through n copies of the per-frame
        state (BVH, work counters, scheduling history), so frames issued on different streams
        overlap (rt_scene_set_frame_slots)."""
        _check(lib().rt_scene_set_frame_slots(self._h, int(n)))

    def set_overlap(self, full, stream=False):
        """Grid of a frame issued while another frame of the scene runs (four or more slots): False =
        half the CUs (default; device-resident pipelines), True = every CU (pipelines that
        copy each frame to the host); stream=True: half the CUs for every frame, the first
        included, while frames are issued back to back (rt_scene_set_overlap)."""
        _check(lib().rt_scene_set_overlap(self._h, 2 if stream else 1 if full else 0))

    def timing_collect(self):
        a, b, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        _check(lib().rt_timing_collect(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return {"bvh_ms_total": a.value, "trace_ms_total": b.value, "frames": n.value}

    def update_scene(self, kernel_dim=16, optimize=True):
        _check(lib().rt_update_scene(self._h, kernel_dim, int(optimize)))

    def canvas(self):
        a = np.zeros((self.height, self.width), np.uint32)
        _check(lib().rt_canvas_read(self._h, _ptr(a), a.size))
        return a

    def get_color(self, x, y):
        c = np.zeros(4, np.uint8)
        _check(lib().rt_canvas_get_color(self._h, x, y, _ptr(c)))
        return tuple(int(v) for v in c)

    def debug_cast(self, x, y):
        buf = ctypes.create_string_buffer(1 << 16)
        _check(lib().rt_debug_cast(self._h, x, y, buf, len(buf)))
        return buf.value.decode().splitlines()


def kat_device(op, *inputs):
    """Evaluate a math primitive on the GPU (test hook; see rt_amd.h rt_kat_device)."""
    sizes = {"normalize3": (3, 0, 0), "cross": (3, 0, 0), "reflect": (3, 0, 0), "refract": (3, 1, 0),
             "quat_rotate": (3, 0, 0), "quat_inverse": (4, 0, 0), "quat_mul": (4, 0, 0), "tri_hit": (3, 1, 0),
             "ray_ctor": (6, 0, 0), "zorder": (0, 0, 1), "to_mat3": (9, 0, 0), "box_hit": (0, 1, 0), "pow": (1, 0, 0),
             "tri_hit_f": (3, 1, 0), "box_hit_f": (0, 1, 0), "box_pair": (0, 2, 0),
             "rcp_cr": (1, 0, 0), "sqrt_cr": (1, 0, 0), "box_from_local": (6, 1, 0), "box_merge": (6, 1, 0),
             "entity": (12, 0, 0), "ray_key": (0, 0, 1), "normalized_unit": (3, 0, 0), "unit_len_rcp": (2, 0, 0),
             "reflect_unit": (3, 0, 0), "reflect_pre_unit": (3, 0, 0)}
    nf, ni, nu = sizes[op]
    ins = [_f(a) for a in inputs] + [None] * (3 - len(inputs))
    n = inputs[0].shape[0]
    of = np.zeros((n, nf), np.float32) if nf else None
    oi = (np.zeros(n, np.int32) if ni == 1 else np.zeros((n, ni), np.int32)) if ni else None
    ou = np.zeros(n, np.uint64) if nu else None
    _check(lib().rt_kat_device(op.encode(), n, _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), _ptr(of), _ptr(oi), _ptr(ou)))
    res = [x for x in (of, oi, ou) if x is not None]
    return res[0] if len(res) == 1 else tuple(res)
