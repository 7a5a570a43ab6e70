"""The numpy float32 restatement of csrc/rt_occl.h, shared by tests/test_occlusion_host.py and
tests/test_gpu_occlusion.py: the surface point, the facing, the tangent frame, a sample's origin
and raw direction, the resolve and (in float64) the direction table.  Every operation is one
float32 + - x / on float32 arrays, in rt_occl.h's order."""
import numpy as np

F = np.float32
AO_MAX_SAMPLES = 1024


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def dot(a, b):
    """rtm::dot: ((0 + x x) + y y) + z z."""
    s = F(0) + a[..., 0] * b[..., 0]
    s = s + a[..., 1] * b[..., 1]
    return s + a[..., 2] * b[..., 2]


def surface_point(o, d, t):
    return o + t[..., None] * d


def faced(n, d):
    flip = dot(n, d) > F(0)
    return np.where(flip[..., None], -n, n)


def tangent_frame(n):
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    s = np.copysign(F(1), nz).astype(np.float32)
    a = F(-1) / (s + nz)
    b = (nx * ny) * a
    t1 = np.stack([F(1) + ((s * nx) * nx) * a, s * b, -(s * nx)], axis=-1)
    t2 = np.stack([b, s + (ny * ny) * a, -ny], axis=-1)
    assert t1.dtype == np.float32 and t2.dtype == np.float32
    return t1, t2


def ray_origin(p, n, bias):
    return p + F(bias) * n


def raw_direction(n, t1, t2, dk):
    dk = f32(dk)
    dx, dy, dz = dk[..., 0:1], dk[..., 1:2], dk[..., 2:3]
    r = (dx * t1 + dy * t2) + dz * n
    assert r.dtype == np.float32
    return r


def sample_rays(o, d, t, nrm, dk, bias):
    """(origin, raw direction) of a sample with table entry dk, from rt_query's pixel-mode outputs."""
    o, d, t, nrm = f32(o), f32(d), f32(t), f32(nrm)
    p = surface_point(o, d, t)
    n = faced(nrm, d)
    t1, t2 = tangent_frame(n)
    return ray_origin(p, n, bias), raw_direction(n, t1, t2, dk)


def visibility(c, n):
    v = F(1) - np.asarray(c).astype(np.float32) / F(n)
    assert v.dtype == np.float32
    return v


def grey(vis):
    """rta::pack of (v, v, v, 1): Color's truncation to bytes."""
    b = (F(255) * f32(vis)).astype(np.uint8).astype(np.uint32)
    return ((b << 24) + (b << 16) + (b << 8) + np.uint32(255)).astype(np.uint32)


def table64():
    """The direction table in float64, before the rounding to float32."""
    k = np.arange(AO_MAX_SAMPLES, dtype=np.float64)
    u, v = k * 0.7548776662466927, k * 0.5698402909980532
    u, v = u - np.floor(u), v - np.floor(v)
    r, phi = np.sqrt(u), 2.0 * np.pi * v
    x, y = r * np.cos(phi), r * np.sin(phi)
    z = np.sqrt(np.maximum(0.0, 1.0 - x * x - y * y))
    return np.stack([x, y, z], axis=-1)
