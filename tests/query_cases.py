"""Shared pieces of the ray-query tests (tests/test_query_host.py, tests/test_gpu_query.py): the
camera of the value check, the camera's sample-0 rays restated in numpy float32, the float64
hit values of a (ray, instance, triangle) and the reference-arithmetic yardstick for them.
TEST INFRASTRUCTURE (may use the oracle)."""
import numpy as np

# The value check (world8_stress, pure translations) at 96 x 64, from a camera above the near edge
# looking 45 degrees down: 94% of its pixels hit (the scene file's own camera: 16%), the rest are sky.
VALUES_SCENE, VALUES_SIZE = "world8_stress", (96, 64)
VALUES_CAMERA = ((0.37, 9.0, -6.3), (0.3826834, 0.0, 0.0, 0.9238795))
# Rays whose world-space known-answer test reports a miss (edge cases of that formulation: the
# product tests the triangle in instance-local space) are left out of the value check; the cap.
KAT_MISS_CAP = 0.01
PERM_SEED, DROPPED = 20240607, 37     # the fixed permutation of the incoherent-packet cases


def all_pixels(W, H):
    """(W H, 2) int32 pixel list (x, y) in frame order."""
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([x.ravel(), y.ravel()], axis=1).astype(np.int32)


def normalized32(v):
    """rmath::Vec::normalized (linear.h:159-167) in float32: 0 + x x + y y + z z, sqrt, (1 / len) v."""
    v = np.asarray(v, np.float32)
    s = np.float32(0) + v[:, 0] * v[:, 0]
    s = s + v[:, 1] * v[:, 1]
    s = s + v[:, 2] * v[:, 2]
    ln = np.sqrt(s, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (np.float32(1) / ln)[:, None] * v
    out[~(ln > np.float32(1e-5))] = 0
    return out.astype(np.float32)


def camera_rays(cam21, pixels):
    """Camera::at (camera.cu:33-42) for integer pixels, from export("camera") = pos(3) quat(4)
    near unit W H r(3) u(3) f(3): (n, 6) float32 origin and normalised direction."""
    c = np.asarray(cam21, np.float32)
    pos, near, unit, W, H = c[0:3], c[7], c[8], c[9], c[10]
    r, u, f = c[11:14], c[14:17], c[17:20]
    px = np.asarray(pixels, np.int32)
    gx = ((px[:, 0].astype(np.float32) - np.float32(0.5) * W) / unit).astype(np.float32)
    gy = ((np.float32(0.5) * H - px[:, 1].astype(np.float32)) / unit).astype(np.float32)
    d = (near * f)[None, :] + gx[:, None] * r[None, :]
    d = (d + gy[:, None] * u[None, :]).astype(np.float32)
    return np.concatenate([np.broadcast_to(pos, d.shape), normalized32(d)], axis=1).astype(np.float32)


def world_triangles(arrays, inst, tri):
    """(n, 3, 3) float32 corners of triangle tri[i] of instance inst[i] moved to world space
    (pure translations: corner + instance position, one float32 add) and the same in float64 (exact sum)."""
    v, t, pos = arrays["vertices"], arrays["tris"], arrays["instances"][:, 4:7]
    corners = v[t[tri, 0:3]]                                   # (n, 3, 3)
    p = pos[inst][:, None, :]
    return (corners + p).astype(np.float32), corners.astype(np.float64) + p.astype(np.float64)


def values64(tri64, rays):
    """t, u, v of geometry.h:229-290 in float64: plane time, then the area ratios of vertices 1 and 2."""
    a, b, c = tri64[:, 0], tri64[:, 1], tri64[:, 2]
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    n = np.cross(b - a, c - a)
    area = np.linalg.norm(n, axis=1)
    t = np.einsum("ij,ij->i", a - o, n) / np.einsum("ij,ij->i", d, n)
    p = o + t[:, None] * d
    u = np.linalg.norm(np.cross(c - p, a - p), axis=1) / area
    v = np.linalg.norm(np.cross(a - p, b - p), axis=1) / area
    return t, u, v


def normals64(arrays, inst, tri, u, v):
    """The interpolated vertex normal (trimesh.cu:58-65) in float64, unit length (pure translations)."""
    nv, t = arrays["normals"].astype(np.float64), arrays["tris"]
    n0, n1, n2 = nv[t[tri, 0]], nv[t[tri, 1]], nv[t[tri, 2]]
    n = (1.0 - u - v)[:, None] * n0 + u[:, None] * n1 + v[:, None] * n2
    return n / np.linalg.norm(n, axis=1)[:, None]


def kat_yardstick(oracle, arrays, rays, inst, tri):
    """The reference's own arithmetic on the world-space triangle (oracle.kat("tri_hit")) against
    float64: (kept mask, e_ref, (t64, u64, v64)).  e_ref = its largest deviation from the float64
    values over the kept rays, t scaled by max(1, |t|): the float32 noise floor."""
    tri32, tri64 = world_triangles(arrays, inst, tri)
    hit, tuv = oracle.kat("tri_hit", tri32.reshape(-1, 9), rays)
    t64, u64, v64 = values64(tri64, rays)
    keep = hit != 0
    dev = np.stack([np.abs(tuv[:, 0] - t64) / np.maximum(1.0, np.abs(t64)), np.abs(tuv[:, 1] - u64), np.abs(tuv[:, 2] - v64)])
    return keep, float(dev[:, keep].max()), (t64, u64, v64)
