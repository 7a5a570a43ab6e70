"""The numpy restatement of rt_occlusion's history across camera moves (csrc/rt_occl.h: reproject,
history_seed, filtered_visibility_total; rt_occlusion_set_history), shared by
tests/test_occlusion_history_host.py and tests/test_gpu_occlusion_history.py.  Float steps are
single float32 operations in rt_occl.h's order (occl_lib.dot is rtm::dot); counts, weights and
their sums are integers."""
import numpy as np

import occl_filter_lib as fl
import occl_lib as ol

F = np.float32
HISTORY_DEFAULT = 32
NORMAL_DEFAULT, PLANE_DEFAULT = fl.NORMAL_DEFAULT, fl.PLANE_DEFAULT


def camera(export):
    """DCamera's fields from Scene.export("camera"): pos, rot, near, unit, W, H, r, u, f."""
    e = ol.f32(export)
    return {"pos": e[0:3], "near": e[7], "unit": e[8], "W": e[9], "H": e[10], "r": e[11:14], "u": e[14:17], "f": e[17:20]}


def reproject(p, cam):
    """rto::reproject on points p (..., 3): (front, on_canvas, qx, qy, cx, cy).  front: a > 0;
    on_canvas: front and 0 <= fx < W and 0 <= fy < H (float comparisons, a NaN rejects); qx, qy the
    source pixel where on_canvas (0 elsewhere)."""
    p = ol.f32(p)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        v = p - cam["pos"]
        a, sx, sy = ol.dot(v, cam["f"]), ol.dot(v, cam["r"]), ol.dot(v, cam["u"])
        front = a > F(0)
        gx, gy = (cam["near"] * sx) / a, (cam["near"] * sy) / a
        cx = gx * cam["unit"] + F(0.5) * cam["W"]
        cy = F(0.5) * cam["H"] - gy * cam["unit"]
        fx, fy = np.floor(cx + F(0.5)), np.floor(cy + F(0.5))
        assert fx.dtype == np.float32 and cx.dtype == np.float32
        on = front & (fx >= F(0)) & (fx < cam["W"]) & (fy >= F(0)) & (fy < cam["H"])
    qx = np.where(on, fx, F(0)).astype(np.int64)
    qy = np.where(on, fy, F(0)).astype(np.int64)
    return front, on, qx, qy, cx, cy


def seed(c, T, max_history):
    """rto::history_seed on int arrays: (c_h, n_h)."""
    c, T = np.asarray(c, np.int64), np.asarray(T, np.int64)
    Ts = np.maximum(T, 1)                                          # (T = 0 never takes the scaled branch)
    scaled = (c * max_history + Ts // 2) // Ts
    over = T > max_history
    return np.where(over, scaled, c).astype(np.int32), np.where(over, max_history, T).astype(np.int32)


def move(new, prev, cam_prev, n_prev, max_history, normal_min=NORMAL_DEFAULT, plane_tol=PLANE_DEFAULT):
    """The seed of every pixel of the new frame.  new: {"p", "n" (H, W, 3), "live" (H, W)};
    prev: the same plus "count" and "weight" (H, W) int32; n_prev: the previous frame's samples since
    its own move.  Returns (count (H, W) int32, weight (H, W) int32, census): census counts the live
    new pixels accepted and those rejected as behind the camera, off the canvas, onto a source that
    is not live, by the normal test and by the plane test (having passed the normal test)."""
    live = new["live"]
    H, W = live.shape
    front, on, qx, qy, _, _ = reproject(new["p"], cam_prev)
    pq, nq, live_q = prev["p"][qy, qx], prev["n"][qy, qx], prev["live"][qy, qx] & on
    ok, ok_n, ok_p = fl.accept(ol.f32(new["p"]), ol.f32(new["n"]), ol.f32(pq), ol.f32(nq), live_q, normal_min, plane_tol)
    ok &= live
    T = prev["weight"][qy, qx].astype(np.int64) + n_prev
    c_h, n_h = seed(prev["count"][qy, qx], T, max_history)
    census = {"live": int(live.sum()), "accepted": int(ok.sum()), "behind": int((live & ~front).sum()),
              "off_canvas": int((live & front & ~on).sum()), "not_live": int((live & on & ~live_q).sum()),
              "normal": int((live & live_q & ~ok_n).sum()), "plane": int((live & live_q & ok_n & ~ok_p).sum())}
    return np.where(ok, c_h, 0).astype(np.int32), np.where(ok, n_h, 0).astype(np.int32), census


def resolve(count, weight, n):
    """visibility = 1 - (float)count / (float)(n_h + n); count 0 where there is no primary hit, so 1 there."""
    v = F(1) - np.asarray(count).astype(np.float32) / (np.asarray(weight).astype(np.int64) + n).astype(np.float32)
    assert v.dtype == np.float32
    return v


def filtered(p, n, live, count, weight, n_samples, normal_min=NORMAL_DEFAULT, plane_tol=PLANE_DEFAULT):
    """The filtered resolve with per-pixel totals: S the sum of the accepted taps' counts, N the sum
    of their weight + n_samples, the centre included.  Returns (visibility, S, N)."""
    p, n = ol.f32(p), ol.f32(n)
    tot = np.asarray(weight).astype(np.int64) + n_samples
    S = np.where(live, count, 0).astype(np.int64)
    N = np.where(live, tot, 1).astype(np.int64)
    for dx, dy in fl.TAPS:
        if dx == 0 and dy == 0:
            continue
        live_q = fl._shift(live, dx, dy, False)
        ok = fl.accept(p, n, fl._shift(p, dx, dy, 0), fl._shift(n, dx, dy, 0), live_q, normal_min, plane_tol)[0] & live
        S += np.where(ok, fl._shift(np.asarray(count), dx, dy, 0), 0)
        N += np.where(ok, fl._shift(tot, dx, dy, 0), 0)
    vis = F(1) - S.astype(np.float32) / N.astype(np.float32)
    assert vis.dtype == np.float32
    return np.where(live, vis, F(1)).astype(np.float32), np.where(live, S, 0), np.where(live, N, 0)
