"""The numpy restatement of the interleaved direction pattern and the filtered resolve of
rt_occlusion (csrc/rt_occl.h: pixel_class, interleaved_entry, filter_accept, filtered_visibility;
csrc/rt_plan.h: occlusion_plan's class map), shared by tests/test_occlusion_filter_host.py and
tests/test_gpu_occlusion_filter.py.  Float steps are single float32 operations in rt_occl.h's
order (occl_lib.dot is rtm::dot); the sums of counts are integers."""
import numpy as np

import occl_lib as ol

F = np.float32
SHARED, INTERLEAVED = 0, 1
ROW, TILE, CLASS = 0, 1, 2
INTERLEAVED_MAX_SAMPLES = ol.AO_MAX_SAMPLES // 16
NORMAL_DEFAULT, PLANE_DEFAULT = 0.9, 1e-2
TAPS = [(dx, dy) for dy in (-2, -1, 0, 1) for dx in (-2, -1, 0, 1)]


def pixel_class(W, H):
    """(H, W): c = (x & 3) + 4 (y & 3)."""
    y, x = np.mgrid[0:H, 0:W]
    return ((x & 3) + 4 * (y & 3)).astype(np.int32)


def entries(W, H, k):
    """(H, W): the table entry of sample k at every pixel in the interleaved pattern."""
    return 16 * k + pixel_class(W, H)


def class_plan(W, H):
    """occlusion_plan's class map: (waves, blocks) -- 16 waves a 32 x 32 region, 4 waves a block."""
    waves = 16 * ((W + 31) // 32) * ((H + 31) // 32)
    return waves, max(1, (waves + 3) // 4)


def class_pixel(W, H, g, lane):
    """The device pixel function of OCCL_MAP_CLASS: (row-major index or -1, class) of lane `lane` of wave g."""
    c, rg = g & 15, g >> 4
    n_rx = (W + 31) >> 5
    ry, rx = divmod(rg, n_rx)
    x, y = 32 * rx + 4 * (lane & 7) + (c & 3), 32 * ry + 4 * (lane >> 3) + (c >> 2)
    return (y * W + x if x < W and y < H else -1), c


def _shift(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx] inside the canvas, `fill` outside."""
    H, W = a.shape[:2]
    b = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    b[ys, xs] = a[yq, xq]
    return b


def accept(pc, nc, pq, nq, live_q, normal_min, plane_tol):
    """rto::filter_accept on arrays (..., 3): live, dot(nc, nq) >= normal_min, |dot(nc, pq - pc)| <= plane_tol;
    also the two partial verdicts, for the reasons' census."""
    with np.errstate(invalid="ignore", over="ignore"):
        ok_n = ol.dot(nc, nq) >= F(normal_min)
        e = pq - pc
        assert e.dtype == np.float32
        ok_p = np.abs(ol.dot(nc, e)) <= F(plane_tol)
    return live_q & ok_n & ok_p, ok_n, ok_p


def filtered(p, n, live, count, n_samples, normal_min=NORMAL_DEFAULT, plane_tol=PLANE_DEFAULT):
    """The filtered resolve: p, n (H, W, 3) float32 surface records, live (H, W) bool, count (H, W)
    int32, n_samples held.  Returns (visibility (H, W) float32, census, S, m): census counts, over
    live centres, the taps rejected as not live, by the normal test, by the plane test (having
    passed the normal test), and the centres whose window the canvas clips; S and m are the sum of
    the accepted taps' counts and their number (0 at a centre that is not live)."""
    p, n = ol.f32(p), ol.f32(n)
    H, W = live.shape
    S = np.where(live, count, 0).astype(np.int64)
    m = np.ones((H, W), np.int64)
    census = {"not_live": 0, "normal": 0, "plane": 0, "clipped": 0}
    inside = np.ones((H, W), bool)
    clipped = np.zeros((H, W), bool)
    for dx, dy in TAPS:
        if dx == 0 and dy == 0:
            continue
        in_q = _shift(inside, dx, dy, False)
        live_q = _shift(live, dx, dy, False)
        ok, ok_n, ok_p = accept(p, n, _shift(p, dx, dy, 0), _shift(n, dx, dy, 0), live_q, normal_min, plane_tol)
        ok &= live
        S += np.where(ok, _shift(count, dx, dy, 0), 0)
        m += ok
        clipped |= live & ~in_q
        census["not_live"] += int((live & in_q & ~live_q).sum())
        census["normal"] += int((live & live_q & ~ok_n).sum())
        census["plane"] += int((live & live_q & ok_n & ~ok_p).sum())
    census["clipped"] = int(clipped.sum())
    vis = F(1) - S.astype(np.float32) / (m * n_samples).astype(np.float32)
    assert vis.dtype == np.float32
    return np.where(live, vis, F(1)).astype(np.float32), census, np.where(live, S, 0).astype(np.int32), np.where(live, m, 0).astype(np.int32)
