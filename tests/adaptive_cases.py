"""Adaptive refinement (rt_accumulate_set_adaptive): the numpy restatement of the tile criterion
(csrc/rt_adapt.h) and the cases of tests/test_adaptive_host.py (CPU) and
tests/test_gpu_adaptive.py (device).  TEST INFRASTRUCTURE (may use the oracle).

The criterion: c = clamp1(sample 0's raw radiance), all four channels; a pixel is an edge pixel
when some pixel of its 8-neighbourhood inside the canvas differs from it by more than the
threshold in some channel (float32 subtraction, abs, `>`: a NaN difference flags nothing); a
tile (8 x 8 pixels, clipped to the canvas) is needed when it holds an edge pixel.

  stress        world8_stress 96 x 64 with the BVH                                      22 of 96 tiles
  stress_odd    world8_stress 50 x 37: partial tiles on both edges                      10 of 35
  world1_brute  world1 64 x 48 without the BVH (refractive)                              2 of 48
  media         the media scene of tests/integrator_cases.py, 48 x 32, depth 9
  sky           world8_stress 96 x 64, the camera turned away from the world: all zeros  0 of 96
  one_leaf      a builder scene of one cube, 24 x 16: the ordered tree is unusable (one leaf),
                so its kernel takes no tile lists and every pass traces every tile (the fallback)

NEEDED records each case's needed-tile count at 8/255 on the oracle's 1-spp frame."""
import numpy as np

import integrator_cases as ic
from conftest import scene_path
from twin import Twin

THRESHOLD = np.float32(8.0) / np.float32(255.0)
TILE = (8, 8)
# case -> (scene, W, H, use_bvh)
CASES = {"stress": ("world8_stress", 96, 64, True), "stress_odd": ("world8_stress", 50, 37, True),
         "world1_brute": ("world1", 64, 48, False), "media": (None, ic.SIZE[0], ic.SIZE[1], True),
         "sky": ("world8_stress", 96, 64, True), "one_leaf": (None, 24, 16, True)}
AWAY = (0.0, 1.0, 0.0, 0.0)             # half a turn about y: the camera looks away from the world
# needed tiles at THRESHOLD on the oracle's 1-spp frame (test_adaptive_host.py recomputes them)
NEEDED = {"stress": 22, "stress_odd": 10, "world1_brute": 2, "media": 23, "sky": 0, "one_leaf": 5}
# the cases whose nearest contrast is checked to lie clear of THRESHOLD (no tie between product and oracle)
MARGIN_CASES = ("stress", "stress_odd", "world1_brute")


def n_tiles(w, h, tile=TILE):
    return ((w + tile[0] - 1) // tile[0]) * ((h + tile[1] - 1) // tile[1])


def build_one_leaf(b, size=(24, 16)):
    m = ic.material(Ka=(0.2, 0.2, 0.2, 1), Kd=(0.7, 0.4, 0.2, 1), Ks=(0.3, 0.3, 0.3, 1), alpha=8.0)
    b.set_trans(b.add_trans(b.build_cube(1.0, m)), pos=(0.1, 0.0, 3.0))
    b.add_point_light((2.0, 3.0, -1.0), (1.0, 1.0, 1.0, 1.0))
    b.finish(size[0], size[1], ic.FOV, ic.UNIT, cam_pos=(0.0, 0.6, 0.0), cam_quat=(0.0995037, 0.0, 0.0, 0.9950372),
             dist_atten=ic.DIST_ATTEN, ambience=ic.AMBIENCE, depth=2)


def make(gpu, oracle, case):
    """A fresh (product scene or None, oracle scene or None, use_bvh) of the case; gpu / oracle may be None."""
    name, w, h, bvh = CASES[case]
    if name is None:
        if gpu is not None and oracle is not None:
            t = Twin(gpu, oracle)
            s, o, b = t.gpu, t.orc, t
        else:
            s = gpu.Scene.create("") if gpu is not None else None
            o = oracle.create() if oracle is not None else None
            b = s if s is not None else o
        if case == "media":
            ic.build(b, "media", depth=9)
        else:
            build_one_leaf(b, (w, h))
        return s, o, bvh
    s = gpu.Scene.load_json(scene_path(name), w, h) if gpu is not None else None
    o = oracle.load(scene_path(name), w, h) if oracle is not None else None
    if case == "sky":
        for x in (s, o):
            if x is not None:
                x.set_camera(quat=AWAY)
    return s, o, bvh


def clamp1(radiance):
    r = np.asarray(radiance, np.float32)
    return np.where(r > np.float32(1), np.float32(1), r)


def neighbour_contrast(radiance_hw4):
    """(H, W) float32: per pixel the largest |c(p).ch - c(q).ch| over its 8 neighbours inside the
    canvas and the channels (NaN differences left out; 0 without a neighbour)."""
    c = clamp1(radiance_hw4)
    h, w = c.shape[:2]
    out = np.zeros((h, w), np.float32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            ys, yd = slice(max(0, dy), h + min(0, dy)), slice(max(0, -dy), h + min(0, -dy))
            xs, xd = slice(max(0, dx), w + min(0, dx)), slice(max(0, -dx), w + min(0, -dx))
            with np.errstate(invalid="ignore"):
                d = np.abs(c[yd, xd] - c[ys, xs])                  # float32 - float32
            assert d.dtype == np.float32
            d = np.where(np.isnan(d), np.float32(0), d).max(axis=-1)
            out[yd, xd] = np.maximum(out[yd, xd], d)
    return out


def edge_pixels(radiance_hw4, threshold):
    c = clamp1(radiance_hw4)
    h, w = c.shape[:2]
    e = np.zeros((h, w), bool)
    thr = np.float32(threshold)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx == 0 and dy == 0:
                continue
            ys, yd = slice(max(0, dy), h + min(0, dy)), slice(max(0, -dy), h + min(0, -dy))
            xs, xd = slice(max(0, dx), w + min(0, dx)), slice(max(0, -dx), w + min(0, -dx))
            with np.errstate(invalid="ignore"):
                d = np.abs(c[yd, xd] - c[ys, xs])
                e[yd, xd] |= (d > thr).any(axis=-1)               # NaN > thr is False
    return e


def need_mask(radiance_hw4, threshold, tile=TILE):
    """bool[n_ty, n_tx]: the needed tiles of a frame whose sample-0 raw radiance is radiance_hw4."""
    e = edge_pixels(radiance_hw4, threshold)
    h, w = e.shape
    n_tx, n_ty = (w + tile[0] - 1) // tile[0], (h + tile[1] - 1) // tile[1]
    pad = np.zeros((n_ty * tile[1], n_tx * tile[0]), bool)
    pad[:h, :w] = e
    return pad.reshape(n_ty, tile[1], n_tx, tile[0]).any(axis=(1, 3))


def pixel_mask(need, w, h, tile=TILE):
    """bool[h, w]: the pixels of the needed tiles."""
    return np.repeat(np.repeat(need, tile[1], axis=0), tile[0], axis=1)[:h, :w]


def compose(need, fr_n, fr_1, keys=("rgba", "radiance")):
    """The adaptive frame: fr_n in the needed tiles' pixels, fr_1 elsewhere; hit ids are fr_1's (sample 0's)."""
    h, w = fr_1["rgba"].shape if "rgba" in fr_1 else fr_1["radiance"].shape[:2]
    m = pixel_mask(need, w, h)
    out = {}
    for k in keys:
        out[k] = np.where(m[..., None] if fr_n[k].ndim == 3 else m, fr_n[k], fr_1[k])
    for k in ("hit_inst", "hit_tri"):
        if k in fr_1:
            out[k] = fr_1[k]
    return out
