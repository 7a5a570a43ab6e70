// rt_adapt.h — adaptive refinement of rt_accumulate: the tile mapping and the per-pixel edge
// predicate, shared by accum_edge_kernel / accum_fold_tiles_kernel (rt_kernels.hip) and the host
// test (tests/adaptive_host.cpp): one definition, as rt_accum.h is for the fold.
// A tile is the pixel group of a whole-frame 1-spp launch (frame_geometry(W, H, 0, 1, 1): gw x gh
// pixels, n_tx tiles a row); tile g covers x in [gw (g % n_tx), +gw), y in [gh (g / n_tx), +gh),
// clipped to the canvas, and lane l of its wave is the pixel (l % gw, l / gw) of it, as
// group_lane maps a 1-spp launch.
// A pixel p is an edge pixel when some pixel q of its 8-neighbourhood inside the canvas has
// |c(p).ch - c(q).ch| > threshold in some channel, c = clamp1 of sample 0's raw radiance (what
// sum_c holds after sample 0's fold: 0 + clamp1(r0); -0 became +0, the differences are the same).
// Float32 subtraction, fabsf and a `>` compare: a NaN difference flags nothing.  A tile is needed
// when it contains an edge pixel; a contrast across a tile border flags both tiles.
#pragma once

#include <stdint.h>

#include "rt_accum.h"

namespace rtad {

using rtm::V4;

struct TileGrid { int W, H, gw, gh, gw_shift, n_tx, n_ty; };   // gw_shift: log2(gw), or -1
RT_HD TileGrid tile_grid(int W, int H, int gw, int gh) {
    TileGrid t{W, H, gw, gh, -1, (W + gw - 1) / gw, (H + gh - 1) / gh};
    for (int k = 0; k < 31; k++)
        if ((1 << k) == gw) t.gw_shift = k;
    return t;
}
RT_HD int n_tiles(const TileGrid& t) { return t.n_tx * t.n_ty; }

// Lane `lane` of tile g: its pixel; false outside the tile or the canvas (such a lane does not vote).
RT_HD bool tile_lane(const TileGrid& t, int g, int lane, int& x, int& y) {
    const int ty = g / t.n_tx, tx = g - ty * t.n_tx;
    const int lx = t.gw_shift >= 0 ? lane & (t.gw - 1) : lane % t.gw;
    const int ly = t.gw_shift >= 0 ? lane >> t.gw_shift : lane / t.gw;
    x = tx * t.gw + lx;
    y = ty * t.gh + ly;
    return ly < t.gh && x < t.W && y < t.H;
}

RT_HD bool contrast(V4 a, V4 b, float thr) {
    return fabsf(a.x - b.x) > thr || fabsf(a.y - b.y) > thr || fabsf(a.z - b.z) > thr || fabsf(a.w - b.w) > thr;
}

// c(x, y): the clamped sample-0 colour of a canvas pixel.
template <class C> RT_HD bool edge_pixel(const TileGrid& t, int x, int y, float thr, C c) {
    const V4 p = c(x, y);
    bool e = false;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if ((dx | dy) == 0 || qx < 0 || qy < 0 || qx >= t.W || qy >= t.H) continue;
            e = e || contrast(p, c(qx, qy), thr);
        }
    return e;
}

}  // namespace rtad
