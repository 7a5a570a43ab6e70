// adaptive_host — the tile criterion of rt_accumulate's adaptive mode (csrc/rt_adapt.h: tile_grid,
// tile_lane, edge_pixel) on the host, with the kernels' float rules: the definitions
// accum_edge_kernel compiles, walked as it walks them (one tile after the other, 64 lanes each,
// the lanes outside the canvas not voting).  tests/test_adaptive_host.py compares every byte with
// the numpy restatement (tests/adaptive_cases.py).
//
//   adaptive_host IN OUT W H GW GH THRESHOLD_BITS
//
// IN: W x H raw sample-0 radiance, float4 each.  Folded from zero as sample 0's fold does
// (rta::fold: sum_c = 0 + clamp1(r0)); the predicate reads sum_c.  OUT: n_tx * n_ty bytes, 1 = needed.
// Prints "n_tx n_ty needed".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_adapt.h"

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: adaptive_host IN OUT W H GW GH THRESHOLD_BITS\n"); return 2; }
    const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), gw = std::atoi(argv[5]), gh = std::atoi(argv[6]);
    const uint32_t bits = (uint32_t)std::strtoul(argv[7], nullptr, 0);
    float thr;
    std::memcpy(&thr, &bits, 4);
    if (W < 1 || H < 1 || gw < 1 || gh < 1 || gw * gh > 64) return 2;
    std::vector<rtm::V4> r0((size_t)W * H), sum_c((size_t)W * H);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(r0.data(), sizeof(rtm::V4), r0.size(), f) != r0.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    std::fclose(f);
    for (size_t i = 0; i < r0.size(); i++) {
        rtm::V4 a = rtm::v4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        rta::fold(a, b, r0[i]);
        sum_c[i] = b;
    }
    const rtad::TileGrid t = rtad::tile_grid(W, H, gw, gh);
    std::vector<uint8_t> need((size_t)rtad::n_tiles(t), 0);
    int needed = 0;
    for (int g = 0; g < rtad::n_tiles(t); g++) {
        bool any = false;
        for (int lane = 0; lane < 64; lane++) {
            int x, y;
            if (!rtad::tile_lane(t, g, lane, x, y)) continue;
            any = any || rtad::edge_pixel(t, x, y, thr, [&](int qx, int qy) { return sum_c[(size_t)qy * W + qx]; });
        }
        need[g] = any ? 1 : 0;
        needed += any;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(need.data(), 1, need.size(), o) != need.size() || std::fclose(o) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    std::printf("%d %d %d\n", t.n_tx, t.n_ty, needed);
    return 0;
}
