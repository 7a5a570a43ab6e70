// occl_filter_host — the interleaved pattern and the filtered resolve of rt_occlusion on the host:
// the accept test and the resolve occl_filter_kernel compiles (csrc/rt_occl.h: filter_accept,
// filtered_visibility, pixel_class, interleaved_entry) walked over a canvas the way the kernel
// walks it, and occlusion_plan (csrc/rt_plan.h) with a pattern, for
// tests/test_occlusion_filter_host.py (beside occl_host.cpp / occl_plan_host.cpp).
//
//   occl_filter_host filter IN OUT W H n NORMAL_MIN_BITS PLANE_TOL_BITS
//        IN:  W * H records of 8 words: p[3] n[3] (float32), live, count (int32)
//        OUT: W * H records of 3 words: visibility (float32), S, m (int32; 0, 0 at a centre that is not live)
//        the two parameters as the decimal of their float32 bit patterns
//   occl_filter_host classes OUT W H k     OUT: W * H records of 2 int32: class, entry of sample k
//   occl_filter_host plan W H map pattern  ->  tree map n_waves block blocks pattern filter_bx filter_by default_interleaved_map
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_device.h"

static bool write_all(const char* path, const void* p, size_t bytes) {
    FILE* o = std::fopen(path, "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", path); return false; }
    const bool ok = std::fwrite(p, 1, bytes, o) == bytes;
    return std::fclose(o) == 0 && ok;
}
static float from_bits(const char* s) {
    const uint32_t b = (uint32_t)std::strtoul(s, nullptr, 10);
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

struct Rec { float p[3], n[3]; int32_t live, count; };
static_assert(sizeof(Rec) == 32, "8 words");

int main(int argc, char** argv) {
    if (argc == 9 && !std::strcmp(argv[1], "filter")) {
        const int W = std::atoi(argv[4]), H = std::atoi(argv[5]), n = std::atoi(argv[6]);
        const float normal_min = from_bits(argv[7]), plane_tol = from_bits(argv[8]);
        if (W < 1 || H < 1 || n < 1) return 2;
        std::vector<Rec> in((size_t)W * H);
        FILE* f = std::fopen(argv[2], "rb");
        if (!f || std::fread(in.data(), sizeof(Rec), in.size(), f) != in.size()) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
        std::fclose(f);
        std::vector<uint32_t> out((size_t)W * H * 3);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const Rec& c = in[(size_t)y * W + x];
                float vis = 1.0f;
                int S = 0, m = 0;
                if (c.live) {
                    const rtm::V3 pc = rtm::v3(c.p[0], c.p[1], c.p[2]), nc = rtm::v3(c.n[0], c.n[1], c.n[2]);
                    S = c.count; m = 1;
                    for (int dy = -rto::AO_FILTER_LO; dy <= rto::AO_FILTER_HI; dy++)
                        for (int dx = -rto::AO_FILTER_LO; dx <= rto::AO_FILTER_HI; dx++) {
                            const int qx = x + dx, qy = y + dy;
                            if ((dx == 0 && dy == 0) || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                            const Rec& q = in[(size_t)qy * W + qx];
                            if (rto::filter_accept(pc, nc, rtm::v3(q.p[0], q.p[1], q.p[2]), rtm::v3(q.n[0], q.n[1], q.n[2]), q.live != 0,
                                                   normal_min, plane_tol)) {
                                S += q.count; m++;
                            }
                        }
                    vis = rto::filtered_visibility(S, m, n);
                }
                uint32_t* o = &out[((size_t)y * W + x) * 3];
                std::memcpy(&o[0], &vis, 4);
                o[1] = (uint32_t)S; o[2] = (uint32_t)m;
            }
        return write_all(argv[3], out.data(), out.size() * 4) ? 0 : 1;
    }
    if (argc == 6 && !std::strcmp(argv[1], "classes")) {
        const int W = std::atoi(argv[3]), H = std::atoi(argv[4]), k = std::atoi(argv[5]);
        if (W < 1 || H < 1) return 2;
        std::vector<int32_t> out((size_t)W * H * 2);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const int c = rto::pixel_class(x, y);
                out[((size_t)y * W + x) * 2] = c;
                out[((size_t)y * W + x) * 2 + 1] = rto::interleaved_entry(k, c);
            }
        return write_all(argv[2], out.data(), out.size() * 4) ? 0 : 1;
    }
    if (argc == 6 && !std::strcmp(argv[1], "plan")) {
        rtd::SceneView S{};
        S.use_bvh = 1; S.n_leaf = 64; S.ftree = 1;
        const rtd::OcclPlan p = rtd::occlusion_plan(std::atoi(argv[2]), std::atoi(argv[3]), S, std::atoi(argv[4]), std::atoi(argv[5]));
        std::printf("%d %d %d %d %d %d %d %d %d\n", p.tree, p.map, p.n_waves, p.block, p.blocks, p.pattern, p.filter_bx, p.filter_by,
                    (int)rtd::RT_OCCL_MAP_INTERLEAVED_DEFAULT);
        return 0;
    }
    std::fprintf(stderr, "usage: occl_filter_host filter IN OUT W H n NMIN_BITS PTOL_BITS | classes OUT W H k | plan W H map pattern\n");
    return 2;
}
