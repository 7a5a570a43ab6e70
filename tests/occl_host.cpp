// occl_host — the per-pixel arithmetic of rt_occlusion (csrc/rt_occl.h: surface point, facing,
// tangent frame, a sample's origin and raw direction, the resolve, the direction table) on the
// host, with the kernels' float rules: the definitions occl_surface_kernel, occlusion_kernel and
// occl_rays_kernel compile.  tests/test_occlusion_host.py compares every bit with numpy.
//
//   occl_host frame IN OUT N      IN: N records of 14 floats: o[3] d[3] t nrm[3] dk[3] bias
//                                 OUT: N records of 18 floats: p[3] n[3] t1[3] t2[3] origin[3] raw[3]
//   occl_host table OUT           OUT: RT_AO_MAX_SAMPLES entries of 3 floats
//   occl_host resolve OUT c n ... OUT: per (c, n) pair the visibility (float) and the grey word (uint32)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_occl.h"

static bool write_all(const char* path, const void* p, size_t bytes) {
    FILE* o = std::fopen(path, "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", path); return false; }
    const bool ok = std::fwrite(p, 1, bytes, o) == bytes;
    return std::fclose(o) == 0 && ok;
}

int main(int argc, char** argv) {
    if (argc >= 5 && !std::strcmp(argv[1], "frame")) {
        const long n = std::atol(argv[4]);
        if (n < 1) return 2;
        std::vector<float> in((size_t)n * 14), out((size_t)n * 18);
        FILE* f = std::fopen(argv[2], "rb");
        if (!f || std::fread(in.data(), sizeof(float), in.size(), f) != in.size()) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 1; }
        std::fclose(f);
        for (long i = 0; i < n; i++) {
            const float* r = &in[(size_t)i * 14];
            const rtm::V3 o = rtm::v3(r[0], r[1], r[2]), d = rtm::v3(r[3], r[4], r[5]), nrm = rtm::v3(r[7], r[8], r[9]);
            const rtm::V3 dk = rtm::v3(r[10], r[11], r[12]);
            const rto::Frame fr = rto::make_frame(rto::surface_point(o, d, r[6]), rto::faced(nrm, d));
            const rtm::V3 org = rto::ray_origin(fr, r[13]), raw = rto::raw_direction(fr, dk);
            const rtm::V3 v[6] = {fr.p, fr.n, fr.t1, fr.t2, org, raw};
            for (int k = 0; k < 6; k++) { float* w = &out[(size_t)i * 18 + 3 * k]; w[0] = v[k].x; w[1] = v[k].y; w[2] = v[k].z; }
        }
        return write_all(argv[3], out.data(), out.size() * sizeof(float)) ? 0 : 1;
    }
    if (argc == 3 && !std::strcmp(argv[1], "table")) {
        std::vector<float> t((size_t)rto::AO_MAX_SAMPLES * 3);
        for (int k = 0; k < rto::AO_MAX_SAMPLES; k++) rto::ao_direction(k, &t[(size_t)3 * k]);
        return write_all(argv[2], t.data(), t.size() * sizeof(float)) ? 0 : 1;
    }
    if (argc >= 5 && (argc - 3) % 2 == 0 && !std::strcmp(argv[1], "resolve")) {
        std::vector<uint32_t> out;
        for (int i = 3; i + 1 < argc; i += 2) {
            const int c = std::atoi(argv[i]), n = std::atoi(argv[i + 1]);
            if (n < 1 || c < 0 || c > n) { std::fprintf(stderr, "bad pair %d %d\n", c, n); return 2; }
            const float vis = rto::visibility(c, n);
            uint32_t bits;
            std::memcpy(&bits, &vis, 4);
            out.push_back(bits);
            out.push_back(rto::grey(vis));
        }
        return write_all(argv[2], out.data(), out.size() * sizeof(uint32_t)) ? 0 : 1;
    }
    std::fprintf(stderr, "usage: occl_host frame IN OUT N | table OUT | resolve OUT c n [c n ...]\n");
    return 2;
}
