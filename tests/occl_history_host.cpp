// occl_history_host — rt_occlusion's history across camera moves on the host: the reprojection and
// the seed occl_reproject_kernel compiles (csrc/rt_occl.h: reproject, history_seed) and the two
// resolves with per-pixel totals (visibility, filtered_visibility_total), for
// tests/test_occlusion_history_host.py (beside occl_filter_host.cpp).
//
//   occl_history_host reproject IN OUT n
//        IN:  a DCamera (16 float32: pos, r, u, f, near, unit, W, H), then n points of 3 float32
//        OUT: n records of 3 int32: accepted by rto::reproject (0 / 1), qx, qy (-1, -1 when not)
//   occl_history_host seed IN OUT n max_history
//        IN:  n records of 2 int32: c, T        OUT: n records of 2 int32: c_h, n_h
//   occl_history_host resolve IN OUT n
//        IN:  n records of 2 int32: S, N        OUT: n records of 2 float32: visibility(S, N), filtered_visibility_total(S, N)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rt_device.h"

template <class T> static bool read_all(const char* path, std::vector<T>& v) {
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", path); return false; }
    const bool ok = std::fread(v.data(), sizeof(T), v.size(), f) == v.size();
    std::fclose(f);
    if (!ok) std::fprintf(stderr, "%s is too short\n", path);
    return ok;
}
static bool write_all(const char* path, const void* p, size_t bytes) {
    FILE* o = std::fopen(path, "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", path); return false; }
    const bool ok = std::fwrite(p, 1, bytes, o) == bytes;
    return std::fclose(o) == 0 && ok;
}

static_assert(sizeof(rt::DCamera) == 64, "16 words");

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "reproject")) {
        const int n = std::atoi(argv[4]);
        if (n < 1) return 2;
        std::vector<float> in(16 + (size_t)n * 3);
        if (!read_all(argv[2], in)) return 1;
        rt::DCamera cam;
        std::memcpy(&cam, in.data(), sizeof cam);
        std::vector<int32_t> out((size_t)n * 3);
        for (int i = 0; i < n; i++) {
            const float* p = &in[16 + (size_t)i * 3];
            int qx = -1, qy = -1;
            const bool ok = rto::reproject(rtm::v3(p[0], p[1], p[2]), cam, qx, qy);
            out[(size_t)i * 3] = ok ? 1 : 0;
            out[(size_t)i * 3 + 1] = ok ? qx : -1;
            out[(size_t)i * 3 + 2] = ok ? qy : -1;
        }
        return write_all(argv[3], out.data(), out.size() * 4) ? 0 : 1;
    }
    if (argc == 6 && !std::strcmp(argv[1], "seed")) {
        const int n = std::atoi(argv[4]), max_history = std::atoi(argv[5]);
        if (n < 1 || max_history < 1) return 2;
        std::vector<int32_t> in((size_t)n * 2), out((size_t)n * 2);
        if (!read_all(argv[2], in)) return 1;
        for (int i = 0; i < n; i++) {
            int c_h = -1, n_h = -1;
            rto::history_seed(in[2 * (size_t)i], in[2 * (size_t)i + 1], max_history, c_h, n_h);
            out[2 * (size_t)i] = c_h; out[2 * (size_t)i + 1] = n_h;
        }
        return write_all(argv[3], out.data(), out.size() * 4) ? 0 : 1;
    }
    if (argc == 5 && !std::strcmp(argv[1], "resolve")) {
        const int n = std::atoi(argv[4]);
        if (n < 1) return 2;
        std::vector<int32_t> in((size_t)n * 2);
        if (!read_all(argv[2], in)) return 1;
        std::vector<float> out((size_t)n * 2);
        for (int i = 0; i < n; i++) {
            out[2 * (size_t)i] = rto::visibility(in[2 * (size_t)i], in[2 * (size_t)i + 1]);
            out[2 * (size_t)i + 1] = rto::filtered_visibility_total(in[2 * (size_t)i], in[2 * (size_t)i + 1]);
        }
        return write_all(argv[3], out.data(), out.size() * 4) ? 0 : 1;
    }
    std::fprintf(stderr, "usage: occl_history_host reproject IN OUT n | seed IN OUT n max_history | resolve IN OUT n\n");
    return 2;
}
