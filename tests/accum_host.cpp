// accum_host — the per-pixel arithmetic of rt_accumulate (csrc/rt_accum.h: fold, mean, pack)
// on the host, with the kernels' float rules: the definitions accum_fold_kernel and the trace
// kernel's resolve compile.  tests/test_accumulate_host.py compares every bit with numpy.
//
//   accum_host IN OUT N_PX N_MAX n1 n2 ...
//
// IN: N_MAX samples of N_PX pixels, float4 each, sample-major.  The samples are folded in order
// as accum_fold_kernel does (the sums of no samples are zero and are not read); after the first
// n_i samples (n_i ascending) one record goes to OUT: sum_r[N_PX] and sum_c[N_PX] (float4), the
// resolved rgba[N_PX] (uint32) and radiance[N_PX] (float4).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rt_accum.h"

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: accum_host IN OUT N_PX N_MAX n1 [n2 ...]\n"); return 2; }
    const long n_px = std::atol(argv[3]), n_max = std::atol(argv[4]);
    if (n_px < 1 || n_max < 1) return 2;
    std::vector<long> emit;
    for (int i = 5; i < argc; i++) {
        const long n = std::atol(argv[i]);
        if (n < 1 || n > n_max || (!emit.empty() && n <= emit.back())) { std::fprintf(stderr, "bad n %ld\n", n); return 2; }
        emit.push_back(n);
    }
    std::vector<rtm::V4> samples((size_t)n_px * n_max);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(samples.data(), sizeof(rtm::V4), samples.size(), f) != samples.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    std::fclose(f);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 1; }
    std::vector<rtm::V4> sum_r(n_px), sum_c(n_px), rad(n_px);
    std::vector<uint32_t> rgba(n_px);
    size_t next = 0;
    for (long k = 0; k < n_max && next < emit.size(); k++) {
        const bool resolve = k + 1 == emit[next];
        for (long i = 0; i < n_px; i++) {
            rtm::V4 a = rtm::v4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
            if (k > 0) { a = sum_r[i]; b = sum_c[i]; }
            rta::fold(a, b, samples[(size_t)k * n_px + i]);
            sum_r[i] = a; sum_c[i] = b;
            if (resolve) {
                rgba[i] = rta::resolve_rgba(b, (int)k + 1);
                rad[i] = rta::resolve_radiance(a, (int)k + 1);
            }
        }
        if (resolve) {
            std::fwrite(sum_r.data(), sizeof(rtm::V4), n_px, o);
            std::fwrite(sum_c.data(), sizeof(rtm::V4), n_px, o);
            std::fwrite(rgba.data(), sizeof(uint32_t), n_px, o);
            std::fwrite(rad.data(), sizeof(rtm::V4), n_px, o);
            next++;
        }
    }
    if (std::fclose(o) != 0) return 1;
    std::printf("%zu\n", next);
    return 0;
}
